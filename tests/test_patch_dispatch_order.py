"""GPU tests (-m gpu) of the dispatch order of the per-layer patch launches (option VRT_PATCH_ORDER, voronoirt_amd/csrc/
vrt_patch.hip: patch_block_of).  Order 1 (share-major) starts every item's longest share of wavelength-pair steps first;
order 0 keeps an item's workgroups side by side.  The same workgroup program runs on the same (patch, angle, pair)
triples -- only which block of the grid carries which triple changes -- so J, J_up, J_down and every angle's I under order 1
must be BIT FOR BIT those under order 0, through the caller-layout entry and the sweep-order entry, and both are the
oracle's: fp64 storage element-wise to 1e-10 (oracle/parity.py), fp32 storage held to the storage-model oracle as
tests/test_patch_launch_edges.py holds it (the model's floats bit for bit in >= 99.9 % of the elements, within 2 float
ulps in the rest), not to 1e-10.

The grid is a body-centred lattice of 2 x 18 x 18 x 6 = 3 888 sites whose layers (648 sites) need two 512-entry patches per
angle: six angles per direction x two patches = twelve work-list slots, hence two rows of eight per launch (asserted from
the plan's own account), so that under order 1 a grid row's split and work-list row both vary.  Per-layer launches are
forced (VRT_PATCH_CHAIN=0) with three workgroups per item (VRT_PATCH_SPLIT=3)."""
import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from oracle.f32_model import PATH_MODEL, draw_case, within_conditions
from oracle.parity import rel as _rel
from voronoirt_amd import _lib, synth

pytestmark = pytest.mark.gpu

RTOL = 1e-10
W, TH, PH, NQ = vrt.read_quadrature("ul7n12.dat")
UP = [i for i in range(NQ) if TH[i] > 90]
ANGLES = {"ul7n12": list(range(NQ)), "up-only": UP}
WHAT = ("J", "I", "J_up", "J_down")


@pytest.fixture(scope="module")
def lattice():
    pos, nbr, bounds = synth.bcc_grid(18, 6, seed=7)
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    yield hs, orc.make_sites(pos, nbr, bounds)
    hs.close()


_refs = {}


def _reference(so, angles, nlam, f32):
    """inputs and (J, I, J_up, J_down) of the oracle, once per (angles, nlam, storage) and read-only"""
    key = (angles, nlam, f32)
    if key not in _refs:
        idx = ANGLES[angles]
        S, al, I0u, I0d = draw_case(so, nlam, seed=300 + nlam)
        f = lambda a: np.asarray(a, dtype=np.float64)
        model = PATH_MODEL["patches"] if f32 else {}
        out = orc.J_voronoi_model(W[idx], TH[idx], PH[idx], f(S), f(al), so, I0_up=f(I0u), I0_down=f(I0d), nthreads=8, **model)
        for a in out:
            a.setflags(write=False)
        _refs[key] = ((S, al, I0u, I0d), out)
    return _refs[key]


def _run(plan, w, n, nlam, f32, inputs):
    """J, I through the caller-layout entry (execute_dev) and J_up, J_down through the sweep-order entry
    (execute_native_dev, brought back to (n, nlam)) of the plan as its options stand"""
    import torch
    nq = len(w)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    dt = torch.float32 if f32 else torch.float64
    Sd, Ad, Ud, Dd = (torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt).contiguous() for x in inputs)
    Jd = torch.full((n, nlam), float("nan"), dtype=dt, device=dev)
    Id = torch.full((nq, n, nlam), float("nan"), dtype=dt, device=dev)
    plan.execute_dev(nlam, nlam, Sd.data_ptr(), Ad.data_ptr(), _lib.ALPHA_SITE_LAM, w, dJ=Jd.data_ptr(),
                     dI0_up=Ud.data_ptr(), dI0_down=Dd.data_ptr(), dI_out=Id.data_ptr(), stream=st, f32=f32)
    torch.cuda.synchronize()
    plan.check()
    assert plan.last_path == "patches"
    assert plan.last_launches > 1                       # per-layer launches, not the chained one
    cnt = plan.native_plane_count(nlam)
    size = 4 if f32 else 8
    S_nat = [torch.empty(cnt, dtype=dt, device=dev) for _ in range(2)]
    A_nat = torch.empty(2 * cnt, dtype=dt, device=dev)
    J_nat = [torch.full((cnt,), float("nan"), dtype=dt, device=dev) for _ in range(2)]
    plan.to_native_dev(nlam, nlam, Sd.data_ptr(), S_nat[0].data_ptr(), S_nat[1].data_ptr(), stream=st, f32=f32)
    plan.to_native_dev(nlam, nlam, Ad.data_ptr(), A_nat.data_ptr(), A_nat.data_ptr() + size * cnt, stream=st, f32=f32)
    plan.execute_native_dev(nlam, S_nat[0].data_ptr(), S_nat[1].data_ptr(), A_nat.data_ptr(), _lib.ALPHA_SITE_LAM_NATIVE,
                            w, dJ_up=J_nat[0].data_ptr(), dJ_down=J_nat[1].data_ptr(), dI0_up=Ud.data_ptr(),
                            dI0_down=Dd.data_ptr(), stream=st, f32=f32)
    assert plan.last_launches > 1
    Jdir = [torch.full((n, nlam), float("nan"), dtype=dt, device=dev) for _ in range(2)]
    plan.from_native_dev(1, nlam, nlam, J_nat[0].data_ptr(), Jdir[0].data_ptr(), stream=st, f32=f32)
    plan.from_native_dev(-1, nlam, nlam, J_nat[1].data_ptr(), Jdir[1].data_ptr(), stream=st, f32=f32)
    torch.cuda.synchronize()
    plan.check()
    return {"J": Jd.cpu().numpy(), "I": Id.cpu().numpy(), "J_up": Jdir[0].cpu().numpy(), "J_down": Jdir[1].cpu().numpy()}


def _plan(hs, angles, monkeypatch):
    idx = ANGLES[angles]
    monkeypatch.setenv("VRT_PATH", "patches")
    for k in ("VRT_STEP_STREAMS", "VRT_STEP_GROUP_DIR", "VRT_PATCH_SPLIT", "VRT_PATCH_CHAIN", "VRT_PAIR_BLOCK", "VRT_PATCH_QUAD",
              "VRT_PATCH_ORDER", "VRT_PATCH_TARGET"):
        monkeypatch.delenv(k, raising=False)
    plan = vrt.FormalPlan(hs, vrt.quadrature_directions(TH[idx], PH[idx]), 3, dirs=[1 if TH[i] > 90 else -1 for i in idx])
    plan.set_option("VRT_PATCH_CHAIN", 0)
    plan.set_option("VRT_PATCH_SPLIT", 3)
    return plan, W[idx]


def _both_orders(hs, so, monkeypatch, angles, nlam, f32):
    inputs, ref = _reference(so, angles, nlam, f32)
    plan, w = _plan(hs, angles, monkeypatch)
    got = {}
    for order in (0, 1):
        plan.set_option("VRT_PATCH_ORDER", order)
        got[order] = _run(plan, w, so.n, nlam, f32, inputs)
    layout = plan.patch_layout
    plan.close()
    # two patches in every (angle, layer), six angles per direction: >= 12 slots = two rows of eight in every launch
    assert layout["fewest_per_angle_layer"] >= 2, layout
    assert min(sum(TH[i] > 90 for i in ANGLES[angles]), sum(TH[i] < 90 for i in ANGLES[angles]) or 99) >= 6
    return got, ref


def _check_against_oracle(label, got, ref, f32, with_down):
    J, I, Ju, Jd = ref
    pairs = [("J", got["J"], J), ("J_up", got["J_up"], Ju)] + ([("J_down", got["J_down"], Jd)] if with_down else [])
    pairs += [(f"I[{a}]", got["I"][a], I[a]) for a in range(I.shape[0])]
    for name, g, r in pairs:
        if f32:
            ok, ndiff, size, ulps = within_conditions(g, r)
            print(f"{label} {name}: {ndiff} of {size} floats differ from the model, at most {ulps:g} ulp")
            assert ok, (label, name, ndiff, size, ulps)
        else:
            err = _rel(g, r)
            print(f"{label} {name}: element-wise relative error {float(err):.2e}")
            assert err < RTOL, (label, name, float(err))


CASES = [("f64", 7, "ul7n12"),          # 4 pair steps over 3 workgroups: shares 2, 1, 1
         ("f64", 6, "ul7n12"),          # 3 pair steps: an even split
         ("f32", 8, "ul7n12"),          # fp32 storage, an even pair count: k_patch_quad
         ("f32", 6, "ul7n12"),          # fp32 storage, an odd pair count: the pair kernel with sibling workgroups
         ("f64", 7, "up-only")]         # one direction: one stream's launches alone


@pytest.mark.parametrize("storage,nlam,angles", CASES)
def test_share_major_order_is_the_same_result(lattice, monkeypatch, storage, nlam, angles):
    hs, so = lattice
    f32 = storage == "f32"
    got, ref = _both_orders(hs, so, monkeypatch, angles, nlam, f32)
    for what in WHAT:
        assert np.array_equal(got[1][what], got[0][what]), what
    if angles == "up-only":
        assert not got[1]["J_down"].any()
    _check_against_oracle(f"{storage} nlam {nlam} {angles} order 1", got[1], ref, f32, with_down=angles != "up-only")


def test_the_launch_that_only_reduces(lattice, monkeypatch):
    """The launch behind the last solved layer has no patch rows, only reduction rows: it forms J_dir of the last layers
    (and of the never-visited last site, whose intensity is 0).  Their J_up and J_down under either order are the oracle's."""
    hs, so = lattice
    nlam = 7
    got, ref = _both_orders(hs, so, monkeypatch, "ul7n12", nlam, False)
    last_up = np.asarray(hs.perm_up[int(hs.layers_up[-2]) - 1:]) - 1        # sites of the last up layer
    last_down = np.asarray(hs.perm_down[int(hs.layers_down[-2]) - 1:]) - 1
    assert last_up.size and last_down.size
    for order in (0, 1):
        for name, sites, r in (("J_up", last_up, ref[2]), ("J_down", last_down, ref[3])):
            g = got[order][name][sites]
            assert np.isfinite(g).all()
            assert _rel(g, r[sites]) < RTOL, (order, name)
            assert np.array_equal(g, got[0][name][sites])
