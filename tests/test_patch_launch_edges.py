"""GPU tests (-m gpu) of the edges of the patch launches (voronoirt_amd/csrc/vrt_patch.hip): how a workgroup finds its
item (the two-dimensional grid: XCD lane + 8 x (split, sibling) across, rows of the work list down, reduction rows behind
them; the item's record in one scalar load; the entry table's nine loads in flight together).  None of it changes an
operation or a value, so J_up, J_down, J and every user angle's I must be BIT FOR BIT the same under the default grouping
of the angles (one direction per stream), with the angles dealt to three streams and with two streams that mix the
directions (VRT_STEP_GROUP_DIR=0: no stream holds a direction, J is reduced behind the sweep) -- other work lists, other
grids, other reduction rows -- and all of them are the oracle's.  (Write-through stores in the per-layer launches, an
option VRT_PATCH_WT of the same change, lost its A/B and was taken out again: profiles/edges/INDEX.md.)

The oracle: fp64 storage against oracle.J_voronoi_model (no storage rounding: the plain fp64 oracle, which also returns
I, J_up and J_down) element-wise to 1e-10 by oracle/parity.py.  fp32 storage cannot meet 1e-10 against fp64 numbers
(floats are 6e-8 apart); it is held to the project's storage-model oracle instead (oracle/f32_model.py, as
tests/test_f32_storage.py does): the model's floats bit for bit in at least 99.9 % of the elements, within 2 float ulps
in the rest.

The grid is a body-centred lattice whose layers (1 152 sites) need at least three 512-entry patches per angle, and whose
work lists have padding slots (patches of a layer x angles of a launch is no multiple of 8): both are asserted from the
plan's own account (FormalPlan.patch_layout)."""
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


@pytest.fixture(scope="module")
def lattice():
    pos, nbr, bounds = synth.bcc_grid(24, 6, seed=7)
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    yield hs, orc.make_sites(pos, nbr, bounds)
    hs.close()


_refs = {}


def _reference(so, angles, nlam, f32):
    """(J, I, J_up, J_down) of the oracle for the case's inputs, once per (angles, nlam, storage) and read-only"""
    key = (angles, nlam, f32)
    if key not in _refs:
        idx = ANGLES[angles]
        S, al, I0u, I0d = draw_case(so, nlam, seed=100 + nlam)
        f = lambda a: np.asarray(a, dtype=np.float64)
        model = PATH_MODEL["patches"] if f32 else {}
        out = orc.J_voronoi_model(W[idx], TH[idx], PH[idx], f(S), f(al), so, I0_up=f(I0u), I0_down=f(I0d), nthreads=8, **model)
        for a in out:
            a.setflags(write=False)
        _refs[key] = ((S, al, I0u, I0d), out)
    return _refs[key]


def _run(plan, w, n, nlam, f32, inputs):
    """J, I (caller layout: execute_dev) and J_up, J_down (sweep order in and out: execute_native_dev, brought back to
    (n, nlam)) of the plan as its options stand; w: the quadrature weights of the plan's angles"""
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
    launches = plan.last_launches
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
    Jdir = [torch.full((n, nlam), float("nan"), dtype=dt, device=dev) for _ in range(2)]
    plan.from_native_dev(1, nlam, nlam, J_nat[0].data_ptr(), Jdir[0].data_ptr(), stream=st, f32=f32)
    plan.from_native_dev(-1, nlam, nlam, J_nat[1].data_ptr(), Jdir[1].data_ptr(), stream=st, f32=f32)
    torch.cuda.synchronize()
    plan.check()
    return {"J": Jd.cpu().numpy(), "I": Id.cpu().numpy(), "J_up": Jdir[0].cpu().numpy(), "J_down": Jdir[1].cpu().numpy()}, launches


def _plan(hs, angles, monkeypatch, quad):
    idx = ANGLES[angles]
    monkeypatch.setenv("VRT_PATH", "patches")
    monkeypatch.setenv("VRT_PATCH_QUAD", "1" if quad else "0")          # read when the plan is created
    for k in ("VRT_STEP_STREAMS", "VRT_STEP_GROUP_DIR", "VRT_PATCH_SPLIT", "VRT_PATCH_CHAIN", "VRT_PAIR_BLOCK"):
        monkeypatch.delenv(k, raising=False)
    plan = vrt.FormalPlan(hs, vrt.quadrature_directions(TH[idx], PH[idx]), 3, dirs=[1 if TH[i] > 90 else -1 for i in idx])
    return plan, W[idx]


# the option combinations, in an order a live plan can follow (the angle groups are rebuilt when the stream count changes)
COMBOS = (("default", {}),
          ("three streams", {"VRT_STEP_STREAMS": 3}),
          ("directions mixed", {"VRT_STEP_STREAMS": 2, "VRT_STEP_GROUP_DIR": 0}))


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


@pytest.mark.parametrize("form", ["per-layer", "chain"])
@pytest.mark.parametrize("storage", ["f64", "f32-quad", "f32-pair"])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("nlam", [3, 4, 5])
@pytest.mark.parametrize("angles", ["ul7n12", "up-only"])
def test_every_option_combination_is_the_same_result(lattice, monkeypatch, angles, nlam, split, storage, form):
    """nlam 3 / 4 / 5: two pairs with a padded wavelength, two full pairs, three pairs (a lone last pair: fp32 storage in
    blocks of two pairs then runs the pair kernel with sibling workgroups); VRT_PATCH_SPLIT 1 / 3: one workgroup per item,
    or more splits than some items have pair steps (workgroups without work)."""
    hs, so = lattice
    f32 = storage != "f64"
    inputs, ref = _reference(so, angles, nlam, f32)
    plan, w = _plan(hs, angles, monkeypatch, quad=storage == "f32-quad")
    plan.set_option("VRT_PATCH_SPLIT", split)
    plan.set_option("VRT_PATCH_CHAIN", 1 if form == "chain" else 0)
    # (the chained launch has no sibling workgroups: floats in blocks of two pairs with an odd pair count keep the launches)
    chained = form == "chain" and not (storage == "f32-quad" and ((nlam + 1) // 2) % 2 == 1)
    got = {}
    for name, opts in COMBOS:
        for k, v in opts.items():
            plan.set_option(k, v)
        got[name], launches = _run(plan, w, so.n, nlam, f32, inputs)
        assert (launches == 1) == chained, (name, launches)
    layout = plan.patch_layout
    assert layout["fewest_per_angle_layer"] >= 3, layout
    assert layout["padding_slots"] >= 1, layout
    plan.close()
    for name in got:
        for what in ("J", "I", "J_up", "J_down"):
            assert np.array_equal(got[name][what], got["default"][what]), (name, what)
    if angles == "up-only":
        assert not got["default"]["J_down"].any()
    _check_against_oracle(f"{angles} nlam {nlam} split {split} {storage} {form}", got["default"], ref, f32, with_down=angles != "up-only")


def test_a_second_call_finds_nothing_left_behind(lattice, monkeypatch):
    """The same plan called twice in a row with DIFFERENT inputs, then again with the first ones: a store of the first
    call that had not reached memory (or a stale line another launch kept) would show in the calls behind it."""
    hs, so = lattice
    nlam = 5
    inputs, ref = _reference(so, "ul7n12", nlam, False)
    other = tuple(np.asarray(x, dtype=np.float64) * s for x, s in zip(inputs, (3.0, 0.5, 2.0, 0.25)))
    plan, w = _plan(hs, "ul7n12", monkeypatch, quad=True)
    plan.set_option("VRT_PATCH_CHAIN", 0)
    first, _ = _run(plan, w, so.n, nlam, False, inputs)
    second, _ = _run(plan, w, so.n, nlam, False, other)
    third, _ = _run(plan, w, so.n, nlam, False, inputs)
    plan.close()
    for what in ("J", "I", "J_up", "J_down"):
        assert np.array_equal(first[what], third[what]), what
        assert not np.array_equal(first[what], second[what]), what
    _check_against_oracle("repeat", third, ref, False, with_down=True)
    f = lambda a: np.asarray(a, dtype=np.float64)
    J2 = orc.J_voronoi(W, TH, PH, f(other[0]), f(other[1]), so, I0_up=f(other[2]), I0_down=f(other[3]), nthreads=8)
    assert _rel(second["J"], J2) < RTOL
