"""GPU tests (-m gpu) of the J reduction that rides in the patch blocks of the per-layer launches (option
VRT_PATCH_REDUCE_RIDE, voronoirt_amd/csrc/vrt_patch.hip: ride_issue / ride_finish).  With the option on, the patch blocks
of launch L form J_dir of layer L - 1 in their own start-up; with it off, reduction blocks behind the patch rows do, as
before.  Both read the same final intensities and add them per element in the same order, so J, J_up, J_down and every
angle's I with the option on must be BIT FOR BIT those with it off, and both are the oracle's: fp64 storage element-wise
to 1e-10 (oracle/parity.py), fp32 storage held to the storage-model oracle as tests/test_patch_dispatch_order.py holds it.

Grids: the body-centred lattice of tests/test_patch_dispatch_order.py (2 x 18 x 18 x 6 = 3 888 sites, layers of 648
sites, two work-list rows per launch) and the suite's 1 500-site Voronoi grid, whose layers are ragged and small (most
blocks of a launch get no slice).  Per-layer launches are forced (VRT_PATCH_CHAIN=0)."""
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
DIRS = [1 if TH[i] > 90 else -1 for i in range(NQ)]
WHAT = ("J", "I", "J_up", "J_down")
ENV = ("VRT_STEP_STREAMS", "VRT_STEP_GROUP_DIR", "VRT_PATCH_SPLIT", "VRT_PATCH_CHAIN", "VRT_PAIR_BLOCK", "VRT_PATCH_QUAD",
       "VRT_PATCH_ORDER", "VRT_PATCH_TARGET", "VRT_PATCH_LEAN", "VRT_PATCH_REDUCE_RIDE")


@pytest.fixture(scope="module")
def grids():
    out = {}
    for name, (pos, nbr, bounds) in (("lattice", synth.bcc_grid(18, 6, seed=7)),
                                     ("voronoi", synth.voronoi_grid(1500, seed=5, bounds=(0.0, 2.0, 0.0, 1.0, 0.0, 1.0), scale_height=0.7))):
        out[name] = (vrt.VoronoiSites(pos, nbr, bounds, device=0), orc.make_sites(pos, nbr, bounds))
    yield out
    for hs, _ in out.values():
        hs.close()


_refs = {}


def _reference(grid, so, nlam, f32):
    """inputs and (J, I, J_up, J_down) of the oracle, once per (grid, nlam, storage) and read-only"""
    key = (grid, nlam, f32)
    if key not in _refs:
        S, al, I0u, I0d = draw_case(so, nlam, seed=500 + nlam)
        f = lambda a: np.asarray(a, dtype=np.float64)
        model = PATH_MODEL["patches"] if f32 else {}
        out = orc.J_voronoi_model(W, TH, PH, f(S), f(al), so, I0_up=f(I0u), I0_down=f(I0d), nthreads=8, **model)
        for a in out:
            a.setflags(write=False)
        _refs[key] = ((S, al, I0u, I0d), out)
    return _refs[key]


class _Case:
    """device copies of one case's inputs and the two entries of a plan"""

    def __init__(self, n, nlam, f32, inputs):
        import torch
        self.torch, self.n, self.nlam, self.f32 = torch, n, nlam, f32
        self.dev = torch.device("cuda", 0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.dt = torch.float32 if f32 else torch.float64
        self.rode = []                                       # the plan's account of the riding form, per sweep
        self.S, self.A, self.U, self.D = (torch.from_numpy(np.ascontiguousarray(x)).to(self.dev).to(self.dt).contiguous() for x in inputs)

    def caller(self, plan, want_J=True, want_I=True):
        """J and I through the caller-layout entry; (J, I, launches)"""
        t = self.torch
        J = t.full((self.n, self.nlam), float("nan"), dtype=self.dt, device=self.dev)
        I = t.full((NQ, self.n, self.nlam), float("nan"), dtype=self.dt, device=self.dev)
        plan.execute_dev(self.nlam, self.nlam, self.S.data_ptr(), self.A.data_ptr(), _lib.ALPHA_SITE_LAM, W, dJ=J.data_ptr() if want_J else 0,
                         dI0_up=self.U.data_ptr(), dI0_down=self.D.data_ptr(), dI_out=I.data_ptr() if want_I else 0, stream=self.st, f32=self.f32)
        t.cuda.synchronize()
        plan.check()
        assert plan.last_path == "patches"
        self.rode.append(plan.patch_ride_stats)
        return J.cpu().numpy(), I.cpu().numpy(), plan.last_launches

    def native(self, plan):
        """J_up and J_down through the sweep-order entry, brought back to (n, nlam); (J_up, J_down, launches)"""
        t, nlam = self.torch, self.nlam
        cnt = plan.native_plane_count(nlam)
        size = 4 if self.f32 else 8
        S_nat = [t.empty(cnt, dtype=self.dt, device=self.dev) for _ in range(2)]
        A_nat = t.empty(2 * cnt, dtype=self.dt, device=self.dev)
        J_nat = [t.full((cnt,), float("nan"), dtype=self.dt, device=self.dev) for _ in range(2)]
        plan.to_native_dev(nlam, nlam, self.S.data_ptr(), S_nat[0].data_ptr(), S_nat[1].data_ptr(), stream=self.st, f32=self.f32)
        plan.to_native_dev(nlam, nlam, self.A.data_ptr(), A_nat.data_ptr(), A_nat.data_ptr() + size * cnt, stream=self.st, f32=self.f32)
        plan.execute_native_dev(nlam, S_nat[0].data_ptr(), S_nat[1].data_ptr(), A_nat.data_ptr(), _lib.ALPHA_SITE_LAM_NATIVE, W,
                                dJ_up=J_nat[0].data_ptr(), dJ_down=J_nat[1].data_ptr(), dI0_up=self.U.data_ptr(),
                                dI0_down=self.D.data_ptr(), stream=self.st, f32=self.f32)
        launches = plan.last_launches
        self.rode.append(plan.patch_ride_stats)
        Jdir = [t.full((self.n, nlam), float("nan"), dtype=self.dt, device=self.dev) for _ in range(2)]
        plan.from_native_dev(1, nlam, nlam, J_nat[0].data_ptr(), Jdir[0].data_ptr(), stream=self.st, f32=self.f32)
        plan.from_native_dev(-1, nlam, nlam, J_nat[1].data_ptr(), Jdir[1].data_ptr(), stream=self.st, f32=self.f32)
        t.cuda.synchronize()
        plan.check()
        return Jdir[0].cpu().numpy(), Jdir[1].cpu().numpy(), launches

    def run(self, plan, native=True):
        J, I, l1 = self.caller(plan)
        if not native:                                       # (the sweep-order entry exists for one pair per block only)
            return {"J": J, "I": I, "launches": (l1,)}
        Ju, Jd, l2 = self.native(plan)
        return {"J": J, "I": I, "J_up": Ju, "J_down": Jd, "launches": (l1, l2)}


def _plan(hs, monkeypatch, env, options):
    monkeypatch.setenv("VRT_PATH", "patches")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():                                # creation-only options
        monkeypatch.setenv(k, str(v))
    plan = vrt.FormalPlan(hs, vrt.quadrature_directions(TH, PH), 3, dirs=DIRS)
    plan.set_option("VRT_PATCH_CHAIN", 0)
    for k, v in options.items():
        plan.set_option(k, v)
    return plan


def _per_layer_count(hs, streams, group_dir):
    """launches of a per-layer sweep: one per layer (from the second to the deeper direction's last) and stream group, and
    one more per group behind the last layer where the groups hold a direction each and reduce it there (with one stream:
    the one group holds both) -- not the single chained launch"""
    layers = max(len(hs.layers_up), len(hs.layers_down)) - 1
    groups = max(1, streams)
    return (layers - 1) * groups + (groups if group_dir else 0)


def _check_against_oracle(label, got, ref, f32):
    J, I, Ju, Jd = ref
    pairs = [("J", got["J"], J)] + ([("J_up", got["J_up"], Ju), ("J_down", got["J_down"], Jd)] if "J_up" in got else [])
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


# (grid, storage, nlam, environment at plan creation, options of the plan)
CASES = {
    "nlam1": ("lattice", "f64", 1, {}, {}),
    "nlam2": ("lattice", "f64", 2, {}, {}),
    "nlam7": ("lattice", "f64", 7, {}, {}),                                      # odd: a ragged last pair
    "nlam13": ("lattice", "f64", 13, {}, {}),
    "nlam64-split1": ("lattice", "f64", 64, {}, {"VRT_PATCH_SPLIT": 1}),         # 648 x 32 pair elements = 41 chunks over the 16 blocks of
                                                                                 #   one split (the limit is 64 chunks): 2-3 per thread
    "voronoi-nlam7": ("voronoi", "f64", 7, {}, {}),
    "voronoi-nlam13-f32": ("voronoi", "f32", 13, {}, {}),
    "pair-block1": ("lattice", "f64", 7, {"VRT_PAIR_BLOCK": 1}, {}),
    "pair-block2": ("lattice", "f64", 7, {"VRT_PAIR_BLOCK": 2}, {}),
    "f32-quad": ("lattice", "f32", 8, {}, {}),                                   # even pair count: k_patch_quad
    "f32-pairs": ("lattice", "f32", 6, {}, {}),                                  # odd pair count: the float pair kernel
    "solve": ("lattice", "f64", 7, {}, {"VRT_PATCH_LEAN": 0}),                   # k_patch_solve
    "order0": ("lattice", "f64", 7, {}, {"VRT_PATCH_ORDER": 0, "VRT_PATCH_SPLIT": 3}),
    "order1": ("lattice", "f64", 7, {}, {"VRT_PATCH_ORDER": 1, "VRT_PATCH_SPLIT": 3}),
    "split1": ("lattice", "f64", 7, {}, {"VRT_PATCH_SPLIT": 1}),
    "split3": ("lattice", "f64", 7, {}, {"VRT_PATCH_SPLIT": 3}),
    "split99": ("lattice", "f64", 7, {}, {"VRT_PATCH_SPLIT": 99}),               # more than the four pair steps: capped
    "one-stream": ("lattice", "f64", 7, {}, {"VRT_STEP_STREAMS": 1}),            # both directions' ranges ride in one launch
    "no-group-dir": ("lattice", "f64", 7, {}, {"VRT_STEP_GROUP_DIR": 0}),        # no stream holds a direction: nothing rides
}


@pytest.mark.parametrize("case", list(CASES))
def test_riding_reduction_is_the_same_result(grids, monkeypatch, case):
    grid, storage, nlam, env, options = CASES[case]
    hs, so = grids[grid]
    f32 = storage == "f32"
    inputs, ref = _reference(grid, so, nlam, f32)
    plan = _plan(hs, monkeypatch, env, options)
    c = _Case(so.n, nlam, f32, inputs)
    got, rode = {}, {}
    for ride in (0, 1):
        plan.set_option("VRT_PATCH_REDUCE_RIDE", ride)
        c.rode = []
        got[ride] = c.run(plan, native=env.get("VRT_PAIR_BLOCK", 1) == 1)
        rode[ride] = c.rode
    plan.close()
    # the plan's own account: with the option off nothing rides; with it on every sweep has launches that reduce in their
    # patch blocks -- unless no stream holds a direction, where no launch reduces at all
    print(f"{case}: riding launches and most chunks per block, per sweep: {rode[1]}")
    assert all(r == {"launches": 0, "max_chunks": 0} for r in rode[0]), rode[0]
    for r in rode[1]:
        if options.get("VRT_STEP_GROUP_DIR", 1) == 0:
            assert r == {"launches": 0, "max_chunks": 0}, r
        else:
            assert r["launches"] > 0 and 1 <= r["max_chunks"] <= 4, r
            if case == "nlam64-split1":
                assert r["max_chunks"] >= 2, r                  # the blocks' second and later chunks, read behind the table
    for what in WHAT:
        assert (what in got[1]) == (what in got[0])
        if what in got[1]:
            assert got[1][what].tobytes() == got[0][what].tobytes(), what
    print(f"{case}: launches {got[1]['launches']} (ride) {got[0]['launches']} (rows)")
    assert got[1]["launches"] == got[0]["launches"]
    count = _per_layer_count(hs, options.get("VRT_STEP_STREAMS", 2), options.get("VRT_STEP_GROUP_DIR", 1))
    assert all(launches == count for launches in got[1]["launches"]), (got[1]["launches"], count)
    _check_against_oracle(f"{case} ride", got[1], ref, f32)


def test_intensities_only_and_J_after_it(grids, monkeypatch):
    """a call that asks for intensities only reduces nothing (riding or not); a J call on the same plan afterwards rides
    again and gives the J of a fresh plan's"""
    hs, so = grids["lattice"]
    nlam = 7
    inputs, ref = _reference("lattice", so, nlam, False)
    c = _Case(so.n, nlam, False, inputs)
    got = {}
    for ride in (0, 1):
        plan = _plan(hs, monkeypatch, {}, {"VRT_PATCH_REDUCE_RIDE": ride})
        J0, I_only, _ = c.caller(plan, want_J=False)
        assert np.isnan(J0).all()                            # J was not asked for: untouched
        assert c.rode[-1] == {"launches": 0, "max_chunks": 0}    # ... and nothing was reduced, riding or not
        J, I, launches = c.caller(plan)
        assert (c.rode[-1]["launches"] > 0) == (ride == 1)
        got[ride] = (I_only, J, I, launches)
        plan.close()
    for a, b in zip(got[0][:3], got[1][:3]):
        assert a.tobytes() == b.tobytes()
    assert got[1][0].tobytes() == got[1][2].tobytes()        # the intensities do not depend on whether J is formed
    assert got[0][3] == got[1][3] == _per_layer_count(hs, 2, 1)
    assert _rel(got[1][1], ref[0]) < RTOL
    for a in range(NQ):
        assert _rel(got[1][0][a], ref[1][a]) < RTOL
