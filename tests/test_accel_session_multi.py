"""Ng acceleration inside the multi-device Λ-iteration session (vrt_multi_lambda_set_acceleration / _last_acceleration) and
the `ng` keyword of MultiDevicePlan.lambda_iteration.

One device is listed W times (no RCCL): every member owns a block of the wavelengths, keeps the history of its own block,
forms its own five sums; the host adds them in member order, makes ONE (a, b), and the step is taken on every member or on
none.  The case is tests/test_accel.py's: the voro_small grid (1500 sites), ul7n12.dat, _lambda_case(pos, bounds, 11) -- 33
wavelengths, so W = 3 gives blocks of 11, 11, 11 (every block odd: a padding wavelength and a stride-2 tail in each member's
plane set), W = 4 gives 9, 8, 8, 8 (an odd block and even ones without a tail), W = 2 gives 17, 16 and W = 1 is the whole.

Bounds (tests/test_accel.py's derivation, none taken from the device): 2^-40 Σ|t| on each sum -- the kernel's longest chain of
additions is 122 links, the host's member sum adds at most 64, the bound admits 8192; δa, δb, the first-order image of
that bound through the 2 x 2 solve; 1e-9 against one oracle step.  Everything elementwise is compared bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import _lib, api
from test_accel import (QUAD, SUM_BOUND, _Session, _apply, _check_session_step, _coefficients, _lambda_case, _reference, _same,
                        _voronoi_oracle_step)

pytestmark = pytest.mark.gpu


class _World:
    """a vrt_multi of W handles on device 0 with the case, and a factory of sessions on it"""

    def __init__(self, voro_small, W, case=None):
        pos, nbr, bounds = voro_small
        self.pos, self.nbr, self.bounds = pos, nbr, bounds
        self.case = case if case is not None else _lambda_case(pos, bounds, 11)
        self.w, th, ph, _ = vrt.read_quadrature(QUAD)
        dirs = [1 if t > 90 else -1 for t in th]
        self.mp = vrt.MultiDevicePlan(pos, nbr, bounds, vrt.quadrature_directions(th, ph), dirs=dirs, devices=(0,) * W)
        self.lc, self.keep = self.case.c_struct()
        self.wd = np.ascontiguousarray(self.w, dtype=np.float64)
        self.n, self.nlam = pos.shape[0], int(self.keep["lam"].size)
        self.sessions = []

    def make(self):
        create = lambda out: _lib.load().vrt_multi_lambda_create(self.mp._h, ctypes.byref(self.lc),
                                                                 self.wd.ctypes.data_as(_lib.p_dbl), out)
        s = _Session("vrt_multi_lambda", create, self.n, self.nlam)
        self.sessions.append(s)
        return s

    def release(self):
        for s in self.sessions:
            s.close()
        self.sessions = []

    def close(self):
        self.release()
        self.mp.close()


@pytest.fixture(scope="module")
def worlds(voro_small):
    """the sweep-order worlds, one per W, shared by the tests of this module"""
    made = {}

    def world(W):
        if W not in made:
            assert os.environ.get("VRT_LAMBDA_NATIVE", "1") == "1"
            made[W] = _World(voro_small, W)
        return made[W]
    yield world
    for w in made.values():
        w.close()


@pytest.fixture(scope="module")
def oracle_sites(voro_small):
    return orc.make_sites(*voro_small)


def _set_state(s, S, pops):
    S, pops = np.ascontiguousarray(S, dtype=np.float64), np.ascontiguousarray(pops, dtype=np.float64)
    return s.fn("set_state")(s.h, S.ctypes.data_as(_lib.p_dbl), pops.ctypes.data_as(_lib.p_dbl))


def _run_to_step(plain, acc):
    """four iterates of both, acceleration (2, 4, 4) on `acc`: (S1..S4 of the plain session, the report, S of acc after the step)"""
    acc.accelerate(2, 4, 4)
    S_hist = []
    for _ in range(4):
        dp, da = plain.iterate(), acc.iterate()
        assert dp == da
        S_hist.append(plain.get()[1])
    return S_hist, acc.last(), acc.get()[1]


# ---- 1: the step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [3, 1, 4])
def test_gpu_multi_session_takes_an_ng_step(W, worlds, oracle_sites):
    """tests/test_accel.py's checks of a session step, on W members: bit for bit through iterate 3, the plain scalar at
    iterate 4, the reported sums within 2^-40 Σ|t| of the exact sums of the session's own iterates, a and b within δa and
    δb and exactly the host formulas of the reported sums, S exactly x_acc of the reported (a, b) with everything else the
    plain iterate's, and iterate 5 within 1e-9 of one oracle step from the extrapolated state"""
    world, so = worlds(W), oracle_sites
    plain, acc = world.make(), world.make()
    try:
        _check_session_step(plain, acc, lambda S, pops: _voronoi_oracle_step(world.case, so, S, pops), f"multi W={W}")
    finally:
        world.release()


def test_gpu_multi_session_takes_an_ng_step_with_one_wavelength_per_member(voro_small, oracle_sites):
    """the same checks on seven wavelengths (tests/test_resume_host.py's small_lambda_case with nbb = 3, nbf = 2) over
    W = 8: seven members hold one wavelength -- a single pair plane with its padding, all of it the stride-2 tail of the
    member's range -- and one holds none, keeps no history and adds no sums"""
    from test_resume_host import small_lambda_case
    assert os.environ.get("VRT_LAMBDA_NATIVE", "1") == "1"
    pos, nbr, bounds = voro_small
    world = _World(voro_small, 8, case=small_lambda_case(pos, bounds, 11, 3, 2))
    assert world.nlam == 7
    try:
        _check_session_step(world.make(), world.make(), lambda S, pops: _voronoi_oracle_step(world.case, oracle_sites, S, pops),
                            "multi W=8, 7 wavelengths")
    finally:
        world.close()


# ---- 2: both layouts ----------------------------------------------------------------------------------------------------------
def test_gpu_multi_session_layouts_agree(voro_small, monkeypatch):
    """VRT_LAMBDA_NATIVE = 1 (every member's block in two sweep-order plane sets) and = 0 (its d_S_new columns in the
    caller's layout), W = 3: each run's a, b within its own δa, δb, the two within the sum of those, and S after the step
    within the first-order image of that through x_acc = x0 + a (x1 - x0) + b (x2 - x0): (δa1 + δa0) |x1 - x0| +
    (δb1 + δb0) |x2 - x0|, plus the image |c| |Δx0| + |a| |Δx1| + |b| |Δx2| of what the two layouts' plain iterates
    differ by (measured, printed; zero when the plain iterates agree bit for bit) and 8 roundings of the largest term"""
    results = {}
    for native in ("1", "0"):
        monkeypatch.setenv("VRT_LAMBDA_NATIVE", native)              # read when the plans are made
        world = _World(voro_small, 3)
        try:
            S_hist, (applied, sums, coeffs), S_acc = _run_to_step(world.make(), world.make())
            ref = _reference(*S_hist[::-1], result=False)
            assert applied == 1
            assert np.array_equal(S_acc, _apply(coeffs[0], coeffs[1], S_hist[3], S_hist[2], S_hist[1]))
            results[native] = (coeffs, S_acc, ref, S_hist)
        finally:
            world.close()
    (c1, S1, ref1, H1), (c0, S0, ref0, H0) = results["1"], results["0"]
    for c, ref in ((c1, ref1), (c0, ref0)):
        assert abs(c[0] - ref["a"]) <= ref["da"] and abs(c[1] - ref["b"]) <= ref["db"]
    da, db = ref1["da"] + ref0["da"], ref1["db"] + ref0["db"]
    assert abs(c1[0] - c0[0]) <= da and abs(c1[1] - c0[1]) <= db
    a, b = max(abs(c1[0]), abs(c0[0])), max(abs(c1[1]), abs(c0[1]))
    c = 1 + a + b
    x0, x1, x2 = H0[3], H0[2], H0[1]
    moved = [np.abs(H1[k] - H0[k]) for k in (3, 2, 1)]
    bound = (da * np.abs(x1 - x0) + db * np.abs(x2 - x0) + c * moved[0] + a * moved[1] + b * moved[2] +
             8 * np.finfo(float).eps * (c * x0 + a * x1 + b * x2))
    print(f"sweep-order a, b = {c1}, caller layout {c0}; plain iterates differ by {[float(m.max()) for m in moved]}; "
          f"S after the step differs by {np.abs(S1 - S0).max():.3g}, bound up to {bound.max():.3g}")
    assert (np.abs(S1 - S0) <= bound).all()


# ---- 3: determinism -----------------------------------------------------------------------------------------------------------
def test_gpu_multi_session_is_deterministic(worlds):
    """two accelerated W = 3 sessions built alike: the same sums, coefficients and S, byte for byte, after iterates 4 and 8
    (the members' sums are added in member order, never in the order their host threads finished)"""
    world = worlds(3)
    s1, s2 = world.make(), world.make()
    try:
        s1.accelerate(2, 4, 4), s2.accelerate(2, 4, 4)
        for it in range(1, 9):
            assert s1.iterate() == s2.iterate()
            if it % 4:
                assert s1.last()[0] == 0 and s2.last()[0] == 0
                continue
            (ap1, sums1, co1), (ap2, sums2, co2) = s1.last(), s2.last()
            assert ap1 == ap2 == 1, it
            assert sums1.tobytes() == sums2.tobytes() and co1.tobytes() == co2.tobytes(), it
            g1, g2 = s1.get(), s2.get()
            assert all(p.tobytes() == q.tobytes() for p, q in zip(g1, g2)), it
    finally:
        world.release()


# ---- 4: off again is plain ------------------------------------------------------------------------------------------------------
def test_gpu_multi_session_with_acceleration_switched_off_again_is_the_plain_session(worlds):
    world = worlds(3)
    plain, acc = world.make(), world.make()
    try:
        acc.accelerate(2, 4, 4)
        acc.accelerate(0, 0, 0)
        for it in range(1, 6):
            dp, da = plain.iterate(), acc.iterate()
            assert dp == da and _same(plain.get(), acc.get()), it
            assert acc.last()[0] == 0 and plain.last()[0] == 0
    finally:
        world.release()


# ---- 5: state -------------------------------------------------------------------------------------------------------------------
def test_gpu_multi_session_set_state_drops_the_history_and_resumes_after_a_step(worlds):
    world = worlds(3)
    plain, acc, fresh = world.make(), world.make(), world.make()
    try:
        acc.accelerate(2, 4, 4)
        for it in (1, 2):
            assert plain.iterate() == acc.iterate()
        _, S2, pops2, _, _ = acc.get()
        assert _set_state(acc, S2, pops2) == 0            # its own state: the iterates go on as they would have ...
        assert acc.last()[0] == 0
        for it in (3, 4):
            assert plain.iterate() == acc.iterate()
            assert acc.last()[0] == 0, it                # ... but iterates 1 and 2 are no history any more: no step at 4
        assert _same(plain.get(), acc.get())             # S is the plain update's
        # the step is due again, and complete, at iterate 8
        S_hist = []
        for it in (5, 6, 7, 8):
            assert plain.iterate() == acc.iterate()
            S_hist.append(plain.get()[1])
            assert (acc.last()[0] != 0) == (it == 8), it
        applied, sums, coeffs = acc.last()
        assert applied == 1
        assert np.array([*_coefficients(sums)[:2]]).tobytes() == coeffs.tobytes()
        J8, S8x, pops8, R8, g8 = acc.get()
        assert np.array_equal(S8x, _apply(coeffs[0], coeffs[1], S_hist[3], S_hist[2], S_hist[1]))
        assert not np.array_equal(S8x, S_hist[3]) and np.array_equal(pops8, plain.get()[2])
        # the state right after an accepted step resumes in a fresh session: one iterate, acceleration off on both
        acc.accelerate(0, 0, 0)
        assert _set_state(fresh, S8x, pops8) == 0
        dw, dg = acc.iterate(), fresh.iterate()
        assert dw == dg and _same(acc.get(), fresh.get())
        assert acc.last()[0] == 0 and fresh.last()[0] == 0
    finally:
        world.release()


# ---- 6: other block sizes -------------------------------------------------------------------------------------------------------
def test_gpu_multi_session_four_members(worlds):
    """W = 4: blocks of 9, 8, 8, 8 -- an odd block with its tail beside even ones without.  The step is accepted, the
    coefficients are the host formulas of the reported sums, the sums are within the bound and S is exactly x_acc."""
    world = worlds(4)
    plain, acc = world.make(), world.make()
    try:
        S_hist, (applied, sums, coeffs), S_acc = _run_to_step(plain, acc)
        assert applied == 1
        assert np.array([*_coefficients(sums)[:2]]).tobytes() == coeffs.tobytes()
        ref = _reference(*S_hist[::-1], result=False)
        print(f"W = 4: sums off by {np.abs(sums - ref['sums']) / ref['mags']} Σ|t|; a, b = {coeffs}")
        assert (np.abs(sums - ref["sums"]) <= SUM_BOUND * ref["mags"]).all()
        assert abs(coeffs[0] - ref["a"]) <= ref["da"] and abs(coeffs[1] - ref["b"]) <= ref["db"]
        assert np.array_equal(S_acc, _apply(coeffs[0], coeffs[1], S_hist[3], S_hist[2], S_hist[1]))
    finally:
        world.release()


# ---- 7: Python ------------------------------------------------------------------------------------------------------------------
def test_gpu_multi_device_lambda_iteration_ng_keyword(worlds, tmp_path):
    world = worlds(2)
    run = lambda maxiter, **kw: world.mp.lambda_iteration(1e-4, maxiter, world.case, world.w, **kw)
    plain = run(60)
    assert len(plain) == 4
    fast = run(60, ng=(4, 4))
    assert len(fast) == 5
    J0, S0, p0, h0 = plain
    J1, S1, p1, h1, steps = fast
    print(f"plain {len(h0)} iterates, accelerated {len(h1)}; steps {steps}")
    assert h0[-1] <= 1e-4 and h1[-1] <= 1e-4
    assert steps and all(it % 4 == 0 for it, *_ in steps)
    assert len(h1) < len(h0)
    assert np.abs(S1 / S0 - 1).max() <= 10 * 1e-4
    with pytest.raises(_lib.VrtError):
        run(2, ng=(3, 4))
    # checkpoint and resume with ng, as for Lambda_voronoi_host: two iterates (no step yet: the plain ones), then the rest
    # from the file -- the history is the file's followed by the new scalars, the schedule counts the new session's iterates
    path = str(tmp_path / "run.npz")
    first = run(2, ng=(4, 4), checkpoint=path)
    assert len(first) == 5 and first[4] == []
    ck = api.read_checkpoint(path)
    assert ck["iterate"] == 2 and ck["history"] == first[3] == h1[:2] == h0[:2]
    assert np.array_equal(ck["S"], first[1]) and np.array_equal(ck["populations"], first[2])
    second = run(60, ng=(4, 4), resume=path, checkpoint=path)
    assert second[3][:2] == first[3] and second[3][-1] <= 1e-4
    assert second[4] and all(it % 4 == 0 for it, *_ in second[4])
    assert len(second[3]) < len(h0)
    ck = api.read_checkpoint(path)
    assert ck["iterate"] == len(second[3]) and ck["history"] == second[3] and np.array_equal(ck["S"], second[1])
    assert np.abs(second[1] / S0 - 1).max() <= 10 * 1e-4
