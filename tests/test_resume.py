"""Resuming the line Λ-iteration sessions from saved S and populations on the device: vrt_lambda_set_state (sweep-order
and caller-layout form), vrt_regular_lambda_set_state, vrt_multi_lambda_set_state (one handle; two handles on one device,
whose wavelength blocks of 9 are 5 and 4), and the S0 / populations0 / checkpoint / resume keywords of the Python drivers.

Every comparison is bit for bit: *_get and the layout kernels copy values, and an iterate reads nothing but (S,
populations) and the constants of the case.  The Voronoi forms run at an odd (9) and an even (10) number of wavelengths:
the odd count has a padding wavelength in the sweep-order plane sets.  The reference of a form -- six iterates of one
session, with what *_get returns after each -- is computed once and shared by the tests of that form."""
import ctypes
import os

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib, api, synth
from test_resume_host import small_lambda_case

pytestmark = pytest.mark.gpu

QUAD = "ul7n12.dat"
BLOCKS = {9: (5, 2), 10: (6, 2), 6: (2, 2)}           # nλ -> (line wavelengths, wavelengths per continuum block)
FORMS = [("native", 9), ("native", 10), ("caller", 9), ("caller", 10), ("regular", 0), ("multi1", 9), ("multi1", 10),
         ("multi2", 9), ("multi2caller", 9), ("multi7", 6)]
NG_FORMS = [("native", 9), ("native", 10), ("caller", 9), ("regular", 0)]       # the multi-device session has no acceleration


class _Session:
    """vrt_lambda_*, vrt_regular_lambda_* or vrt_multi_lambda_* through ctypes"""

    def __init__(self, prefix, create, n, nlam):
        self.L = _lib.load()
        self.prefix, self.n, self.nlam = prefix, n, nlam
        self.h = ctypes.c_void_p()
        _lib.check(create(ctypes.byref(self.h)))

    def fn(self, name):
        return getattr(self.L, f"{self.prefix}_{name}")

    def iterate(self):
        d = ctypes.c_double()
        _lib.check(self.fn("iterate")(self.h, ctypes.byref(d)))
        return d.value

    def get(self):
        n, nlam = self.n, self.nlam
        out = [np.zeros((n, nlam)), np.zeros((n, nlam)), np.zeros((3, n)), np.zeros((n, 3, 3)), np.zeros(n)]
        _lib.check(self.fn("get")(self.h, *(a.ctypes.data_as(_lib.p_dbl) for a in out)))
        return out                                  # J, S, populations, R, gamma

    def step(self):
        """one iterate: (scalar, J, S, populations, R, gamma)"""
        return (self.iterate(), *self.get())

    def set_state(self, S, pops):
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (S, pops)]
        return self.fn("set_state")(self.h, *(None if a is None else a.ctypes.data_as(_lib.p_dbl) for a in keep))

    def accelerate(self, order, start, period):
        _lib.check(self.fn("set_acceleration")(self.h, order, start, period))

    def applied(self):
        applied = ctypes.c_int(9)
        _lib.check(self.fn("last_acceleration")(self.h, ctypes.byref(applied), None, None))
        return applied.value

    def close(self):
        if self.h:
            self.fn("destroy")(self.h)
            self.h = ctypes.c_void_p()


class _World:
    """The grid, plan and case of one form, a factory of fresh sessions on them, and the reference: `rec[k]` is what
    iterate k of a session started by create returned, k = 1 .. 6 (rec[0] is None)."""

    def __init__(self, form, nlam, voro_small):
        self.form, self.sessions, self.closers = form, [], []
        # the form of S is chosen when a plan is made
        old = os.environ.get("VRT_LAMBDA_NATIVE")
        os.environ["VRT_LAMBDA_NATIVE"] = "0" if form in ("caller", "multi2caller") else "1"
        try:
            self._build(form, nlam, voro_small)
        finally:
            if old is None:
                del os.environ["VRT_LAMBDA_NATIVE"]
            else:
                os.environ["VRT_LAMBDA_NATIVE"] = old
        first = self.make()
        self.rec = [None] + [first.step() for _ in range(6)]
        first.close()

    def _build(self, form, nlam, voro_small):
        L = _lib.load()
        if form == "regular":
            z, x, y, kw = synth.regular_line_case(16, 10, 9, seed=7)
            self.case = vrt.LineCase(**kw)
            self.raster = (z, x, y)
            w, k, dirs = api._regular_directions(QUAD)
            lc, keep = self.case.c_struct()
            n, nlam = int(keep["doppler"].size), int(keep["lam"].size)
            solver = api._regular_solver(z, x, y, n, 0)
            kd, wd = np.ascontiguousarray(k, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
            self.keep = (lc, keep, kd, wd, dirs)
            self.closers.append(solver.close)
            # (a regular handle serves one session at a time: the sessions take turns, every call returns synchronised)
            create = lambda out: L.vrt_regular_lambda_create(solver._h, kd.shape[0], kd.ctypes.data_as(_lib.p_dbl),
                                                             dirs.ctypes.data_as(_lib.p_int), wd.ctypes.data_as(_lib.p_dbl),
                                                             ctypes.byref(lc), 3, out)
            self.args = ("vrt_regular_lambda", create, n, nlam)
            return
        pos, nbr, bounds = voro_small
        self.grid = voro_small
        self.case = small_lambda_case(pos, bounds, 11, *BLOCKS[nlam])
        lc, keep = self.case.c_struct()
        assert int(keep["lam"].size) == nlam
        w, th, ph, _ = vrt.read_quadrature(QUAD)
        wd = np.ascontiguousarray(w, dtype=np.float64)
        self.keep = (lc, keep, wd)
        if form in ("native", "caller"):
            self.sites = vrt.VoronoiSites(pos, nbr, bounds, device=0)
            self.closers.append(self.sites.close)
            plan, _ = api._quadrature_plan(self.sites, QUAD, 3)
            create = lambda out: L.vrt_lambda_create(plan._h, ctypes.byref(lc), wd.ctypes.data_as(_lib.p_dbl), out)
            self.args = ("vrt_lambda", create, pos.shape[0], nlam)
        else:
            self.devices = (0,) * {"multi1": 1, "multi7": 7}.get(form, 2)
            dirs = [1 if t > 90 else -1 for t in th]
            self.weights = w
            self.mp = vrt.MultiDevicePlan(pos, nbr, bounds, vrt.quadrature_directions(th, ph), dirs=dirs, devices=self.devices)
            self.closers.append(self.mp.close)
            create = lambda out: L.vrt_multi_lambda_create(self.mp._h, ctypes.byref(lc), wd.ctypes.data_as(_lib.p_dbl), out)
            self.args = ("vrt_multi_lambda", create, pos.shape[0], nlam)

    def make(self):
        s = _Session(*self.args)
        self.sessions.append(s)
        return s

    def state(self, k):
        """(S, populations) after iterate k of the reference"""
        return self.rec[k][2], self.rec[k][3]

    def release(self):
        """the sessions a test made (the world itself stays for the next test)"""
        for s in self.sessions:
            s.close()
        self.sessions = []

    def close(self):
        self.release()
        for c in reversed(self.closers):
            c()


_worlds = {}


@pytest.fixture(scope="module")
def worlds(voro_small):
    def world(form, nlam):
        if (form, nlam) not in _worlds:
            _worlds[(form, nlam)] = _World(form, nlam, voro_small)
        return _worlds[(form, nlam)]
    yield world
    for w in _worlds.values():
        w.close()
    _worlds.clear()


@pytest.fixture
def world(request, worlds):
    w = worlds(*request.param)
    yield w
    w.release()


def _same(a, b):
    """two results of _Session.step or .get: every array, and the scalar if there is one, bit for bit"""
    return len(a) == len(b) and all(np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q for p, q in zip(a, b))


def _ids(forms):
    return [f"{f}-{n}" if n else f for f, n in forms]


# ---- 1: continuation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", FORMS, indirect=True, ids=_ids(FORMS))
def test_gpu_fresh_session_continues_bit_for_bit(world):
    """A fresh session given the state after iterate 3 returns the scalar, J, S, populations, R and γ of iterates 4, 5, 6."""
    assert all(np.isfinite(r[0]) and r[0] > 0 for r in world.rec[1:])
    assert not np.array_equal(world.rec[3][2], world.rec[6][2])              # the reference did move
    fresh = world.make()
    assert fresh.set_state(*world.state(3)) == 0
    for k in (4, 5, 6):
        got = fresh.step()
        assert got[0] == world.rec[k][0], k
        for name, a, b in zip(("J", "S", "populations", "R", "gamma"), got[1:], world.rec[k][1:]):
            assert np.array_equal(a, b), (k, name)


# ---- 2: round trip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", FORMS, indirect=True, ids=_ids(FORMS))
def test_gpu_set_state_round_trips_through_get(world):
    S3, pops3 = world.state(3)
    s = world.make()
    s.iterate()                                     # (J, R and γ of a session that never iterated are not all defined)
    J1, _, _, R1, g1 = s.get()
    assert s.set_state(S3, pops3) == 0
    J, S, pops, R, g = s.get()
    assert np.array_equal(S, S3) and np.array_equal(pops, pops3)
    # J, R and γ stay those of the last iterate this session ran
    assert np.array_equal(J, J1) and np.array_equal(R, R1) and np.array_equal(g, g1)
    assert np.array_equal(J1, world.rec[1][1]) and np.array_equal(R1, world.rec[1][4]) and np.array_equal(g1, world.rec[1][5])
    # ... and on a session that has not iterated at all
    fresh = world.make()
    assert fresh.set_state(S3, pops3) == 0
    _, S, pops, _, _ = fresh.get()
    assert np.array_equal(S, S3) and np.array_equal(pops, pops3)


# ---- 3: halves ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", FORMS, indirect=True, ids=_ids(FORMS))
def test_gpu_set_state_with_one_half_keeps_the_other(world):
    (S1, pops1), (S3, pops3) = world.state(1), world.state(3)
    assert not np.array_equal(S1, S3) and not np.array_equal(pops1, pops3)
    for S, pops in ((S3, None), (None, pops3)):
        half, both = world.make(), world.make()
        assert half.step()[0] == world.rec[1][0]
        assert half.set_state(S, pops) == 0
        _, S_got, pops_got, _, _ = half.get()
        assert np.array_equal(S_got, S1 if S is None else S3) and np.array_equal(pops_got, pops1 if pops is None else pops3)
        assert both.set_state(S1 if S is None else S3, pops1 if pops is None else pops3) == 0
        want, got = both.step(), half.step()
        assert _same(got, want)
        assert not np.array_equal(got[2], world.rec[2][2])                   # (not simply iterate 2 of the reference)
        world.release()


# ---- 4: refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", FORMS, indirect=True, ids=_ids(FORMS))
def test_gpu_refused_state_leaves_the_session_untouched(world):
    S3, pops3 = world.state(3)
    s = world.make()
    assert s.set_state(S3, pops3) == 0
    n, nlam = s.n, s.nlam
    at_S, at_p = (n // 3, nlam - 1), (1, n - 7)         # (the last wavelength: the last block of a multi-device session)
    bad = []
    for v in (np.nan, 0.0, -1.0):
        Sb = world.rec[5][2].copy()
        Sb[at_S] = v
        bad.append((Sb, world.rec[5][3]))
        bad.append((Sb, None))
    for v in (np.nan, -1.0):
        pb = world.rec[5][3].copy()
        pb[at_p] = v
        bad.append((world.rec[5][2], pb))
        bad.append((None, pb))
    assert len(bad) == 10
    for Sb, pb in bad:
        assert s.set_state(Sb, pb) == _lib.VRT_EINVAL
        assert len(s.L.vrt_last_error() or b"") > 0
    assert s.set_state(None, None) == _lib.VRT_EINVAL
    _, S, pops, _, _ = s.get()
    assert np.array_equal(S, S3) and np.array_equal(pops, pops3)
    assert _same(s.step(), world.rec[4])                # the next iterate is the one it would have run anyway
    # a zero population is a state (an empty level), not an error
    pz = pops3.copy()
    pz[2, 5] = 0.0
    assert s.set_state(None, pz) == 0


# ---- 5: Ng --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", NG_FORMS, indirect=True, ids=_ids(NG_FORMS))
def test_gpu_state_after_an_ng_step_resumes_in_a_plain_session(world):
    """What *_get returns right after an accepted step is the extrapolated S (in both sweep-order copies); a plain session
    given it continues as the accelerated one does with acceleration switched off."""
    acc = world.make()
    acc.accelerate(2, 4, 4)
    for k in (1, 2, 3, 4):
        assert acc.iterate() == world.rec[k][0]         # the scalar is that of the plain update
    assert acc.applied() == 1
    _, S4x, pops4, _, _ = acc.get()
    assert not np.array_equal(S4x, world.rec[4][2]) and np.array_equal(pops4, world.rec[4][3])
    acc.accelerate(0, 0, 0)
    plain = world.make()
    assert plain.set_state(S4x, pops4) == 0
    for k in (5, 6, 7):
        want, got = acc.step(), plain.step()
        assert _same(got, want), k
    assert not np.array_equal(got[2], world.rec[6][2])


@pytest.mark.parametrize("world", NG_FORMS, indirect=True, ids=_ids(NG_FORMS))
def test_gpu_set_state_drops_the_ng_history(world):
    """Settings (2, 4, 4): steps fall due after iterates 4, 8, 12, each from the three iterates recorded before it.  Right
    after set_state nothing is reported as applied, and a step is taken only once three further iterates are recorded:
    set after iterate 4, the next step is that of iterate 8 and none comes earlier; set after iterate 5 -- one of the three
    already recorded -- the step due at 8 finds an incomplete history and is not taken, the next is that of iterate 12."""
    s = world.make()
    s.accelerate(2, 4, 4)
    for _ in range(4):
        s.iterate()
    assert s.applied() == 1
    _, S, pops, _, _ = s.get()
    assert s.set_state(S, pops) == 0
    assert s.applied() == 0
    for k in (5, 6, 7, 8):
        s.iterate()
        assert (s.applied() != 0) == (k == 8), k
    late = world.make()
    late.accelerate(2, 4, 4)
    for _ in range(5):
        late.iterate()
    _, S, pops, _, _ = late.get()
    assert late.set_state(S, pops) == 0
    assert late.applied() == 0
    for k in range(6, 13):
        late.iterate()
        assert (late.applied() != 0) == (k == 12), k


# ---- 6: Python ----------------------------------------------------------------------------------------------------------------
def _check_resumed_run(run, path):
    """run(maxiter, **kw) -> (J, S, populations, history): three iterates with a checkpoint, three more from it, against six"""
    full = run(6)
    first = run(3, checkpoint=path)
    ck = api.read_checkpoint(path)
    assert ck["iterate"] == 3 and ck["history"] == first[3] == full[3][:3]
    assert np.array_equal(ck["S"], first[1]) and np.array_equal(ck["populations"], first[2])
    second = run(3, resume=path, checkpoint=path, checkpoint_every=2)
    assert second[3] == full[3] and len(second[3]) == 6
    for a, b in zip(second[:3], full[:3]):
        assert np.array_equal(a, b)
    ck = api.read_checkpoint(path)                       # written after new iterate 2 and after the last
    assert ck["iterate"] == 6 and ck["history"] == full[3] and np.array_equal(ck["S"], full[1])
    # the same through the arrays, and a state the session refuses
    third = run(3, S0=first[1], populations0=first[2])
    assert third[3] == full[3][3:] and all(np.array_equal(a, b) for a, b in zip(third[:3], full[:3]))
    bad = first[1].copy()
    bad[3, 0] = 0.0
    with pytest.raises(vrt.VrtError) as e:
        run(1, S0=bad)
    assert e.value.code == _lib.VRT_EINVAL
    with pytest.raises(ValueError):
        run(1, S0=first[1][:, :-1])
    return full


@pytest.mark.parametrize("world", [("native", 9)], indirect=True, ids=["native-9"])
def test_gpu_lambda_voronoi_host_checkpoint_and_resume(world, tmp_path):
    run = lambda maxiter, **kw: vrt.Lambda_voronoi_host(0.0, maxiter, world.sites, world.case, QUAD, **kw)
    full = _check_resumed_run(run, str(tmp_path / "run.npz"))
    assert full[3] == [r[0] for r in world.rec[1:]] and np.array_equal(full[1], world.rec[6][2])


@pytest.mark.parametrize("world", [("regular", 0)], indirect=True, ids=["regular"])
def test_gpu_lambda_regular_checkpoint_and_resume(world, tmp_path):
    z, x, y = world.raster
    run = lambda maxiter, **kw: vrt.Lambda_regular(0.0, maxiter, z, x, y, world.case, QUAD, **kw)
    full = _check_resumed_run(run, str(tmp_path / "run.npz"))
    assert full[3] == [r[0] for r in world.rec[1:]] and np.array_equal(full[1], world.rec[6][2])


@pytest.mark.parametrize("world", [("multi1", 9), ("multi2", 9)], indirect=True, ids=["multi1-9", "multi2-9"])
def test_gpu_multi_device_lambda_iteration_checkpoint_and_resume(world, tmp_path):
    run = lambda maxiter, **kw: world.mp.lambda_iteration(0.0, maxiter, world.case, world.weights, **kw)
    full = _check_resumed_run(run, str(tmp_path / "run.npz"))
    assert full[3] == [r[0] for r in world.rec[1:]] and np.array_equal(full[1], world.rec[6][2])


@pytest.mark.parametrize("native", [False, True])
@pytest.mark.parametrize("world", [("native", 9)], indirect=True, ids=["native-9"])
def test_gpu_lambda_voronoi_starts_from_given_arrays(world, native):
    """the torch-driven loop: three of its own iterates, three more from their S and populations, against six"""
    run = lambda maxiter, **kw: vrt.Lambda_voronoi(0.0, maxiter, world.sites, world.case, QUAD, native=native, **kw)
    full, first = run(6), run(3)
    second = run(3, S0=first[1], populations0=first[2])
    assert second[3] == full[3][3:] and first[3] == full[3][:3]
    for a, b in zip(second[:3], full[:3]):
        assert np.array_equal(a, b)
    bad = first[1].copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        run(1, S0=bad)
