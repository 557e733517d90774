"""Accelerated Λ-iteration with the diagonal operator Λ* on the regular-grid LINE session, on the device:
vrt_regular_line_lambda_diagonal[_dev], vrt_regular_lambda_use_operator / _get_operator and api.line_lambda_diagonal_regular /
Lambda_regular(operator="diagonal"), against the continuum's Λ* kernel angle by angle (bit for bit), the oracle's one-sweep
unit response with an α per angle and the oracle-driven ALI loop (tests/test_regular_line_ali_host.py) on the 6 x 6 x 6
ghosted raster of line_case_644.

Tolerances: Λ* against the unit response 1e-12 of its maximum (tests/test_regular_ali.py); the session against the oracle
loop as test_regular_lambda.test_gpu_lambda_regular_matches_oracle_loop (J to 1e-9 of its maximum, S and the populations
to 1e-9 relative, the history to rtol 1e-8); everything else is bit for bit."""
import ctypes

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib, api, synth
from test_line_ali_host import fixed_point_bound, hard_case
from test_regular_ali_host import ghost_mask
from test_regular_lambda import MIXED, STEEP
from test_regular_line_ali_host import (COUNTS, MARGIN, QUAD, TARGET, first_iterate_reference, line_case_644,
                                        oracle_regular_line_loop)

pytestmark = pytest.mark.gpu

# iterates of the device session to TARGET on the hard variant with the operator on and Ng(4, 4), measured by
# test_gpu_regular_line_ali_composes_with_ng (the ALI count without Ng: COUNTS["hard"][1] = 35)
NG_COUNT_HARD = 21

d = lambda a: a.ctypes.data_as(_lib.p_dbl)
pi = lambda a: a.ctypes.data_as(_lib.p_int)


# ---- rasters and α of the kernel tests ----------------------------------------------------------------------------------------
def _axes(nz, nx, ny, seed):
    """ghosted axes of nz x nx x ny points: uneven z, even x and y of different spacing"""
    rng = np.random.default_rng(seed)
    z = np.cumsum(0.5 + rng.random(nz)) * 1.0e5
    return z, 1.3e5 * np.arange(nx, dtype=np.float64), 0.9e5 * np.arange(ny, dtype=np.float64)


def _raster(name):
    if name == "16x12x11":                                  # the raster of test_regular_lambda.raster
        z, x, y, _ = synth.regular_line_case(16, 10, 9, seed=7)
        return z, x, y
    nz, nx, ny = {"2x3x4": (2, 3, 4), "3x4x3": (3, 4, 3), "5x3x3": (5, 3, 3), "4x4x4": (4, 4, 4)}[name]
    return _axes(nz, nx, ny, seed=nz + 10 * nx + 100 * ny)


def _alpha(z, x, y, n_angles, nlam, seed):
    """random per-angle α (n_angles, n, nlam) with Δτ = α dz from 1e-3 to 1e3, the ghost border wrapped from the interior"""
    rng = np.random.default_rng(seed)
    dz = np.diff(z).mean() if z.size > 1 else 1.0
    inner = 10.0 ** rng.uniform(-3, 3, (n_angles, y.size - 2, x.size - 2, z.size, nlam)) / dz
    full = np.pad(inner, [(0, 0), (1, 1), (1, 1), (0, 0), (0, 0)], mode="wrap")
    return np.ascontiguousarray(full.reshape(n_angles, -1, nlam))


def _quadrature(tmp_path, name):
    if name == "ul7n12":
        return QUAD
    p = tmp_path / ("mixn5.dat" if name == "mixed" else "steepn4.dat")          # (the point count is read off the name)
    p.write_text(MIXED if name == "mixed" else STEEP)
    return str(p)


def _to_planes(rows, z, x, y):
    """(n, nlam) rows in Julia point order -> [l][iz][iy][ix]"""
    return np.ascontiguousarray(rows.reshape(y.size, x.size, z.size, -1).transpose(3, 2, 0, 1))


def _from_planes(planes, z, x, y):
    return np.ascontiguousarray(planes.transpose(2, 3, 1, 0).reshape(y.size * x.size * z.size, -1))


# ---- 1: the kernel against the continuum kernel, angle by angle ------------------------------------------------------------------
@pytest.mark.parametrize("quad", ["ul7n12", "mixed", "steep"])
@pytest.mark.parametrize("shape", ["16x12x11", "2x3x4", "3x4x3", "5x3x3", "4x4x4"])
def test_gpu_line_diagonal_is_the_sum_of_the_continuum_kernel_angle_by_angle(tmp_path, shape, quad):
    """Λ*_line = Σ_a (vrt_regular_lambda_diagonal_dev with only angle a active, on angle a's α), added on the host in angle
    order: bit for bit, by the host entry and by the device entry on plane-major arrays; interior rows of one and two points,
    two planes, an inactive θ = 90 angle (mixed) whose α -- NaN here -- is never read"""
    import torch
    z, x, y = _raster(shape)
    q = _quadrature(tmp_path, quad)
    w, k, dirs = api._regular_directions(q)
    nq, n = k.shape[0], z.size * x.size * y.size
    L = _lib.load()
    dev = torch.device("cuda", 0)
    solver = api._regular_solver(z, x, y, n, 0)
    try:
        for nlam in (1, 2, 5):
            alpha = _alpha(z, x, y, nq, nlam, seed=nlam)
            alpha[dirs == 0] = np.nan
            want = np.zeros((n, nlam))
            for a in np.flatnonzero(dirs):
                only = np.zeros_like(dirs)
                only[a] = dirs[a]
                d_alpha = torch.from_numpy(alpha[a]).to(dev)
                d_diag = torch.full((n, nlam), -7.0, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                assert L.vrt_regular_lambda_diagonal_dev(solver._h, nq, d(k), pi(only), d(w), nlam, nlam, d_alpha.data_ptr(),
                                                         d_diag.data_ptr()) == 0
                want = want + d_diag.cpu().numpy()
            got = vrt.line_lambda_diagonal_regular(z, x, y, alpha, q)
            assert np.array_equal(got, want), (nlam, np.abs(got - want).max())
            ghost = ghost_mask(z, x, y)
            assert (got[ghost] == 0.0).all() and (got >= 0).all() and (got < 1).all()
            if z.size > 2:
                assert (got.reshape(y.size, x.size, z.size, nlam)[1:-1, 1:-1, 1:-1] > 0).all()
            # the device entry: α plane-major per ACTIVE angle, Λ* plane-major, every element written
            planes = np.stack([_to_planes(alpha[a], z, x, y) for a in np.flatnonzero(dirs)])
            d_alpha_pl = torch.from_numpy(planes).to(dev)
            d_diag_pl = torch.full((nlam, z.size, y.size, x.size), -7.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            assert L.vrt_regular_line_lambda_diagonal_dev(solver._h, nq, d(k), pi(dirs), d(w), nlam, d_alpha_pl.data_ptr(),
                                                          d_diag_pl.data_ptr(), None) == 0
            assert np.array_equal(_from_planes(d_diag_pl.cpu().numpy(), z, x, y), want)
    finally:
        solver.close()


def test_gpu_line_diagonal_host_form_pads_and_checks_alpha(tmp_path):
    """ld > nlam: the padding columns (NaN in α, -7 in diag) are neither read nor written; α that is read must be finite and
    > 0 (VRT_EINVAL, diag untouched), the block of an inactive angle is not read at all"""
    z, x, y = _raster("4x4x4")
    q = _quadrature(tmp_path, "mixed")
    w, k, dirs = api._regular_directions(q)
    nq, n = k.shape[0], z.size * x.size * y.size
    alpha = _alpha(z, x, y, nq, 3, seed=5)
    want = vrt.line_lambda_diagonal_regular(z, x, y, alpha, q)
    wide = np.full((nq, n, 5), np.nan)
    wide[:, :, :3] = alpha
    wide[dirs == 0] = np.nan
    L = _lib.load()
    solver = api._regular_solver(z, x, y, n, 0)
    try:
        host = np.full((n, 5), -7.0)
        assert L.vrt_regular_line_lambda_diagonal(solver._h, nq, d(k), pi(dirs), d(w), 3, 5, d(wide), d(host)) == 0
        assert np.array_equal(host[:, :3], want) and (host[:, 3:] == -7.0).all()
        active = int(np.flatnonzero(dirs)[-1])
        for bad in (0.0, -1.0, np.nan, np.inf):
            wide_bad = wide.copy()
            wide_bad[active, 5, 2] = bad
            host_bad = np.full((n, 5), -7.0)
            assert L.vrt_regular_line_lambda_diagonal(solver._h, nq, d(k), pi(dirs), d(w), 3, 5, d(wide_bad),
                                                      d(host_bad)) == _lib.VRT_EINVAL
            assert (host_bad == -7.0).all()
    finally:
        solver.close()


# ---- 2: zero velocity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad", ["ul7n12", "mixed"])
def test_gpu_line_diagonal_with_one_alpha_for_all_angles_is_the_continuum_diagonal(tmp_path, quad):
    z, x, y = _raster("16x12x11")
    q = _quadrature(tmp_path, quad)
    nq = api._regular_directions(q)[1].shape[0]
    alpha = _alpha(z, x, y, 1, 5, seed=9)[0]
    got = vrt.line_lambda_diagonal_regular(z, x, y, np.broadcast_to(alpha, (nq,) + alpha.shape), q)
    assert np.array_equal(got, vrt.lambda_diagonal_regular(z, x, y, alpha, q))


# ---- 3: the kernel against the oracle's unit response ---------------------------------------------------------------------------
def test_gpu_line_diagonal_matches_the_oracle_unit_response():
    z, x, y, _ = line_case_644()
    alpha, ref = first_iterate_reference()
    got = vrt.line_lambda_diagonal_regular(z, x, y, alpha, QUAD)
    print(f"max-norm {np.abs(got - ref).max() / np.abs(ref).max():.3g}")
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert (got[ghost_mask(z, x, y)] == 0.0).all()


# ---- the session, hand-driven ---------------------------------------------------------------------------------------------------
class _Session:
    """vrt_regular_lambda_* called directly on a solver of its own"""

    def __init__(self, z, x, y, case, quadrature=QUAD):
        self.L = _lib.load()
        w, k, dirs = api._regular_directions(quadrature)
        lc, keep = case.c_struct()
        self.n, self.nlam = int(keep["doppler"].size), int(keep["lam"].size)
        self.solver = api._regular_solver(z, x, y, self.n, 0)
        self.keep = (lc, keep, w, k, dirs)
        self.h = ctypes.c_void_p()
        rc = self.L.vrt_regular_lambda_create(self.solver._h, k.shape[0], d(k), pi(dirs), d(w), ctypes.byref(lc), 3,
                                              ctypes.byref(self.h))
        assert rc == 0, rc

    def iterate(self):
        c = ctypes.c_double()
        assert self.L.vrt_regular_lambda_iterate(self.h, ctypes.byref(c)) == 0
        return c.value

    def get(self):
        J, S, pops = np.zeros((self.n, self.nlam)), np.zeros((self.n, self.nlam)), np.zeros((3, self.n))
        assert self.L.vrt_regular_lambda_get(self.h, d(J), d(S), d(pops), None, None) == 0
        return J, S, pops

    def set_state(self, S, pops):
        S, pops = np.ascontiguousarray(S), np.ascontiguousarray(pops)
        assert self.L.vrt_regular_lambda_set_state(self.h, d(S), d(pops)) == 0

    def use_operator(self, op):
        return self.L.vrt_regular_lambda_use_operator(self.h, op)

    def operator(self):
        op, cnt = ctypes.c_int(-1), ctypes.c_int64(-1)
        assert self.L.vrt_regular_lambda_get_operator(self.h, ctypes.byref(op), ctypes.byref(cnt)) == 0
        assert self.L.vrt_regular_lambda_get_operator(self.h, ctypes.byref(op), None) == 0
        return op.value, cnt.value

    def close(self):
        if self.h:
            self.L.vrt_regular_lambda_destroy(self.h)
            self.h = ctypes.c_void_p()
        if self.solver is not None:
            self.solver.close()
            self.solver = None


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


# ---- 4: chunking ----------------------------------------------------------------------------------------------------------------
def test_gpu_regular_line_ali_bit_identical_under_chunking(monkeypatch):
    """one solve per chunk, four (with nλ = 9 the chunk edges fall inside an angle's wavelengths) and the default: three ALI
    iterates give the same J, S, populations and history.  VRT_REG_LAMBDA_BYTES is read when the regular handle is made; a
    solve's workspace is 8 (2 vol + 5 plane) bytes."""
    z, x, y, case = line_case_644()
    assert case.B0.shape[1] == 9
    vol, plane = z.size * x.size * y.size, x.size * y.size
    ref = vrt.Lambda_regular(0.0, 3, z, x, y, case, QUAD, operator="diagonal")
    for nbytes in (1, 4 * 8 * (2 * vol + 5 * plane)):
        monkeypatch.setenv("VRT_REG_LAMBDA_BYTES", str(nbytes))
        got = vrt.Lambda_regular(0.0, 3, z, x, y, case, QUAD, operator="diagonal")
        assert _same(ref[:3], got[:3]) and ref[3] == got[3], nbytes
    monkeypatch.delenv("VRT_REG_LAMBDA_BYTES")
    assert not np.array_equal(ref[1], vrt.Lambda_regular(0.0, 3, z, x, y, case, QUAD)[1])       # the operator does act


# ---- 5: the session against the oracle-driven ALI loop --------------------------------------------------------------------------
def test_gpu_regular_line_ali_session_matches_oracle_loop():
    z, x, y, case = line_case_644()
    J_ref, S_ref, pops_ref, hist_ref, seen = oracle_regular_line_loop(case, z, x, y, 6, 0.0, ali=True)
    assert seen["fallback"] == 0
    s = _Session(z, x, y, case)
    try:
        assert s.operator() == (0, 0)
        assert s.use_operator(1) == 0 and s.operator() == (1, 0)
        hist = []
        for _ in range(6):
            hist.append(s.iterate())
            assert s.operator() == (1, 0)                              # no entry fell back to the plain update
        J, S, pops = s.get()
    finally:
        s.close()
    print(f"J {np.abs(J - J_ref).max() / np.abs(J_ref).max():.3g}, S {np.abs(S / S_ref - 1).max():.3g}, "
          f"pops {np.abs(pops / pops_ref - 1).max():.3g}")
    assert np.abs(J - J_ref).max() < 1e-9 * np.abs(J_ref).max()
    assert np.abs(S / S_ref - 1).max() < 1e-9
    assert np.abs(pops / pops_ref - 1).max() < 1e-9
    assert np.allclose(hist, hist_ref, rtol=1e-8)


# ---- 6: off again ---------------------------------------------------------------------------------------------------------------
def test_gpu_regular_line_ali_switched_off_again_is_the_plain_session():
    z, x, y, case = line_case_644()
    a, b = _Session(z, x, y, case), _Session(z, x, y, case)
    try:
        assert a.use_operator(1) == 0 and a.use_operator(1) == 0 and a.use_operator(0) == 0 and a.operator() == (0, 0)
        assert a.use_operator(2) == _lib.VRT_EINVAL and a.use_operator(-1) == _lib.VRT_EINVAL and a.operator() == (0, 0)
        assert [a.iterate() for _ in range(3)] == [b.iterate() for _ in range(3)]
        assert _same(a.get(), b.get())
        # between two iterates: one ALI iterate moves S away from the plain run, and off again the update is the plain one
        assert a.use_operator(1) == 0
        a.iterate(), b.iterate()
        assert not np.array_equal(a.get()[1], b.get()[1])
        assert a.use_operator(0) == 0
        b.set_state(*a.get()[1:])
        assert a.iterate() == b.iterate() and _same(a.get(), b.get())
    finally:
        a.close()
        b.close()


# ---- 7: iterate counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["standard", "hard"])
def test_gpu_regular_line_ali_stops_at_the_oracle_counts(name):
    z, x, y, case = line_case_644()
    if name == "hard":
        case = hard_case(case)
    cap = max(COUNTS[name]) + 50
    plain = vrt.Lambda_regular(TARGET, cap, z, x, y, case, QUAD)
    ali = vrt.Lambda_regular(TARGET, cap, z, x, y, case, QUAD, operator="diagonal")
    n_plain, n_ali = len(plain[3]), len(ali[3])
    bound = fixed_point_bound(plain[3], ali[3])
    dist = np.abs(ali[1] / plain[1] - 1).max()
    print(f"{name}: plain {n_plain} iterates, ALI {n_ali} to {TARGET:g}; |S_ali / S_plain - 1| = {dist:.3g}, bound {bound:.3g}")
    assert abs(n_plain - COUNTS[name][0]) <= MARGIN and abs(n_ali - COUNTS[name][1]) <= MARGIN
    assert plain[3][-1] <= TARGET and ali[3][-1] <= TARGET
    assert dist < bound                                                  # one fixed point


# ---- 8: Ng -----------------------------------------------------------------------------------------------------------------------
def test_gpu_regular_line_ali_composes_with_ng():
    z, x, y, case = line_case_644()
    case = hard_case(case)
    cap = COUNTS["hard"][1] + 50
    ali = vrt.Lambda_regular(TARGET, cap, z, x, y, case, QUAD, operator="diagonal")
    J, S, pops, hist, steps = vrt.Lambda_regular(TARGET, cap, z, x, y, case, QUAD, operator="diagonal", ng=(4, 4))
    print(f"hard: ALI {len(ali[3])} iterates, ALI + Ng(4, 4) {len(hist)}; steps {[(i, ok) for i, ok, _, _ in steps]}")
    assert hist[-1] <= TARGET and np.isfinite(S).all() and (S > 0).all() and (pops > 0).all()
    assert any(ok == 1 for _, ok, _, _ in steps)
    assert len(hist) <= len(ali[3])
    assert abs(len(hist) - NG_COUNT_HARD) <= MARGIN


# ---- 9: resume -------------------------------------------------------------------------------------------------------------------
def test_gpu_regular_line_ali_resumes_bit_for_bit():
    z, x, y, case = line_case_644()
    a, b = _Session(z, x, y, case), _Session(z, x, y, case)
    try:
        assert a.use_operator(1) == 0
        for _ in range(3):
            a.iterate()
        _, S, pops = a.get()
        assert b.use_operator(1) == 0
        b.set_state(S, pops)
        assert [a.iterate() for _ in range(3)] == [b.iterate() for _ in range(3)]
        assert _same(a.get(), b.get())
    finally:
        a.close()
        b.close()


# ---- 10: Python -----------------------------------------------------------------------------------------------------------------
def test_gpu_lambda_regular_operator_is_the_hand_driven_session(tmp_path):
    z, x, y, case = line_case_644()
    s = _Session(z, x, y, case)
    try:
        assert s.use_operator(1) == 0
        hist = [s.iterate() for _ in range(4)]
        want = s.get()
    finally:
        s.close()
    J, S, pops, h = vrt.Lambda_regular(0.0, 4, z, x, y, case, QUAD, operator="diagonal")
    assert h == hist and _same((J, S, pops), want)
    # with a checkpoint and resume: two iterates, then two more from the file
    ck = str(tmp_path / "run.npz")
    vrt.Lambda_regular(0.0, 2, z, x, y, case, QUAD, operator="diagonal", checkpoint=ck)
    J2, S2, pops2, h2 = vrt.Lambda_regular(0.0, 2, z, x, y, case, QUAD, operator="diagonal", resume=ck)
    assert h2 == hist and _same((J2, S2, pops2), want)
