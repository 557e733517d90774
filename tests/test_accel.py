"""Ng acceleration of the Λ-iteration on the device: vrt_ng_accelerate_dev (the reduction and the apply kernel), the
acceleration of the two single-device sessions (vrt_lambda_*, vrt_regular_lambda_*) and the `ng` keyword of
api.Lambda_voronoi_host / api.Lambda_regular.

CPU reference (numpy, here): the per-element terms in the library's order of operations, each of the five sums by
math.fsum (exact), then the host formulas for a, b, c and x_acc.

THE BOUND ON A SUM: 2^-40 Σ|t_i|.  The terms are bit-identical by construction, and a summation whose longest chain of
additions has L links errs by at most L 2^-53 Σ|t_i| to first order (Higham, Accuracy and Stability of Numerical
Algorithms, §4.2); 2^-40 admits L <= 8192.  The kernel's L at the largest array a session can hold (4 M sites x 100
wavelengths) is 122 (derived beside k_ng_sums in csrc/vrt_accel.hip).
THE BOUND ON a, b (δa, δb): the first-order image of that bound through the 2 x 2 solve, δa = 2 Σ_k |∂a/∂s_k| 2^-40 Σ|t_k|
with the analytic partial derivatives, the 2 for the neglected second order."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import _lib, api, synth
from test_physics import _lambda_case
from test_regular_lambda import _oracle_J

QUAD = "ul7n12.dat"
SUM_BOUND = 2.0 ** -40      # x Σ|t_i|: L <= 8192 links of 2^-53 each; the kernel's L is 122 at 4 M sites x 100 wavelengths


# ---- the numpy reference -------------------------------------------------------------------------------------------------
def _fsum(t):
    """exact sum of a (large) array without a Python list of its whole length"""
    flat = t.reshape(-1)
    step = 1 << 22
    return math.fsum(itertools.chain.from_iterable(flat[i:i + step].tolist() for i in range(0, flat.size, step)))


def _coefficients(sums):
    """the host formulas, operation for operation"""
    A1, B1, C1, B2, C2 = (np.float64(v) for v in sums)
    with np.errstate(all="ignore"):                 # (det == 0: IEEE quotients, as the library's host code forms them)
        det = A1 * B2 - B1 * B1
        a = (C1 * B2 - C2 * B1) / det
        b = (C2 * A1 - C1 * B1) / det
        return float(a), float(b), float((1.0 - a) - b)


def _apply(a, b, x0, x1, x2):
    c = (1.0 - a) - b
    return (c * x0 + a * x1) + b * x2


def _reference(x0, x1, x2, x3, result=True):
    """sums (fsum), Σ|t| per sum, a, b, x_acc, δa, δb"""
    w = 1.0 / x0
    q1 = (x0 - 2.0 * x1) + x2
    q2 = ((x0 - x1) - x2) + x3
    q3 = x0 - x1
    wq1, wq2 = w * q1, w * q2
    del w
    sums, mags = [], []
    for u, v in ((wq1, q1), (wq1, q2), (wq1, q3), (wq2, q2), (wq2, q3)):
        t = u * v
        sums.append(_fsum(t))
        mags.append(_fsum(np.abs(t)) if t.size < (1 << 22) else float(np.abs(t).sum()) * (1 + 1e-6))
        del t
    del q1, q2, q3, wq1, wq2
    sums, mags = np.array(sums), np.array(mags)
    ref = {"sums": sums, "mags": mags}
    A1, B1, C1, B2, C2 = sums
    det = A1 * B2 - B1 * B1
    if det != 0 and np.isfinite(det):
        a, b, c = _coefficients(sums)
        da_ds = np.array([-a * B2, -C2 + 2 * a * B1, B2, C1 - a * A1, -B1]) / det
        db_ds = np.array([C2 - b * B2, -C1 + 2 * b * B1, -B1, -b * A1, A1]) / det
        ref.update(a=a, b=b, da=2 * float(np.abs(da_ds) @ (SUM_BOUND * mags)), db=2 * float(np.abs(db_ds) @ (SUM_BOUND * mags)))
        if result:
            ref["x_acc"] = _apply(a, b, x0, x1, x2)
    return ref


def _iterates(count, seed):
    """positive random x whose successive iterates differ by relative 1e-1 ... 1e-6"""
    rng = np.random.default_rng(seed)
    xs = [1.0 + rng.random(count)]
    for _ in range(3):
        step = 10.0 ** rng.uniform(-6, -1, count)
        step *= np.where(rng.random(count) < 0.5, -1.0, 1.0)
        xs.append(xs[-1] * (1.0 + step))
    return xs


def _geometric(l1, l2, N=200_000, seed=3):
    rng = np.random.default_rng(seed)
    xs = rng.uniform(1.0, 2.0, N)
    u, v = 0.1 * rng.normal(size=N), 0.1 * rng.normal(size=N)
    return xs, [xs + l1 ** k * u + l2 ** k * v for k in range(4)]


# ---- the device call on torch tensors -------------------------------------------------------------------------------------
def _device(xs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in xs]


def _accelerate(d):
    import torch
    out = torch.full_like(d[0], -7.0)
    applied, sums, coeffs = api.ng_accelerate_dev(d[0].numel(), *(t.data_ptr() for t in d), out.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream)
    return applied, sums, coeffs, out


# ---- 1, 2: sums, coefficients, result ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097, 1_000_003, 2 ** 26 + 3])
def test_gpu_ng_sums_coefficients_and_result(count):
    xs = _iterates(count, seed=count % 1000)
    ref = _reference(*xs, result=False)
    d = _device(xs)
    applied, sums, coeffs, out = _accelerate(d)
    err = np.abs(sums - ref["sums"])
    print(f"count {count}: |sum - fsum| / Σ|t| = {err / ref['mags']}, bound {SUM_BOUND:.3e}; a, b = {coeffs}")
    assert (err <= SUM_BOUND * ref["mags"]).all(), (sums, ref["sums"], ref["mags"])
    # run to run: identical bits
    applied2, sums2, coeffs2, out2 = _accelerate(d)
    assert applied2 == applied and sums2.tobytes() == sums.tobytes() and coeffs2.tobytes() == coeffs.tobytes()
    # the coefficients are the host formulas applied to the RETURNED sums, bit for bit
    a, b, c = _coefficients(sums)
    if not (math.isfinite(a) and math.isfinite(b)):        # a singular system (one element: rank 1) is rejected
        assert not applied
        return
    assert np.array([a, b]).tobytes() == coeffs.tobytes()
    if applied:
        x_acc = out.cpu().numpy()
        assert np.array_equal(x_acc, _apply(a, b, xs[0], xs[1], xs[2]))
        assert np.array_equal(x_acc, out2.cpu().numpy())
        assert np.isfinite(x_acc).all() and (x_acc > 0).all()
    else:                                          # a rejection must be one the rules call for
        x_acc = _apply(a, b, xs[0], xs[1], xs[2])
        assert not (np.isfinite(x_acc).all() and (x_acc > 0).all())


@pytest.mark.gpu
def test_gpu_ng_accelerate_takes_unaligned_arrays_with_the_same_bits():
    """arrays that start 8 bytes off a 16-byte boundary take the scalar loads: the same assignment of elements to
    accumulators, so the same sums bit for bit"""
    import torch
    count = 100_001
    xs = _iterates(count, seed=17)
    d = _device(xs)
    _, sums, coeffs, out = _accelerate(d)
    pad = [torch.empty(count + 1, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    off = []
    for p, t in zip(pad, d):
        p[1:] = t
        off.append(p[1:])
        assert off[-1].data_ptr() % 16 == 8
    _, sums_u, coeffs_u, out_u = _accelerate(off)
    assert sums_u.tobytes() == sums.tobytes() and coeffs_u.tobytes() == coeffs.tobytes()
    assert torch.equal(out, out_u)


@pytest.mark.gpu
def test_gpu_ng_accelerate_host_arrays():
    x_star, xs = _geometric(0.9, 0.5, N=2000)
    xs = [x.reshape(50, 40) for x in xs]
    x_acc, sums, coeffs = vrt.api.ng_accelerate(*xs)
    assert x_acc.shape == (50, 40) and np.abs(x_acc - x_star.reshape(50, 40)).max() < 1e-9
    assert np.array_equal(x_acc, _apply(coeffs[0], coeffs[1], xs[0], xs[1], xs[2]))


# ---- 3: it extrapolates -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("l1,l2", [(0.9, 0.5), (0.99, 0.9), (0.95, -0.3)])
def test_gpu_ng_returns_the_limit_of_two_geometric_modes(l1, l2):
    """x_k = x* + λ1^k u + λ2^k v, k = 0..3: second-order Ng returns x* in exact arithmetic"""
    x_star, xs = _geometric(l1, l2)
    ref = _reference(*xs)
    e_ref = np.abs(ref["x_acc"] - x_star).max()
    applied, sums, coeffs, out = _accelerate(_device(xs))
    assert applied
    e = np.abs(out.cpu().numpy() - x_star).max()
    delta = ref["da"] * np.abs(xs[1] - xs[0]).max() + ref["db"] * np.abs(xs[2] - xs[0]).max()
    before = np.abs(xs[0] - x_star).max()
    print(f"λ = ({l1}, {l2}): error before {before:.3g}, device {e:.3g}, reference {e_ref:.3g}, Δ {delta:.3g}")
    assert e <= e_ref + delta
    assert abs(coeffs[0] - ref["a"]) <= ref["da"] and abs(coeffs[1] - ref["b"]) <= ref["db"]


# ---- 4: rejection -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_ng_rejects_a_step_that_leaves_the_positive_numbers():
    x_star, xs = _geometric(0.9, 0.5, N=50_000)
    j = 31_337
    # one element converging to -0.01 from positive iterates (0.49, 0.44, 0.395, 0.3545)
    for k in range(4):
        xs[k][j] = -0.01 + 0.9 ** k * 0.5
    assert all((x > 0).all() for x in xs)
    ref = _reference(*xs)
    assert ref["x_acc"][j] < 0 and (np.delete(ref["x_acc"], j) > 0).all()
    applied, sums, coeffs, _ = _accelerate(_device(xs))
    assert not applied
    assert abs(coeffs[0] - ref["a"]) <= ref["da"] and abs(coeffs[1] - ref["b"]) <= ref["db"]
    # ... and the same history without that element is taken
    ok = [np.delete(x, j) for x in xs]
    assert _accelerate(_device(ok))[0]


@pytest.mark.gpu
def test_gpu_ng_rejects_four_equal_arrays():
    x = 1.0 + np.random.default_rng(5).random(10_000)
    applied, sums, coeffs, _ = _accelerate(_device([x, x, x, x]))
    assert not applied and not sums.any()           # det == 0
    x_acc, sums, coeffs = vrt.api.ng_accelerate(x, x, x, x)
    assert x_acc is None


# ---- sessions ---------------------------------------------------------------------------------------------------------------
class _Session:
    """vrt_lambda_* or vrt_regular_lambda_* through ctypes"""

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

    def accelerate(self, order, start, period):
        _lib.check(self.fn("set_acceleration")(self.h, order, start, period))

    def last(self):
        applied, sums, coeffs = ctypes.c_int(9), np.zeros(5), np.zeros(2)
        _lib.check(self.fn("last_acceleration")(self.h, ctypes.byref(applied), sums.ctypes.data_as(_lib.p_dbl),
                                                coeffs.ctypes.data_as(_lib.p_dbl)))
        return applied.value, sums, coeffs

    def get(self):
        n, nlam = self.n, self.nlam
        out = [np.zeros((n, nlam)), np.zeros((n, nlam)), np.zeros((3, n)), np.zeros((n, 3, 3)), np.zeros(n)]
        _lib.check(self.fn("get")(self.h, *(a.ctypes.data_as(_lib.p_dbl) for a in out)))
        return out                                  # J, S, populations, R, gamma

    def close(self):
        if self.h:
            self.fn("destroy")(self.h)
            self.h = ctypes.c_void_p()


def _voronoi_sessions(voro_small, count):
    pos, nbr, bounds = voro_small
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    case = _lambda_case(pos, bounds, 11)
    plan, w = api._quadrature_plan(hs, QUAD, 3)
    lc, keep = case.c_struct()
    wd = np.ascontiguousarray(w, dtype=np.float64)
    create = lambda out: _lib.load().vrt_lambda_create(plan._h, ctypes.byref(lc), wd.ctypes.data_as(_lib.p_dbl), out)
    sessions = [_Session("vrt_lambda", create, hs.n, int(keep["lam"].size)) for _ in range(count)]
    return hs, case, sessions, (lc, keep, wd)


def _voronoi_oracle_step(case, so, S_old, pops):
    """one pass of the loop body of test_physics._oracle_lambda_iteration from (S_old, pops)"""
    w, th, ph, nq = vrt.read_quadrature(QUAD)
    bottom = so.perm_up[: so.layers_up[1] - 1] - 1
    gamma, strength = orc.line_terms(case.gamma_static, case.gamma_unsold, pops, case.strength_const, case.Bij, case.Bji)
    alpha = np.stack([orc.line_opacity(orc.direction(th[a], ph[a]), case.lam, case.lambda0, case.c0, case.velocity,
                                       case.doppler, gamma, strength, case.alpha_cont) for a in range(nq)])
    J = orc.J_voronoi(w, th, ph, S_old, alpha, so, I0_up=case.B0[bottom], nthreads=8)
    return _epilogue(case, J, S_old, gamma)


def _regular_oracle_step(case, z, x, y, S_old, pops):
    """one pass of the loop body of test_regular_lambda._oracle_lambda from (S_old, pops)"""
    J, gamma = _oracle_J(S_old, pops, z, x, y, case, QUAD)
    return _epilogue(case, J, S_old, gamma)


def _epilogue(case, J, S_old, gamma):
    S_new = (1 - case.eps)[:, None] * J + case.eps[:, None] * case.B0
    diff = float(np.abs(1 - S_old / S_new).max())
    R = orc.calculate_R(case.lam, case.blocks, J, case.planck2, case.lambda0, case.c0, case.doppler, gamma,
                        case.sigma_bb_const, case.sigma_bf1, case.sigma_bf2, case.temperature, case.lte,
                        case.hc_over_kB, case.pref_ij, case.pref_ji)
    return J, S_new, orc.revised_populations(R, case.C, case.atom_density), diff


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _check_session_step(plain, acc, oracle_step, label):
    """the checks shared by the two sessions; returns (a, b, S after iterate 5) of the accelerated one"""
    acc.accelerate(2, 4, 4)
    S_hist = []
    for it in (1, 2, 3):
        dp, da = plain.iterate(), acc.iterate()
        gp, ga = plain.get(), acc.get()
        assert dp == da and _same(gp, ga), it        # bit for bit through iterate 3
        assert acc.last()[0] == 0 and plain.last()[0] == 0
        S_hist.append(gp[1])
    dp, da = plain.iterate(), acc.iterate()
    assert dp == da                                  # the scalar is that of the plain update
    gp4, ga4 = plain.get(), acc.get()
    S1, S2, S3, S4 = S_hist[0], S_hist[1], S_hist[2], gp4[1]
    assert plain.last()[0] == 0
    applied, sums, coeffs = acc.last()
    assert applied == 1
    ref = _reference(S4, S3, S2, S1)
    a, b = coeffs
    print(f"{label}: a = {a!r}, b = {b!r}; numpy {ref['a']!r}, {ref['b']!r}; δa {ref['da']:.3g}, δb {ref['db']:.3g}; "
          f"sums off by {np.abs(sums - ref['sums']) / ref['mags']} Σ|t|")
    assert (np.abs(sums - ref["sums"]) <= SUM_BOUND * ref["mags"]).all()
    assert abs(a - ref["a"]) <= ref["da"] and abs(b - ref["b"]) <= ref["db"]
    assert np.array([*_coefficients(sums)[:2]]).tobytes() == coeffs.tobytes()
    # the S the session holds is x_acc of the REPORTED coefficients; everything else is the plain iterate's
    assert np.array_equal(ga4[1], _apply(a, b, S4, S3, S2))
    assert not np.array_equal(ga4[1], S4)
    for k in (0, 2, 3, 4):
        assert np.array_equal(ga4[k], gp4[k]), k
    # iterate 5 against one oracle step from (x_acc, the populations after iterate 4)
    d5 = acc.iterate()
    J5, S5, pops5, _, _ = acc.get()
    assert acc.last()[0] == 0
    J_ref, S_ref, pops_ref, d_ref = oracle_step(ga4[1], ga4[2])
    assert np.abs(J5 - J_ref).max() < 1e-9 * np.abs(J_ref).max() and np.abs(S5 / S_ref - 1).max() < 1e-9
    assert np.abs(pops5 / pops_ref - 1).max() < 1e-9
    assert np.isclose(d5, d_ref, rtol=1e-8, atol=0)
    return ref, a, b, S5


@pytest.mark.gpu
def test_gpu_voronoi_session_takes_an_ng_step(voro_small):
    pos, nbr, bounds = voro_small
    so = orc.make_sites(pos, nbr, bounds)
    hs, case, (plain, acc), _ = _voronoi_sessions(voro_small, 2)
    try:
        _check_session_step(plain, acc, lambda S, pops: _voronoi_oracle_step(case, so, S, pops), "voronoi")
        # the next step is due after iterate 8, from iterates 5..8 of the accelerated session itself
        S_acc = [acc.get()[1]]
        for it in (6, 7, 8):
            acc.iterate()
            assert (acc.last()[0] != 0) == (it == 8)
            if it < 8:
                S_acc.append(acc.get()[1])
        applied, sums, coeffs = acc.last()
        assert np.array([*_coefficients(sums)[:2]]).tobytes() == coeffs.tobytes()
        if applied == 1:                             # S is an extrapolation again: not the plain update of S_acc[-1]
            assert (acc.get()[1] > 0).all()
    finally:
        plain.close()
        acc.close()
        hs.close()


@pytest.mark.gpu
def test_gpu_voronoi_session_layouts_agree(voro_small, monkeypatch):
    """VRT_LAMBDA_NATIVE = 1 (S in two sweep-order copies, 33 wavelengths: a padding wavelength in the planes) and = 0 (one
    copy in the caller's layout): the same step within the bounds of the sums"""
    pos, nbr, bounds = voro_small
    results = {}
    for native in ("1", "0"):
        monkeypatch.setenv("VRT_LAMBDA_NATIVE", native)              # read when the plan is made
        hs, case, (plain, acc), _ = _voronoi_sessions(voro_small, 2)
        try:
            acc.accelerate(2, 4, 4)
            S_hist = []
            for it in range(4):
                plain.iterate(), acc.iterate()
                S_hist.append(plain.get()[1])
            applied, sums, coeffs = acc.last()
            acc.iterate()
            results[native] = (applied, coeffs, acc.get()[1], _reference(*S_hist[::-1], result=False))
        finally:
            plain.close()
            acc.close()
            hs.close()
    (ap1, c1, S1, ref1), (ap0, c0, S0, ref0) = results["1"], results["0"]
    assert ap1 == ap0 == 1
    for c, ref in ((c1, ref1), (c0, ref0)):
        assert abs(c[0] - ref["a"]) <= ref["da"] and abs(c[1] - ref["b"]) <= ref["db"]
    assert abs(c1[0] - c0[0]) <= ref1["da"] + ref0["da"] and abs(c1[1] - c0[1]) <= ref1["db"] + ref0["db"]
    print(f"native a, b = {c1}, caller layout {c0}; S after iterate 5 differs by {np.abs(S1 / S0 - 1).max():.3g}")
    assert np.abs(S1 / S0 - 1).max() < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["voronoi", "regular"])
def test_gpu_session_with_acceleration_switched_off_again_is_the_plain_session(kind, voro_small, raster):
    if kind == "voronoi":
        hs, case, (plain, acc), _ = _voronoi_sessions(voro_small, 2)
        closer = hs.close
    else:
        solver, case, (plain, acc), _ = _regular_sessions(raster, 2)
        closer = solver.close
    try:
        acc.accelerate(2, 4, 4)
        for it in range(1, 9):
            dp, da = plain.iterate(), acc.iterate()
            if it == 2:
                acc.accelerate(0, 0, 0)
            assert dp == da and _same(plain.get(), acc.get()), it
            assert acc.last()[0] == 0
    finally:
        plain.close()
        acc.close()
        closer()


@pytest.fixture(scope="module")
def raster():
    z, x, y, kw = synth.regular_line_case(16, 10, 9, seed=7)
    return z, x, y, vrt.LineCase(**kw)


def _regular_sessions(raster, count):
    z, x, y, case = raster
    w, k, dirs = api._regular_directions(QUAD)
    lc, keep = case.c_struct()
    n, nlam = int(keep["doppler"].size), int(keep["lam"].size)
    solver = api._regular_solver(z, x, y, n, 0)
    kd, wd = np.ascontiguousarray(k, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    create = lambda out: _lib.load().vrt_regular_lambda_create(solver._h, kd.shape[0], kd.ctypes.data_as(_lib.p_dbl),
                                                               dirs.ctypes.data_as(_lib.p_int),
                                                               wd.ctypes.data_as(_lib.p_dbl), ctypes.byref(lc), 3, out)
    # (a regular handle serves one session at a time: the sessions take turns, every call returns synchronised)
    sessions = [_Session("vrt_regular_lambda", create, n, nlam) for _ in range(count)]
    return solver, case, sessions, (lc, keep, kd, wd, dirs)


@pytest.mark.gpu
def test_gpu_regular_session_takes_an_ng_step(raster):
    z, x, y, case = raster
    solver, case, (plain, acc), _ = _regular_sessions(raster, 2)
    try:
        _check_session_step(plain, acc, lambda S, pops: _regular_oracle_step(case, z, x, y, S, pops), "regular")
    finally:
        plain.close()
        acc.close()
        solver.close()


@pytest.mark.gpu
def test_gpu_regular_session_takes_an_ng_step_on_a_raster_of_odd_size():
    """5 x 5 x 5 ghosted points x 3 wavelengths (synth.three_wavelength_line_case): n nλ = 375 is odd, so the range the step
    works on ends in a tail entry behind the dense pairs (the 16 x 12 x 11 x 33 raster above has an even count)"""
    z, x, y, kw = synth.three_wavelength_line_case(5, 3, 3, seed=7)
    solver, case, (plain, acc), _ = _regular_sessions((z, x, y, vrt.LineCase(**kw)), 2)
    try:
        assert (plain.n, plain.nlam) == (125, 3)
        _check_session_step(plain, acc, lambda S, pops: _regular_oracle_step(case, z, x, y, S, pops), "regular, odd")
    finally:
        plain.close()
        acc.close()
        solver.close()


# ---- 7: it pays -----------------------------------------------------------------------------------------------------------------
def _pays(plain, fast):
    J0, S0, p0, h0 = plain
    J1, S1, p1, h1, steps = fast
    delta, rho = h0[-1], h0[-1] / h0[-2]
    bound = 2 * delta / (1 - rho)
    diff = np.abs(S1 / S0 - 1).max()
    print(f"plain {len(h0)} iterates, accelerated {len(h1)}; steps {steps}; δ {delta:.3g}, ρ {rho:.4f}: "
          f"|S_ng / S_plain - 1| = {diff:.3g} against {bound:.3g}")
    assert h0[-1] <= 1e-4 and h1[-1] <= 1e-4
    assert len(h1) < len(h0)
    assert steps and all(applied for _, applied, _, _ in steps)             # no rejected step
    assert [it for it, *_ in steps] == list(range(4, len(h1) + 1, 4))
    assert 0 < rho < 1 and diff <= bound


@pytest.mark.gpu
def test_gpu_lambda_voronoi_host_converges_in_fewer_iterates_with_ng(voro_small):
    pos, nbr, bounds = voro_small
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    case = _lambda_case(pos, bounds, 11)
    try:
        plain = vrt.Lambda_voronoi_host(1e-4, 400, hs, case, QUAD, ng=None)
        assert len(plain) == 4
        _pays(plain, vrt.Lambda_voronoi_host(1e-4, 400, hs, case, QUAD, ng=(4, 4)))
    finally:
        hs.close()


@pytest.mark.gpu
def test_gpu_lambda_regular_ng_keyword(raster):
    """ng=None: today's tuple; ng=(4, 4): a fifth element listing the due steps, S that of the session"""
    z, x, y, case = raster
    assert len(vrt.Lambda_regular(0.0, 2, z, x, y, case, QUAD)) == 4
    J, S, pops, hist, steps = vrt.Lambda_regular(0.0, 5, z, x, y, case, QUAD, ng=(4, 4))
    assert len(hist) == 5 and len(steps) == 1 and steps[0][0] == 4 and steps[0][1] is True
    solver, case, (acc,), _ = _regular_sessions(raster, 1)
    try:
        acc.accelerate(2, 4, 4)
        ds = [acc.iterate() for _ in range(5)]
        assert ds == hist and np.array_equal(acc.get()[1], S)
    finally:
        acc.close()
        solver.close()
    with pytest.raises(_lib.VrtError):
        vrt.Lambda_regular(0.0, 2, z, x, y, case, QUAD, ng=(3, 4))
