"""The continuum scattering Λ-iteration on the device (src/lambda_continuum.jl): vrt_continuum_*, vrt_regular_continuum_*,
vrt_continuum_update_dev and api.Lambda_continuum / api.Lambda_continuum_regular / api.continuum_update_dev, against the
same loop driven by the oracle (tests/test_continuum_host.py: orc.J_voronoi, orc.short_characteristics_up/down) on the
synthetic cases of synth.continuum_case / synth.regular_continuum_case.

Tolerances against the oracle loop are those of the line twins (tests/test_physics.py,
tests/test_regular_lambda.py::test_gpu_lambda_regular_matches_oracle_loop): J to 1e-9 of its maximum, S to 1e-9
relative, the history to rtol 1e-8."""
import ctypes

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import _lib, api, synth
from test_continuum_host import QUAD, bcc_case, oracle_J_regular, oracle_J_voronoi, oracle_loop, raster_case
from test_regular_lambda import MIXED, STEEP

pytestmark = pytest.mark.gpu


class _Session:
    """vrt_continuum_* / vrt_regular_continuum_* called directly"""

    def __init__(self, prefix, create, case):
        self.L, self.prefix, self.case = _lib.load(), prefix, case
        self.h = ctypes.c_void_p()
        self.rc = create(ctypes.byref(self.h))

    def fn(self, name):
        return getattr(self.L, self.prefix + name)

    def iterate(self):
        d = ctypes.c_double()
        assert self.fn("iterate")(self.h, ctypes.byref(d)) == 0
        return d.value

    def get(self):
        J, S = np.zeros((self.case.n, self.case.nlam)), np.zeros((self.case.n, self.case.nlam))
        assert self.fn("get")(self.h, J.ctypes.data_as(_lib.p_dbl), S.ctypes.data_as(_lib.p_dbl)) == 0
        return J, S

    def set_source(self, S):
        S = np.ascontiguousarray(S, dtype=np.float64)
        return self.fn("set_source")(self.h, S.ctypes.data_as(_lib.p_dbl))

    def close(self):
        if self.h:
            self.fn("destroy")(self.h)
            self.h = ctypes.c_void_p()


def _voronoi_session(sites, case, quadrature=QUAD):
    plan, w = api._quadrature_plan(sites, quadrature, 3)
    cc = case.c_struct()
    w = np.ascontiguousarray(w, dtype=np.float64)
    s = _Session("vrt_continuum_", lambda out: _lib.load().vrt_continuum_create(plan._h, ctypes.byref(cc),
                                                                               w.ctypes.data_as(_lib.p_dbl), out), case)
    s.keep = (cc, w, plan)
    return s


@pytest.fixture(scope="module")
def bcc():
    """grid, oracle sites and the 8-iterate oracle loops per wavelength count, computed once"""
    pos, nbr, bounds, _ = bcc_case(1)
    return {"pos": pos, "nbr": nbr, "bounds": bounds, "sites": vrt.VoronoiSites(pos, nbr, bounds),
            "so": orc.make_sites(pos, nbr, bounds), "cases": {}, "loops": {}}


def _bcc_case(bcc, nlam):
    if nlam not in bcc["cases"]:
        bcc["cases"][nlam] = vrt.ContinuumCase(**synth.continuum_case(bcc["pos"], bcc["bounds"], nlam, 11))
    return bcc["cases"][nlam]


def _bcc_loop(bcc, nlam):
    if nlam not in bcc["loops"]:
        case = _bcc_case(bcc, nlam)
        bcc["loops"][nlam] = oracle_loop(case, lambda S: oracle_J_voronoi(case, bcc["so"], S), 8)
    return bcc["loops"][nlam]


@pytest.fixture(scope="module")
def voro(voro_small):
    pos, nbr, bounds = voro_small
    case = vrt.ContinuumCase(**synth.continuum_case(pos, bounds, 2, 3))
    return {"sites": vrt.VoronoiSites(pos, nbr, bounds), "so": orc.make_sites(pos, nbr, bounds), "case": case}


@pytest.fixture(scope="module")
def raster():
    return raster_case(2)


def _quad(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _against_oracle(got, ref):
    J, S, hist = got[:3]
    J_ref, S_ref, hist_ref, _ = ref
    assert len(hist) == len(hist_ref)
    assert np.abs(J - J_ref).max() < 1e-9 * np.abs(J_ref).max()
    assert np.abs(S / S_ref - 1).max() < 1e-9
    assert np.allclose(hist, hist_ref, rtol=1e-8)


# ---- 1: the Voronoi session against the oracle-driven loop -----------------------------------------------------------------
@pytest.mark.parametrize("nlam", [1, 2, 3, 5])
def test_gpu_continuum_session_matches_oracle_loop(bcc, nlam):
    """one half pair; one full pair; two pairs (the data-flag chain form); three pairs"""
    case = _bcc_case(bcc, nlam)
    got = vrt.Lambda_continuum(0.0, 8, bcc["sites"], case, QUAD)
    _against_oracle(got, _bcc_loop(bcc, nlam))
    # the loop condition is the reference's: diff > ϵ && i < maxiter
    hist = got[2]
    eps = hist[4] * 1.0001
    assert len(vrt.Lambda_continuum(eps, 8, bcc["sites"], case, QUAD)[2]) == next(i for i, h in enumerate(hist) if h <= eps) + 1
    J0, S0, h0 = vrt.Lambda_continuum(1.0, 8, bcc["sites"], case, QUAD)
    assert h0 == [] and np.array_equal(S0, case.B0) and not J0.any()          # J zeros before the first iterate


def test_gpu_continuum_session_matches_oracle_loop_on_a_true_voronoi_grid(voro):
    case = voro["case"]
    got = vrt.Lambda_continuum(0.0, 8, voro["sites"], case, QUAD)
    _against_oracle(got, oracle_loop(case, lambda S: oracle_J_voronoi(case, voro["so"], S), 8))


# ---- 2: bit for bit across the paths -------------------------------------------------------------------------------------------
def _pieces_loop(sites, case, iters):
    """the loop written from the pieces: vrt_plan_execute_dev + vrt_continuum_update_dev on torch tensors"""
    import torch
    dev = torch.device("cuda", sites.device)
    plan, w = api._quadrature_plan(sites, QUAD, 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, eps, alpha = t(case.B0), t(case.eps), t(case.alpha)
    S_new, S_old, J = B.clone(), torch.zeros_like(B), torch.zeros_like(B)
    n1 = int(sites.layers_up[1] - 1)
    I0 = B[torch.as_tensor(sites.perm_up[:n1] - 1, device=dev)].contiguous()
    st = torch.cuda.current_stream().cuda_stream
    hist = []
    for _ in range(iters):
        S_old.copy_(S_new)
        plan.execute_dev(case.nlam, case.nlam, S_old.data_ptr(), alpha.data_ptr(), _lib.ALPHA_SITE_LAM, w, dJ=J.data_ptr(),
                         dI0_up=I0.data_ptr(), stream=st)
        diff, n_thick = vrt.continuum_update_dev(sites, J, B, eps, S_old, S_new, case.eps_thick)
        assert n_thick == int(case.thick().sum())
        hist.append(diff)
    torch.cuda.synchronize()
    return J.cpu().numpy(), S_new.cpu().numpy(), hist


@pytest.mark.parametrize("nlam", [1, 3, 4])
def test_gpu_continuum_paths_agree_bit_for_bit(bcc, nlam):
    """the sweep-order session, the caller-layout session and the loop written from the pieces: S, J and the history"""
    case = _bcc_case(bcc, nlam)
    nat = vrt.Lambda_continuum(0.0, 5, bcc["sites"], case, QUAD)
    cal = vrt.Lambda_continuum(0.0, 5, bcc["sites"], case, QUAD, native=False)
    pcs = _pieces_loop(bcc["sites"], case, 5)
    for other in (cal, pcs):
        assert np.array_equal(nat[0], other[0]) and np.array_equal(nat[1], other[1])
        assert nat[2] == other[2]


# ---- 3: the mask -----------------------------------------------------------------------------------------------------------------
def test_gpu_continuum_mask_changes_the_scalar_and_not_S(bcc):
    case = _bcc_case(bcc, 3)
    every = vrt.ContinuumCase(case.alpha, case.eps, case.B0, eps_thick=0.0)       # ε > 0 everywhere: nothing masked
    a = vrt.Lambda_continuum(0.0, 3, bcc["sites"], case, QUAD)
    b = vrt.Lambda_continuum(0.0, 3, bcc["sites"], every, QUAD)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2][0] != b[2][0] and all(x <= y for x, y in zip(a[2], b[2]))
    ref = _bcc_loop(bcc, 3)
    assert np.allclose(b[2], ref[3][:3], rtol=1e-8) and np.allclose(a[2], ref[2][:3], rtol=1e-8)


@pytest.mark.parametrize("nlam,ld", [(3, 5), (1, 1), (4, 4)])
def test_gpu_continuum_update_on_hand_made_arrays(bcc, nlam, ld):
    """the standalone update: every entry updated, the maximum over the thick ones, their count, NaN seen only there; n nlam
    no multiple of 256 and ld > nlam among the shapes (the padding columns are neither read nor written)"""
    import torch
    sites = bcc["sites"]
    n = sites.n
    assert (n * 3) % 256 != 0
    rng = np.random.default_rng(nlam)
    J, B, S_old = (1.0 + rng.random((n, ld)) for _ in range(3))
    eps = 10.0 ** rng.uniform(-7, 0, (n, ld))
    thick = eps[:, :nlam] > 1e-4
    S_old[tuple(np.argwhere(~thick)[1])] = 100.0               # the largest term of all sits at a thin entry
    dev = torch.device("cuda", sites.device)
    t = lambda a: torch.from_numpy(a).to(dev)

    def run(B_):
        S_new = torch.full((n, ld), -7.0, dtype=torch.float64, device=dev)
        diff, cnt = vrt.continuum_update_dev(sites, t(J), t(B_), t(eps), t(S_old), S_new, 1e-4, nlam=nlam)
        return diff, cnt, S_new.cpu().numpy()

    diff, cnt, S_new = run(B)
    ref = (1 - eps) * J + eps * B
    assert np.array_equal(S_new[:, :nlam], ref[:, :nlam]) and (S_new[:, nlam:] == -7.0).all()
    rel = np.abs(1 - S_old / ref)[:, :nlam]
    assert cnt == int(thick.sum()) and 0 < cnt < n * nlam
    assert diff == rel[thick].max() and diff != rel.max()
    # a NaN at a thin entry is not seen; at a thick one it is the result
    thin_at = tuple(np.argwhere(~thick)[0])
    thick_at = tuple(np.argwhere(thick)[-1])
    for at, seen in ((thin_at, False), (thick_at, True)):
        Bn = B.copy()
        Bn[at] = np.nan
        d, c, Sn = run(Bn)
        assert np.isnan(Sn[at]) and c == cnt
        assert np.isnan(d) if seen else d == diff


def test_gpu_continuum_session_mask_of_a_single_entry(bcc):
    """the sessions' own update kernels (sweep order and caller layout): with the threshold AT the second largest ε (the
    comparison is strict) one entry is thick, and the scalar is that entry's term"""
    case = _bcc_case(bcc, 3)
    at = np.unravel_index(np.argmax(case.eps), case.eps.shape)
    second = np.sort(case.eps.ravel())[-2]
    one = vrt.ContinuumCase(case.alpha, case.eps, case.B0, eps_thick=float(second))
    ref = _bcc_loop(bcc, 3)
    J1 = oracle_J_voronoi(case, bcc["so"], case.B0)
    S1 = (1 - case.eps) * J1 + case.eps * case.B0
    want = abs(1 - case.B0[at] / S1[at])
    for native in (True, False):
        h = vrt.Lambda_continuum(0.0, 1, bcc["sites"], one, QUAD, native=native)[2]
        assert np.isclose(h[0], want, rtol=1e-8) and h[0] != ref[2][0]


# ---- 4: the boundary -------------------------------------------------------------------------------------------------------------
def test_gpu_continuum_up_solves_start_from_B0_not_S(bcc):
    case = _bcc_case(bcc, 2)
    so = bcc["so"]
    S0 = 2.0 * case.B0
    J, S, hist = vrt.Lambda_continuum(0.0, 1, bcc["sites"], case, QUAD, S0=S0)
    J_ref = oracle_J_voronoi(case, so, S0)                                         # I0_up = B0[bottom]
    assert np.abs(J - J_ref).max() < 1e-9 * np.abs(J_ref).max()
    n1 = int(so.layers_up[1] - 1)
    J_S = oracle_J_voronoi(case, so, S0, I0_up=S0[so.perm_up[:n1] - 1])            # what starting from S would give
    assert np.abs(J_S - J_ref).max() > 1e-3 * np.abs(J_ref).max()
    S_ref = (1 - case.eps) * J_ref + case.eps * case.B0
    assert np.abs(S / S_ref - 1).max() < 1e-9
    assert np.isclose(hist[0], np.abs(1 - S0 / S_ref)[case.thick()].max(), rtol=1e-8)


# ---- 5: resume ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [True, False])
def test_gpu_continuum_resumes_from_a_saved_source(bcc, native, monkeypatch):
    if not native:
        monkeypatch.setenv("VRT_LAMBDA_NATIVE", "0")                                # (read when the plan is created)
    case = _bcc_case(bcc, 3)
    sites = vrt.VoronoiSites(bcc["pos"], bcc["nbr"], bcc["bounds"])
    first, fresh = _voronoi_session(sites, case), _voronoi_session(sites, case)
    try:
        assert first.rc == 0 and fresh.rc == 0
        for _ in range(6):
            first.iterate()
        _, S6 = first.get()
        d7 = first.iterate()
        J7, S7 = first.get()
        assert fresh.set_source(S6) == 0
        assert fresh.iterate() == d7
        Jr, Sr = fresh.get()
        assert np.array_equal(Jr, J7) and np.array_equal(Sr, S7)
        # an S with a zero (or a NaN, an Inf, a negative value) is refused and nothing changes
        for bad in (0.0, -1.0, np.nan, np.inf):
            Sb = S7.copy()
            Sb[17, 1] = bad
            assert fresh.set_source(Sb) == _lib.VRT_EINVAL
            assert np.array_equal(fresh.get()[1], S7)
        assert fresh.iterate() == first.iterate()
    finally:
        first.close()
        fresh.close()
        sites.close()


# ---- 6: the regular session ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad", ["ul7n12", "mixed", "steep"])
def test_gpu_continuum_regular_matches_oracle_loop(raster, tmp_path, quad):
    z, x, y, case = raster
    q = {"ul7n12": QUAD, "mixed": _quad(tmp_path, "mixn5.dat", MIXED), "steep": _quad(tmp_path, "steepn4.dat", STEEP)}[quad]
    got = vrt.Lambda_continuum_regular(0.0, 4, z, x, y, case, q)
    _against_oracle(got, oracle_loop(case, lambda S: oracle_J_regular(case, z, x, y, S, q), 4))
    if quad == "mixed":                                # the θ = 90 angle adds nothing: the set without it gives the same bits
        rows = [ln for ln in MIXED.splitlines() if float(ln.split()[1]) != 90.0]
        got4 = vrt.Lambda_continuum_regular(0.0, 4, z, x, y, case, _quad(tmp_path, "mixn4.dat", "\n".join(rows) + "\n"))
        assert np.array_equal(got4[0], got[0]) and np.array_equal(got4[1], got[1]) and got4[2] == got[2]


def test_gpu_continuum_regular_bit_identical_under_chunking(raster, tmp_path, monkeypatch):
    """one-solve chunks (VRT_REG_LAMBDA_BYTES = 1, read when the regular handle is created: chunk boundaries inside an
    angle's wavelengths) against the default chunking; resume and the S0 keyword on the raster"""
    z, x, y, case = raster
    q = _quad(tmp_path, "mixn5.dat", MIXED)
    ref = vrt.Lambda_continuum_regular(0.0, 3, z, x, y, case, q)
    monkeypatch.setenv("VRT_REG_LAMBDA_BYTES", "1")
    one = vrt.Lambda_continuum_regular(0.0, 3, z, x, y, case, q)
    monkeypatch.delenv("VRT_REG_LAMBDA_BYTES")
    assert np.array_equal(ref[0], one[0]) and np.array_equal(ref[1], one[1]) and ref[2] == one[2]
    two = vrt.Lambda_continuum_regular(0.0, 2, z, x, y, case, q)
    third = vrt.Lambda_continuum_regular(0.0, 1, z, x, y, case, q, S0=two[1])
    assert np.array_equal(third[0], ref[0]) and np.array_equal(third[1], ref[1]) and third[2][0] == ref[2][2]
    bad = two[1].copy()
    bad[3, 0] = 0.0
    with pytest.raises(vrt.VrtError) as e:
        vrt.Lambda_continuum_regular(0.0, 1, z, x, y, case, q, S0=bad)
    assert e.value.code == _lib.VRT_EINVAL


def test_gpu_continuum_create_refuses_bad_cases(bcc, raster):
    """the array checks of create itself, on real handles (the same answers as vrt_continuum_case_check)"""
    case = _bcc_case(bcc, 2)
    eps = case.eps.copy()
    eps[3, 1] = 1.5
    alpha = case.alpha.copy()
    alpha[5, 0] = 0.0
    for bad in (vrt.ContinuumCase(case.alpha, eps, case.B0), vrt.ContinuumCase(alpha, case.eps, case.B0),
                vrt.ContinuumCase(case.alpha, case.eps, case.B0, eps_thick=1.0)):
        with pytest.raises(vrt.VrtError) as e:
            vrt.Lambda_continuum(0.0, 1, bcc["sites"], bad, QUAD)
        assert e.value.code == _lib.VRT_EINVAL
    z, x, y, rc = raster
    with pytest.raises(vrt.VrtError) as e:
        vrt.Lambda_continuum_regular(0.0, 1, z, x, y, vrt.ContinuumCase(rc.alpha, rc.eps, rc.B0, eps_thick=1.0), QUAD)
    assert e.value.code == _lib.VRT_EINVAL


# ---- 7: Ng ---------------------------------------------------------------------------------------------------------------------------
def _pays(kind, plain, fast, again, thick):
    """Both runs stop at their first iterate with masked maximum <= 1e-4.  A fixed-point iteration that contracts by ρ per
    iterate and last moved by δ is within δ ρ / (1 - ρ) < δ / (1 - ρ) of its fixed point; δ and ρ are read off the plain
    run's last two entries, as tests/test_accel.py does, and each run is allowed that distance: 2 δ / (1 - ρ), asserted
    over EVERY entry of S, thin ones included (the figure over the thick entries alone is printed beside it)."""
    J0, S0, h0 = plain
    J1, S1, h1, steps = fast
    delta, rho = h0[-1], h0[-1] / h0[-2]
    bound = 2 * delta / (1 - rho)
    diff = np.abs(S1 / S0 - 1)
    print(f"{kind}: plain {len(h0)} iterates, accelerated {len(h1)}; steps {steps}; δ {delta:.3g}, ρ {rho:.4f}: "
          f"|S_ng / S_plain - 1| = {diff.max():.3g} all, {diff[thick].max():.3g} thick, against {bound:.3g}")
    assert h0[-1] <= 1e-4 and h1[-1] <= 1e-4
    assert len(h1) <= len(h0)                                                  # Ng never costs iterates here
    assert steps and all(applied for _, applied, _, _ in steps)                # at least one step, none rejected
    assert [it for it, *_ in steps] == list(range(4, len(h1) + 1, 4))
    assert 0 < rho < 1 and diff.max() <= bound
    assert np.array_equal(again[0], J1) and np.array_equal(again[1], S1) and again[2] == h1 and again[3] == steps


def test_gpu_continuum_converges_with_ng_on_the_voronoi_grid(voro):
    case, sites = voro["case"], voro["sites"]
    plain = vrt.Lambda_continuum(1e-4, 400, sites, case, QUAD)
    fast = vrt.Lambda_continuum(1e-4, 400, sites, case, QUAD, ng=(4, 4))
    _pays("voronoi 1500 x 2", plain, fast, vrt.Lambda_continuum(1e-4, 400, sites, case, QUAD, ng=(4, 4)), case.thick())
    # the caller-layout session sums the same entries in another order: the same steps, S to rounding
    cal = vrt.Lambda_continuum(1e-4, 400, sites, case, QUAD, ng=(4, 4), native=False)
    assert len(cal[2]) == len(fast[2]) and [s[:2] for s in cal[3]] == [s[:2] for s in fast[3]]
    assert np.abs(cal[1] / fast[1] - 1).max() < 1e-9


def test_gpu_continuum_converges_with_ng_on_the_raster(raster):
    z, x, y, case = raster
    run = lambda **kw: vrt.Lambda_continuum_regular(1e-4, 400, z, x, y, case, QUAD, **kw)
    _pays("raster 16 x 12 x 11 x 2", run(), run(ng=(4, 4)), run(ng=(4, 4)), case.thick())


def test_gpu_continuum_converges_with_ng_on_a_raster_of_odd_size():
    """5 x 5 x 5 ghosted points x 3 wavelengths: n nλ = 375 is odd, so the range Ng works on ends in a tail entry behind the
    dense pairs (every other raster case here has an even count)"""
    z, x, y, kw = synth.regular_continuum_case(5, 3, 3, 7, 3)
    case = vrt.ContinuumCase(**kw)
    assert (case.n, case.nlam) == (125, 3)
    run = lambda **kw: vrt.Lambda_continuum_regular(1e-4, 400, z, x, y, case, QUAD, **kw)
    _pays("raster 5 x 5 x 5 x 3", run(), run(ng=(4, 4)), run(ng=(4, 4)), case.thick())
