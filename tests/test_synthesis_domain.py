"""The emergent-spectrum kernels at their decisions and launch seams: k_tau_unity (csrc/vrt_synth.hip) against the exact
rational reference of oracle/synth_ref.py on every column, k_synth_opacity (csrc/vrt_physics.hip) against a 40-digit
evaluation over its field domain and across its 32-wavelength launches, vrt_regular_emergent_dev (csrc/vrt_regular.hip)
through the regular solver's shape table, and api.emergent_spectrum's chunk loop.  The inputs are built and shown to
be what they claim in tests/test_synthesis_domain_host.py.  Figures are printed before they are asserted
(profiles/synthesis_domain/test_synthesis_domain_figures.txt)."""
import contextlib
import functools
import os
import time

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from oracle import synth_ref as ref
from voronoirt_amd import _lib
from test_regular import _random_problem
from test_regular_domain_host import ALL_FORMS, SHAPE_ANGLES, SHAPES, expected_launch
from test_synthesis import _plotter, _wrap_pad
from test_synthesis_domain_host import (DYADIC, NONFINITE, SEAM_NLAM, SHAPE_NLAM, SYNTH_K, SYNTH_SHAPES, dyadic_raster,
                                        in_candidates, kernel_tau, nonfinite_raster, rel_err, synth_case_hp, synth_cases,
                                        synth_problem, tau_pairs, tau_rasters, tau_reference)

pytestmark = pytest.mark.gpu
CONTRACT = 1e-12


@pytest.fixture(scope="module", autouse=True)
def _module_clock():
    """the module's wall time, first test to last, for the record (the references are computed inside it)"""
    t0 = time.time()
    yield
    print("\ntest_synthesis_domain.py: %.1f s from its first test to its last" % (time.time() - t0))


def _planes(H, z):
    """plane index of every returned height (each must be a z value, bit for bit)"""
    arg = np.searchsorted(z, H)
    assert np.array_equal(z[np.clip(arg, 0, z.size - 1)], H), "a height that is no plane's z"
    return arg


def _tau_dev(k, ra):
    import torch
    dev = torch.device("cuda", 0)
    dA = torch.from_numpy(ra.ghosted).to(dev)
    out = torch.full(ra.alpha.shape[:3], np.nan, dtype=torch.float64, device=dev)
    vrt.tau_unity_dev(k, ra.z, ra.x, ra.y, ra.alpha.shape[0], dA.data_ptr(), out.data_ptr())
    return out.cpu().numpy()


# ---- 1. tau = 1 heights ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tau_rasters()))
def test_tau_unity_returns_a_candidate_in_every_column(name):
    ra = tau_rasters()[name]
    ghosted = ra.ghosted
    n_dir = n_col = n_undecided = n_same = 0
    worst = 0.0
    for rname, label, k in tau_pairs():
        if rname != name:
            continue
        tau, B, cands = tau_reference(name, label)
        H = vrt.tau_unity(k, ghosted, ra.z, ra.x, ra.y)
        assert H.shape == ra.alpha.shape[:3]
        arg = _planes(H, ra.z)
        ok = in_candidates(arg, cands)
        arg_t, taus = kernel_tau(ra.alpha, ra.z, ra.dx, ra.dy, k)
        exact = np.array([float(t) for t in tau.ravel()]).reshape(tau.shape)
        same = np.array_equal(arg, arg_t)
        if same:                    # the same planes as the fp64 statement order: its tau is the kernel's, as far as heights show
            worst = max(worst, float(np.max(np.where(B > 0, np.abs(taus - exact) / np.where(B > 0, B, 1.0), 0.0))))
        n_dir, n_col, n_same = n_dir + 1, n_col + ok.size, n_same + int(same)
        n_undecided += sum(len(c) > 1 for c in cands)
        assert ok.all(), (name, label, np.flatnonzero(~ok)[:5])
        assert np.array_equal(_tau_dev(k, ra), H), (name, label)     # the device form: the same bits
    print("tau unity %-12s: %3d directions, %5d columns all inside their candidates, decided by the reference alone %.4f, "
          "%d directions with the planes of the fp64 statement order (worst |tau - exact| / B there %.3f)"
          % (name, n_dir, n_col, 1.0 - n_undecided / n_col, n_same, worst))
    assert n_dir >= 9


@pytest.mark.parametrize("kz", [-1.0, 1.0])
def test_tau_unity_dyadic_columns_and_ties(kz):
    ra = dyadic_raster()
    k = np.array([kz, 0.0, 0.0])
    want = ref.first_argmin(ref.tau_exact(ra.alpha, ra.z, ra.dx, ra.dy, k)[0])
    H = vrt.tau_unity(k, ra.ghosted, ra.z, ra.x, ra.y)
    got = _planes(H, ra.z)
    print("tau unity dyadic k_z %+g: planes of column (0, 0): %s" % (kz, {n: int(got[c, 0, 0]) for c, (n, _, _) in enumerate(DYADIC)}))
    for c, (case, _, plane) in enumerate(DYADIC):
        assert got[c, 0, 0] == plane, case
    assert np.array_equal(got, want)
    assert np.array_equal(_tau_dev(k, ra), H)


@pytest.mark.parametrize("kz", [-1.0, 1.0])
def test_tau_unity_nan_is_the_first_argmin_and_neighbours_are_not_read(kz):
    """write_tau_unity(DATA) at k = (+-1, 0, 0): Julia's argmin returns the first NaN, and a column is computed from its
    own values alone"""
    ra = nonfinite_raster()
    k = np.array([kz, 0.0, 0.0])
    want = ref.first_argmin(ref.tau_exact(ra.alpha, ra.z, ra.dx, ra.dy, k)[0])
    H = vrt.tau_unity(k, ra.ghosted, ra.z, ra.x, ra.y)
    got = _planes(H, ra.z)
    print("tau unity non-finite k_z %+g: centre column %s, clean %d" %
          (kz, {n: int(got[c, 1, 1]) for c, (n, _, _) in enumerate(NONFINITE)}, int(got[-1, 1, 1])))
    for c, (case, (iy, ix, iz), v) in enumerate(NONFINITE):
        if "beside" in case:
            assert H[c, 1, 1] == H[-1, 1, 1], case                   # unchanged by the neighbouring column
        assert got[c, iy, ix] == want[c, iy, ix], case
    assert got[0, 1, 1] == 3 and got[1, 1, 1] == 2 and got[2, 1, 1] == 0
    assert np.array_equal(got, want)
    assert np.array_equal(_tau_dev(k, ra), H)


# ---- 2. raster opacity and source function ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(synth_cases()))
def test_synth_opacity_field_domain(name):
    raster, pops, case, src = synth_cases()[name]
    A_hp, S_hp, K = synth_case_hp(name)
    S, A = vrt.synth_opacity(SYNTH_K, raster, pops, case, src)
    Si, Ai = S[:, 1:-1, 1:-1], A[:, 1:-1, 1:-1]
    eA, eS = rel_err(Ai, A_hp), rel_err(Si, S_hp)
    with np.errstate(all="ignore"):
        S64, A64 = _plotter(SYNTH_K, raster, pops, case, src)
    print("synth opacity %-18s: kappa <= %-8.3g worst rel. error / kappa: alpha_tot %.3e, S %.3e; plain: %.3e, %.3e; "
          "non-finite S %d" % (name, K.max(), (eA / K).max(), (eS / K).max(), eA.max(), eS.max(), int((~np.isfinite(Si)).sum())))
    for got, want in ((Ai, A64), (Si, S64)):                          # NaN and Inf exactly where the fp64 restatement has them
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(got)], want[np.isinf(want)]), name
    assert np.array_equal(np.isfinite(Si), np.isfinite(S_hp)) and np.isfinite(Ai).all() == np.isfinite(A_hp).all()
    assert np.all(eA <= CONTRACT * K), name
    assert np.all(eS <= CONTRACT * K), name
    if name == "smooth":
        assert K.max() <= 100 and eA.max() < CONTRACT and eS.max() < CONTRACT
    assert np.array_equal(A, _wrap_pad(Ai)) and np.array_equal(S, _wrap_pad(Si), equal_nan=True)


def _synth_dev_slices(problem, k, step):
    import torch
    raster, pops, case, src = problem
    ny, nx, nz = raster["temperature"].shape
    dev = torch.device("cuda", 0)
    d = {n: torch.from_numpy(np.ascontiguousarray(raster[n], dtype=np.float64)).to(dev) for n in vrt.api.SYNTH_FIELDS}
    dp = torch.from_numpy(np.ascontiguousarray(pops)).to(dev)
    nl = case.lam.size
    dS = torch.full((nl, ny + 2, nx + 2, nz), np.nan, dtype=torch.float64, device=dev)
    dA = torch.full_like(dS, np.nan)
    ptr = {n: t.data_ptr() for n, t in d.items()}
    for l0 in range(0, nl, step):
        l1 = min(nl, l0 + step)
        vrt.synth_opacity_dev(k, nz, nx, ny, case, src, ptr, dp.data_ptr(), dS[l0].data_ptr(), dA[l0].data_ptr(),
                              lam=case.lam[l0:l1], planck2=case.planck2[l0:l1])
    torch.cuda.synchronize()
    return dS.cpu().numpy(), dA.cpu().numpy()


@pytest.mark.parametrize("shape,nlam", [(s, SHAPE_NLAM[s]) for s in SYNTH_SHAPES] +
                         [(SYNTH_SHAPES[-1], n) for n in SEAM_NLAM if n != SHAPE_NLAM[SYNTH_SHAPES[-1]]])
def test_synth_opacity_ghosts_and_wavelength_seam(shape, nlam):
    """nx = 1 / ny = 1 ghosts, and the launches of 32 wavelengths: every wavelength of the one call equals the same
    wavelength computed alone and in device slices of 5 and of 40, bit for bit"""
    problem = synth_problem(shape, nlam)
    raster, pops, case, src = problem
    nz, nx, ny = shape
    S, A = vrt.synth_opacity(SYNTH_K, raster, pops, case, src)
    assert S.shape == A.shape == (nlam, ny + 2, nx + 2, nz)
    assert np.isfinite(S).all() and np.isfinite(A).all() and (A > 0).all()
    assert np.array_equal(A, _wrap_pad(A[:, 1:-1, 1:-1])) and np.array_equal(S, _wrap_pad(S[:, 1:-1, 1:-1]))
    for l in range(nlam):
        S1, A1 = vrt.synth_opacity(SYNTH_K, raster, pops, case, src, lam=case.lam[l:l + 1], planck2=case.planck2[l:l + 1])
        assert np.array_equal(S1[0], S[l]) and np.array_equal(A1[0], A[l]), (shape, nlam, l)
    for step in (5, 40):
        Sd, Ad = _synth_dev_slices(problem, SYNTH_K, step)
        assert np.array_equal(Sd, S) and np.array_equal(Ad, A), (shape, nlam, step)
    assert len({A[l].tobytes() for l in range(nlam)}) == nlam          # no two wavelengths alike: an offset error shows
    print("synth opacity seam (nz, nx, ny) = %-10s nlam %2d: one call = %d single calls = device slices of 5 and 40" % (shape, nlam, nlam))


# ---- 3. emergent intensity through the regular solver's shape table ----------------------------------------------------------
EMERGENT_NLAM = 5


@contextlib.contextmanager
def _env(**kw):
    old = {n: os.environ.get(n) for n in kw}
    os.environ.update({n: str(v) for n, v in kw.items()})
    try:
        yield
    finally:
        for n, v in old.items():
            if v is None:
                del os.environ[n]
            else:
                os.environ[n] = v


@functools.lru_cache(maxsize=None)
def _emergent_problem(shape, cls):
    """axes (x, y ghosted by periodic_axis, as top_intensity builds them), five wavelengths of random fields and the up
    directions of the class"""
    nz, nx, ny = shape
    seed = 900 + nz + 3 * nx + 7 * ny
    rng = np.random.default_rng(seed)
    z = np.cumsum(rng.uniform(0.1, 0.3, nz))
    x, y = np.arange(nx - 2) * 0.1, np.arange(ny - 2) * 0.13
    S = np.stack([_random_problem(nz, nx, ny, seed + l)[3] for l in range(EMERGENT_NLAM)])
    A = np.stack([_random_problem(nz, nx, ny, seed + l)[4] for l in range(EMERGENT_NLAM)])
    ks = [orc.direction(t, p) for t, p in SHAPE_ANGLES[cls] if t > 90]
    return z, x, y, S, A, ks


def _ghost_axis(a, d):
    return vrt.periodic_axis(a) if a.size > 1 else np.array([a[0] - d, a[0], a[0] + d])


@functools.lru_cache(maxsize=None)
def _run_emergent(shape, cls, mode):
    """[(k, form after the emergent call, max oracle difference of wavelength 0)] of one row; asserts bit equality
    with execute_dev for the chunkings"""
    import torch
    z, x, y, S, A, ks = _emergent_problem(shape, cls)
    xg, yg = _ghost_axis(x, 0.1), _ghost_axis(y, 0.13)
    nz, nx, ny = shape
    assert (xg.size, yg.size) == (nx, ny)
    dev = torch.device("cuda", 0)
    dS, dA = torch.from_numpy(S).to(dev), torch.from_numpy(A).to(dev)
    dI0 = dS[..., 0].contiguous()
    vol, plane = nz * nx * ny, nx * ny
    per_solve = 8 * (6 * vol + 6 * plane)
    nl = EMERGENT_NLAM
    out = []
    for k in ks:
        with _env(VRT_REG_XY=mode):
            solver = vrt.RegularSolver(z, xg, yg, device=0)
        dI = torch.full((nl,) + S.shape[1:], np.nan, device=dev, dtype=torch.float64)
        solver.execute_dev(np.tile(k, (nl, 1)), [True] * nl, dS.data_ptr(), vol, dA.data_ptr(), vol, dI0.data_ptr(),
                           dI.data_ptr(), 3, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        form_exec = solver.last_launch_form()
        solver.close()
        want = dI.cpu().numpy()[:, 1:-1, 1:-1, -1]
        forms = []
        for c in (1, 2, nl):
            with _env(VRT_REG_XY=mode, VRT_REG_EMERGENT_BYTES=per_solve * c):
                solver = vrt.RegularSolver(z, xg, yg, device=0)
            top = torch.full((nl, ny - 2, nx - 2), np.nan, device=dev, dtype=torch.float64)
            vrt.top_intensity_dev(solver, k, nl, dS.data_ptr(), dA.data_ptr(), top.data_ptr())
            torch.cuda.synchronize()
            forms.append(solver.last_launch_form())
            solver.close()
            assert np.array_equal(top.cpu().numpy(), want), (shape, cls, mode, c)
        assert forms[0] == forms[1] == forms[2] == form_exec, (shape, cls, mode, forms, form_exec)
        out.append((k, forms[0], want))
    return out


ROWS = sorted({(s, c, m) for s, c, m, _ in SHAPES})


@pytest.mark.parametrize("row", ROWS, ids=["%dx%dx%d-%s-xy%s" % (r[0] + (r[1], r[2])) for r in ROWS])
def test_top_intensity_equals_execute_over_the_shape_table(row):
    """top_intensity_dev under chunks of 1, 2 and all 5 wavelengths (an uneven last chunk) against the top interior
    plane of execute_dev, bit for bit; the launch form is the shape table's (it does not depend on the number of solves
    below 128: the doubling rule's 256 Ki thread cap is far away)"""
    shape, cls, mode = row
    res = _run_emergent(shape, cls, mode)
    assert len(res) >= 2
    for k, form, _ in res:
        print("emergent %-14s %-5s VRT_REG_XY=%s k = (%+.3f, %+.3f, %+.3f): form %-16s threads %4d %s"
              % (shape, cls, mode, k[0], k[1], k[2], form[0], form[1], form[2] or ""))
        assert form == expected_launch(shape, cls, mode), (shape, cls, mode)


@pytest.mark.parametrize("shape,cls", sorted({(s, c) for s, c, m, _ in SHAPES if m == "1"}))
def test_top_intensity_against_the_oracle_and_host_form(shape, cls):
    """wavelength 0 of one direction per raster against short_characteristics_up at the solver's 1e-12, and the host
    form (which builds the ghosted axes itself) equal to the device form"""
    z, x, y, S, A, ks = _emergent_problem(shape, cls)
    k, _, got = _run_emergent(shape, cls, "1")[0]
    xg, yg = _ghost_axis(x, 0.1), _ghost_axis(y, 0.13)
    I = orc.short_characteristics_up(k, S[0], S[0][:, :, 0].copy(), A[0], z, xg, yg)
    want = I[1:-1, 1:-1, -1]
    d = np.abs(got[0] - want).max() / np.abs(want).max()
    print("emergent %-14s %-5s wavelength 0 against the oracle: max|gpu - oracle| / max|oracle| %.3e" % (shape, cls, d))
    assert d < CONTRACT
    if x.size > 1 and y.size > 1:
        assert np.array_equal(vrt.top_intensity(k, S, A, z, x, y), got)


def test_emergent_entry_reaches_every_launch_form():
    """vrt_regular_emergent_dev goes through regular_solve as vrt_regular_execute_dev does, so no form is out of its
    reach: UNREACHABLE is empty, and a form may enter it only with the reason."""
    UNREACHABLE = {}
    seen = {form[0] for row in ROWS for _, form, _ in _run_emergent(*row)}
    print("emergent entry: forms reached %s; cannot be reached: %s" % (sorted(seen), UNREACHABLE or "none"))
    assert seen == ALL_FORMS - set(UNREACHABLE) == set(_lib.REG_FORMS)
    assert any(s == (2, 3, 3) for s, _, _ in ROWS)                   # the 1 x 1 interior ran


# ---- 4. the chunk loop of emergent_spectrum -----------------------------------------------------------------------------------
def test_emergent_spectrum_chunks_and_composition(voro_small):
    from voronoirt_amd import synth
    pos, nbr, bounds = voro_small
    sites = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    atm = synth.atmosphere_raster(14, 9, 8, seed=4, box_xy=1.0, z_min=0.0, z_max=2.0)
    raster, _, case, src = synth.line_raster(atm, 33, seed=4)
    rng = np.random.default_rng(7)
    n1 = 1e17 * 10.0 ** (-2.5 * pos[:, 0]) * (1.0 + 0.1 * rng.random(pos.shape[0]))
    pops = np.stack([n1, n1 * 1e-3 * (1.0 + rng.random(pos.shape[0])), n1 * 1e-2], axis=1)
    th, ph = 130.0, 35.0
    res = {c: vrt.emergent_spectrum(sites, pops, raster, case, th, ph, src_const=src, tau=True, chunk=c) for c in (0, 32, 5, 1)}
    I_top, H = res[0]
    z, x, y = raster["z"], raster["x"], raster["y"]
    assert I_top.shape == H.shape == (33, y.size, x.size)
    for c in (32, 5, 1):
        assert np.array_equal(res[c][0], I_top) and np.array_equal(res[c][1], H), c
    P = vrt.Voronoi_to_Raster_inv_dist(sites, pops[:, :2], z, x, y)
    k = vrt.direction(th, ph)
    S_ref, A_ref = _plotter(k, raster, P, case, src)
    S_g, A_g = _wrap_pad(S_ref), _wrap_pad(A_ref)
    xg, yg = vrt.periodic_axis(x), vrt.periodic_axis(y)
    worst = 0.0
    for l in range(case.lam.size):
        I = orc.short_characteristics_up(k, S_g[l], S_g[l][:, :, 0], A_g[l], z, xg, yg)
        worst = max(worst, float(np.max(np.abs(I_top[l] / I[1:-1, 1:-1, -1] - 1.0))))
    print("emergent spectrum, 33 wavelengths: chunks 0, 32, 5, 1 the same bits; worst |I_top / composition - 1| %.3e" % worst)
    assert worst < 1e-10
    S, A = vrt.synth_opacity(k, raster, P, case, src)
    assert np.array_equal(H, vrt.tau_unity(k, A, z, x, y))
    assert np.array_equal(I_top, vrt.top_intensity(k, S, A, z, x, y))
    assert len(np.unique(H)) >= 3
    sites.close()
