"""Emergent spectra on the GPU (vrt_synth_opacity*, vrt_regular_emergent_dev / vrt_top_intensity, vrt_tau_unity*,
api.emergent_spectrum) against the oracle and numpy restatements of plotter, write_top_intensity and write_tau_unity
(src/plot_utils.jl:101-140, :297-355, :434-576)."""

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import synth

pytestmark = pytest.mark.gpu

DIRS = [(180.0, 0.0), (0.0, 0.0), (130.0, 35.0), (95.0, 30.0), (95.0, 75.0)]


def _rel(a, b):
    return float(np.max(np.abs(a / b - 1.0)))


def _wrap_pad(a):
    """periodic_borders (src/atmosphere.jl:191-214) of (..., ny, nx, nz) arrays"""
    pad = [(0, 0)] * (a.ndim - 3) + [(1, 1), (1, 1), (0, 0)]
    return np.pad(a, pad, mode="wrap")


@pytest.fixture(scope="module")
def small():
    atm = synth.atmosphere_raster(40, 12, 7, seed=3)
    raster, pops, case, src = synth.line_raster(atm, 7, seed=3)
    return raster, pops, case, src


def _plotter(k, raster, pops, case, src, g_ratio=4.0):
    """plotter (src/plot_utils.jl:297-355) in numpy with the oracle's α_line; interior (nlam, ny, nx, nz)"""
    shape = raster["temperature"].shape
    n = raster["temperature"].size
    flat = {k_: np.asarray(raster[k_]).reshape(-1) for k_ in ("doppler", "gamma_static", "gamma_unsold", "temperature",
                                                              "alpha_cont")}
    vel = np.asarray(raster["velocity"]).reshape(3, n).T.copy()
    n1, n2 = pops[0].reshape(-1), pops[1].reshape(-1)
    gamma, strength = orc.line_terms(flat["gamma_static"], flat["gamma_unsold"], np.stack([n1, n2, np.zeros(n)]),
                                     case.strength_const, case.Bij, case.Bji)
    a_l = orc.line_opacity(k, case.lam, case.lambda0, case.c0, vel, flat["doppler"], gamma, strength, np.zeros(n)).T
    a_c = flat["alpha_cont"][None, :]
    S_l = src / (g_ratio * n1 / n2 - 1.0)
    S_c = case.planck2[:, None] / (np.exp(case.hc_over_kB / (case.lam[:, None] * flat["temperature"][None, :])) - 1.0)
    S = (a_l * S_l[None, :] + a_c * S_c) / (a_l + a_c)
    A_ref = orc.line_opacity(k, case.lam, case.lambda0, case.c0, vel, flat["doppler"], gamma, strength,
                             flat["alpha_cont"]).T
    nl = case.lam.size
    return S.reshape((nl,) + shape), A_ref.reshape((nl,) + shape)


# ---- 1. raster opacity and source function -----------------------------------------------------------------------------
@pytest.mark.parametrize("th,ph", DIRS)
def test_opacity_matches_oracle_and_plotter(small, th, ph):
    raster, pops, case, src = small
    k = vrt.direction(th, ph)
    S, A = vrt.synth_opacity(k, raster, pops, case, src)
    nl, (ny, nx, nz) = case.lam.size, raster["temperature"].shape
    assert S.shape == A.shape == (nl, ny + 2, nx + 2, nz)
    S_ref, A_ref = _plotter(k, raster, pops, case, src)
    assert _rel(A[:, 1:-1, 1:-1], A_ref) < 1e-12
    assert _rel(S[:, 1:-1, 1:-1], S_ref) < 1e-12
    # ghost columns and corners: their wrapped interior values, bit for bit
    assert np.array_equal(A, _wrap_pad(A[:, 1:-1, 1:-1]))
    assert np.array_equal(S, _wrap_pad(S[:, 1:-1, 1:-1]))
    # the line matters: line centre well above the continuum
    assert (A[nl // 2, 1:-1, 1:-1] / raster["alpha_cont"]).max() > 10


def test_opacity_dev_chunks_equal_host(small):
    import torch
    raster, pops, case, src = small
    k = vrt.direction(130.0, 35.0)
    S, A = vrt.synth_opacity(k, raster, pops, case, src)
    ny, nx, nz = raster["temperature"].shape
    dev = torch.device("cuda", 0)
    d = {n: torch.from_numpy(np.ascontiguousarray(raster[n], dtype=np.float64)).to(dev) for n in vrt.api.SYNTH_FIELDS}
    dp = torch.from_numpy(np.ascontiguousarray(pops)).to(dev)
    nl = case.lam.size
    dS = torch.zeros((nl, ny + 2, nx + 2, nz), dtype=torch.float64, device=dev)
    dA = torch.zeros_like(dS)
    ptr = {n: t.data_ptr() for n, t in d.items()}
    for l0 in range(0, nl, 3):                       # wavelength slices
        l1 = min(nl, l0 + 3)
        vrt.synth_opacity_dev(k, nz, nx, ny, case, src, ptr, dp.data_ptr(), dS[l0].data_ptr(), dA[l0].data_ptr(),
                              lam=case.lam[l0:l1], planck2=case.planck2[l0:l1])
    torch.cuda.synchronize()
    assert np.array_equal(dS.cpu().numpy(), S) and np.array_equal(dA.cpu().numpy(), A)


# ---- 2. emergent intensity, top plane only ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields(small):
    raster, pops, case, src = small
    out = {}
    for th, ph in DIRS:
        k = vrt.direction(th, ph)
        out[(th, ph)] = (k,) + vrt.synth_opacity(k, raster, pops, case, src)
    return out


@pytest.mark.parametrize("th,ph", [(180.0, 0.0), (95.0, 30.0), (95.0, 75.0), (130.0, 35.0)])
def test_top_intensity_matches_oracle(small, fields, th, ph):
    raster, _, case, _ = small
    z, x, y = raster["z"], raster["x"], raster["y"]
    xg, yg = vrt.periodic_axis(x), vrt.periodic_axis(y)
    k, S, A = fields[(th, ph)]
    I_top = vrt.top_intensity(k, S, A, z, x, y)
    assert I_top.shape == (case.lam.size, y.size, x.size)
    kinds = set()
    for l in range(case.lam.size):
        I, kd = orc.short_characteristics_up(k, S[l], S[l][:, :, 0], A[l], z, xg, yg, return_planes=True)
        kinds |= set(kd[1:].tolist())
        assert _rel(I_top[l], I[1:-1, 1:-1, -1]) < 1e-12
    if th == 95.0:
        assert kinds >= {1, 2 if ph == 30.0 else 3}   # reaches the yz / xz plane kinds (row march)
    if th == 180.0:
        assert kinds == {1}                          # all xy: the split path


@pytest.mark.parametrize("xy", ["1", "0"])
@pytest.mark.parametrize("th,ph", [(180.0, 0.0), (95.0, 30.0), (95.0, 75.0)])
def test_top_intensity_bitwise_equals_execute(small, fields, monkeypatch, xy, th, ph):
    """the top interior plane of vrt_regular_execute_dev on the same inputs, on the split xy path and the single
    kernel, and the same for chunks of 1, 3 and all wavelengths"""
    raster, _, case, _ = small
    monkeypatch.setenv("VRT_REG_XY", xy)
    z, x, y = raster["z"], raster["x"], raster["y"]
    xg, yg = vrt.periodic_axis(x), vrt.periodic_axis(y)
    k, S, A = fields[(th, ph)]
    nl = case.lam.size
    I = vrt.short_characteristics_batch(np.tile(k, (nl, 1)), [True] * nl, S, S[..., 0], A, z, xg, yg)
    ref = I[:, 1:-1, 1:-1, -1]
    vol, plane = S[0].size, xg.size * yg.size
    per_solve = 8 * (6 * vol + 6 * plane)
    for c in (1, 3, nl):
        monkeypatch.setenv("VRT_REG_EMERGENT_BYTES", str(per_solve * c))
        assert np.array_equal(vrt.top_intensity(k, S, A, z, x, y), ref), c


def test_top_intensity_dev_on_a_handle(small, fields):
    import torch
    raster, _, case, _ = small
    z, x, y = raster["z"], raster["x"], raster["y"]
    k, S, A = fields[(95.0, 75.0)]
    ref = vrt.top_intensity(k, S, A, z, x, y)
    dev = torch.device("cuda", 0)
    dS, dA = torch.from_numpy(S).to(dev), torch.from_numpy(A).to(dev)
    out = torch.zeros(ref.shape, dtype=torch.float64, device=dev)
    solver = vrt.RegularSolver(z, vrt.periodic_axis(x), vrt.periodic_axis(y))
    vrt.top_intensity_dev(solver, k, S.shape[0], dS.data_ptr(), dA.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    solver.close()
    assert np.array_equal(out.cpu().numpy(), ref)


# ---- 3. τ = 1 heights ------------------------------------------------------------------------------------------------
def _tau_vertical(A, z):
    """write_tau_unity(DATA) (src/plot_utils.jl:434-490): A interior (nlam, ny, nx, nz)"""
    zc = z[::-1]
    Y = A[..., ::-1]
    tau = np.zeros(Y.shape)
    for i in range(1, zc.size):
        tau[..., i] = tau[..., i - 1] + 0.5 * abs(zc[i] - zc[i - 1]) * (Y[..., i] + Y[..., i - 1])
    return zc[np.argmin(np.abs(tau - 1.0), axis=-1)]


def _tau_inclined(A, z, x, y, k):
    """the corrected geometry: plane iz at (x[ix] + s k_x, y[iy] + s k_y), s = (z_top - z[iz])/|k_z|, periodic
    bilinear alpha, trapezoid over the path.  Returns (heights, tau (nlam, ny, nx, nz) from the top down)."""
    nl, ny, nx, nz = A.shape
    dx, dy = (x[-1] - x[0]) / (nx - 1), (y[-1] - y[0]) / (ny - 1)
    X, Y = np.meshgrid(x, y)                                     # (ny, nx)
    tau = np.zeros(A.shape)
    prev = A[..., nz - 1]
    for j, iz in enumerate(range(nz - 2, -1, -1), start=1):
        s = (z[-1] - z[iz]) / abs(k[0])
        u = (X + s * k[1] - x[0]) / dx
        v = (Y + s * k[2] - y[0]) / dy
        i0, j0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        tx, ty = u - i0, v - j0
        i0, j0 = i0 % nx, j0 % ny
        i1, j1 = (i0 + 1) % nx, (j0 + 1) % ny
        P = A[..., iz]
        a = ((1 - ty) * ((1 - tx) * P[:, j0, i0] + tx * P[:, j0, i1]) + ty * ((1 - tx) * P[:, j1, i0] + tx * P[:, j1, i1]))
        r = abs((z[iz + 1] - z[iz]) / k[0])
        tau[..., j] = tau[..., j - 1] + 0.5 * r * (a + prev)
        prev = a
    zc = z[::-1]
    return zc[np.argmin(np.abs(tau - 1.0), axis=-1)], tau


@pytest.mark.parametrize("kz", [-1.0, 1.0])
def test_tau_unity_vertical_is_write_tau_unity(small, fields, kz):
    raster, _, case, _ = small
    z, x, y = raster["z"], raster["x"], raster["y"]
    A = fields[(180.0, 0.0)][2]
    H = vrt.tau_unity(np.array([kz, 0.0, 0.0]), A, z, x, y)
    ref = _tau_vertical(A[:, 1:-1, 1:-1], z)
    assert H.shape == (case.lam.size, y.size, x.size)
    assert np.array_equal(H, ref)
    assert len(np.unique(H)) >= 3                                 # the surface moves with wavelength and column


@pytest.mark.parametrize("th,ph", [(130.0, 35.0), (95.0, 30.0), (150.0, -120.0)])
def test_tau_unity_inclined_matches_corrected_geometry(small, fields, th, ph):
    raster, _, _, _ = small
    z, x, y = raster["z"], raster["x"], raster["y"]
    k, A = vrt.direction(th, ph), fields[(130.0, 35.0)][2]
    H = vrt.tau_unity(k, A, z, x, y)
    ref, tau = _tau_inclined(A[:, 1:-1, 1:-1], z, x, y, k)
    d = np.sort(np.abs(tau - 1.0), axis=-1)
    clear = (d[..., 1] - d[..., 0]) > 1e-9
    assert clear.mean() > 0.9
    assert np.array_equal(H[clear], ref[clear])
    # every column, none left out: the plane is one of the exact reference's candidates (oracle/synth_ref.py)
    from oracle import synth_ref
    dx, dy = (x[-1] - x[0]) / (x.size - 1), (y[-1] - y[0]) / (y.size - 1)
    cands = synth_ref.tau_candidates(*synth_ref.tau_exact(A[:, 1:-1, 1:-1], z, dx, dy, k))
    planes = np.searchsorted(z, H).ravel()
    assert np.array_equal(z[planes], H.ravel())
    assert all(int(p) in c for p, c in zip(planes, cands))


def test_tau_unity_uniform_alpha_is_vertical_of_alpha_over_mu(small):
    raster, _, _, _ = small
    z, x, y = raster["z"], raster["x"], raster["y"]
    prof = 30.0 / (z[-1] - z[0]) * np.exp(-(z - z[0]) / (0.15 * (z[-1] - z[0])))
    A = np.broadcast_to(prof * np.array([0.3, 1.0, 4.0])[:, None, None, None], (3, y.size + 2, x.size + 2, z.size)).copy()
    k = vrt.direction(130.0, 35.0)
    mu = abs(k[0])
    H = vrt.tau_unity(k, A, z, x, y)
    Hv = vrt.tau_unity(np.array([-1.0, 0.0, 0.0]), A / mu, z, x, y)
    assert np.array_equal(H, Hv)
    assert np.all(H == H[:, :1, :1])


def test_tau_unity_rolls_with_the_raster(small, fields):
    raster, _, _, _ = small
    z, x, y = raster["z"], raster["x"], raster["y"]
    k, _, A = fields[(130.0, 35.0)]
    H = vrt.tau_unity(k, A, z, x, y)
    Ar = _wrap_pad(np.roll(A[:, 1:-1, 1:-1], 1, axis=2))
    assert np.array_equal(vrt.tau_unity(k, Ar, z, x, y), np.roll(H, 1, axis=2))


def test_tau_unity_dev_equals_host(small, fields):
    import torch
    raster, _, _, _ = small
    z, x, y = raster["z"], raster["x"], raster["y"]
    k, _, A = fields[(95.0, 30.0)]
    H = vrt.tau_unity(k, A, z, x, y)
    dev = torch.device("cuda", 0)
    dA = torch.from_numpy(A).to(dev)
    out = torch.zeros(H.shape, dtype=torch.float64, device=dev)
    vrt.tau_unity_dev(k, z, x, y, A.shape[0], dA.data_ptr(), out.data_ptr())
    assert np.array_equal(out.cpu().numpy(), H)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------
def test_emergent_spectrum_end_to_end(voro_small):
    pos, nbr, bounds = voro_small
    sites = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    atm = synth.atmosphere_raster(14, 9, 8, seed=4, box_xy=1.0, z_min=0.0, z_max=2.0)
    raster, _, case, src = synth.line_raster(atm, 5, seed=4)
    rng = np.random.default_rng(7)
    n1 = 1e17 * 10.0 ** (-2.5 * pos[:, 0]) * (1.0 + 0.1 * rng.random(pos.shape[0]))
    pops = np.stack([n1, n1 * 1e-3 * (1.0 + rng.random(pos.shape[0])), n1 * 1e-2], axis=1)       # (n, 3)
    th, ph = 130.0, 35.0
    I_top, H = vrt.emergent_spectrum(sites, pops, raster, case, th, ph, src_const=src, tau=True, chunk=2)
    z, x, y = raster["z"], raster["x"], raster["y"]
    assert I_top.shape == H.shape == (case.lam.size, y.size, x.size)
    # host composition: Voronoi_to_Raster_inv_dist -> numpy plotter -> oracle solve
    P = vrt.Voronoi_to_Raster_inv_dist(sites, pops[:, :2], z, x, y)
    k = vrt.direction(th, ph)
    S_ref, A_ref = _plotter(k, raster, P, case, src)
    S_g, A_g = _wrap_pad(S_ref), _wrap_pad(A_ref)
    xg, yg = vrt.periodic_axis(x), vrt.periodic_axis(y)
    for l in range(case.lam.size):
        I = orc.short_characteristics_up(k, S_g[l], S_g[l][:, :, 0], A_g[l], z, xg, yg)
        assert _rel(I_top[l], I[1:-1, 1:-1, -1]) < 1e-10
    _, A = vrt.synth_opacity(k, raster, P, case, src)
    assert np.array_equal(H, vrt.tau_unity(k, A, z, x, y))
    assert np.array_equal(I_top, vrt.emergent_spectrum(sites, pops, raster, case, th, ph, src_const=src))
    sites.close()
