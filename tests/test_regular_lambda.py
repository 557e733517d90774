"""The line Λ-iteration on the regular grid (J_λ_regular, Λ_regular: src/lambda_iteration.jl:1-58, :116-205) on the
device -- vrt_regular_execute_line, vrt_regular_lambda_* and api.J_lambda_regular_line / api.Lambda_regular -- against
the same loop driven by the oracle: orc.line_terms, orc.line_opacity per angle, orc.short_characteristics_up/down per
(angle, wavelength), orc.calculate_R and orc.revised_populations, on a small raster with its periodic ghost border."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrt_regular_execute_line", "vrt_regular_lambda_create", "vrt_regular_lambda_iterate", "vrt_regular_lambda_get",
       "vrt_regular_lambda_destroy")

# ul7n12 with a θ = 90 entry (adds nothing) among ups and downs; steep rays only (every plane of the xy kind)
MIXED = ("0.062174023651822  70.292581108446825 346.412955051617416\n"
         "0.078304613457687 152.666292044518485 315.475247829748128\n"
         "0.050000000000000  90.000000000000000  30.000000000000000\n"
         "0.090740740740741 112.824260481870382 335.790538127899197\n"
         "0.084923207761833  78.189290607965106  55.428463450411122\n")
STEEP = ("0.25 170.0 30.0\n"
         "0.25 155.0 200.0\n"
         "0.25 10.0 120.0\n"
         "0.25 25.0 300.0\n")


@pytest.fixture(scope="module")
def raster():
    z, x, y, kw = synth.regular_line_case(16, 10, 9, seed=7)
    return z, x, y, vrt.LineCase(**kw)


def _quad(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _oracle_J(S, pops, z, x, y, case, quadrature, n_sweeps=3, I0_up=None):
    """J_λ_regular's line method (src/lambda_iteration.jl:1-58) with the oracle's restatements; S (n, nλ); I0_up
    (nλ, ny, nx) numpy, default B_0's bottom plane (:38)"""
    w, th, ph, nq = vrt.read_quadrature(quadrature)
    nz, nx, ny = z.size, x.size, y.size
    gamma, strength = orc.line_terms(case.gamma_static, case.gamma_unsold, pops, case.strength_const, case.Bij, case.Bji)
    J = np.zeros_like(S)
    B0 = np.asarray(case.B0)
    for a in range(nq):
        if th[a] == 90:
            continue
        k = orc.direction(th[a], ph[a])
        alpha = orc.line_opacity(k, case.lam, case.lambda0, case.c0, case.velocity, case.doppler, gamma, strength,
                                 case.alpha_cont)
        for l in range(S.shape[1]):
            S_l, a_l = S[:, l].reshape(ny, nx, nz), alpha[:, l].reshape(ny, nx, nz)
            if th[a] > 90:
                I0 = B0[:, l].reshape(ny, nx, nz)[:, :, 0] if I0_up is None else I0_up[l]
                I = orc.short_characteristics_up(k, S_l, I0, a_l, z, x, y, n_sweeps)
            else:
                I = orc.short_characteristics_down(k, S_l, np.zeros((ny, nx)), a_l, z, x, y, n_sweeps)
            J[:, l] += w[a] * I.ravel()
    return J, gamma


def _oracle_lambda(case, z, x, y, quadrature, maxiter, eps_conv=0.0):
    """Λ_regular's loop (src/lambda_iteration.jl:159-193) with the oracle's restatements"""
    pops = case.lte.copy()
    S_new, S_old = case.B0.copy(), np.zeros_like(case.B0)
    hist, diff, i, J = [], np.inf, 0, None
    while diff > eps_conv and i < maxiter:
        S_old = S_new.copy()
        J, gamma = _oracle_J(S_old, pops, z, x, y, case, quadrature)
        S_new = (1 - case.eps)[:, None] * J + case.eps[:, None] * case.B0
        diff = float(np.abs(1 - S_old / S_new).max())
        R = orc.calculate_R(case.lam, case.blocks, J, case.planck2, case.lambda0, case.c0, case.doppler, gamma,
                            case.sigma_bb_const, case.sigma_bf1, case.sigma_bf2, case.temperature, case.lte,
                            case.hc_over_kB, case.pref_ij, case.pref_ji)
        pops = orc.revised_populations(R, case.C, case.atom_density)
        hist.append(diff)
        i += 1
    return J, S_new, pops, hist


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_regular_lambda_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert f"{name}(" in header, name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert "vrt_regular_lambda;" in header


def test_regular_lambda_refuses_null_arguments_without_a_device():
    """NULL handle, NULL arrays, a NULL line case: VRT_EINVAL before anything touches a device (child process)."""
    script = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from voronoirt_amd import _lib
L = _lib.load()
d = lambda a: a.ctypes.data_as(_lib.p_dbl)
k = np.array([-1.0, 0.0, 0.0]); w = np.ones(1); dirs = np.ones(1, dtype=np.int32); v = np.ones(64)
pi = dirs.ctypes.data_as(_lib.p_int)
fake = ctypes.c_void_p(8)
rc = []
rc.append(L.vrt_regular_execute_line(None, 1, d(k), pi, d(w), 2, d(v), 1.0, 1.0, d(v), d(v), d(v), d(v), d(v), d(v), None, 3, d(v)))
rc.append(L.vrt_regular_execute_line(fake, 1, d(k), pi, d(w), 2, None, 1.0, 1.0, d(v), d(v), d(v), d(v), d(v), d(v), None, 3, d(v)))
rc.append(L.vrt_regular_execute_line(fake, 1, None, pi, d(w), 2, d(v), 1.0, 1.0, d(v), d(v), d(v), d(v), d(v), d(v), None, 3, d(v)))
rc.append(L.vrt_regular_execute_line(fake, 1, d(k), pi, d(w), 2, d(v), 1.0, 1.0, d(v), d(v), d(v), d(v), d(v), d(v), None, 3, None))
h = ctypes.c_void_p()
rc.append(L.vrt_regular_lambda_create(fake, 1, d(k), pi, d(w), None, 3, ctypes.byref(h)))
lc = _lib.LineCaseStruct()
lc.nlam = 4
rc.append(L.vrt_regular_lambda_create(None, 1, d(k), pi, d(w), ctypes.byref(lc), 3, ctypes.byref(h)))
rc.append(L.vrt_regular_lambda_create(fake, 1, d(k), pi, d(w), ctypes.byref(lc), 3, ctypes.byref(h)))   # NULL arrays
rc.append(L.vrt_regular_lambda_create(fake, 1, d(k), pi, d(w), ctypes.byref(lc), 3, None))
rc.append(L.vrt_regular_lambda_iterate(None, None))
rc.append(L.vrt_regular_lambda_get(None, None, None, None, None, None))
L.vrt_regular_lambda_destroy(None)
print(" ".join(str(r) for r in rc), h.value is None)
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    *codes, null_out = r.stdout.split()
    assert codes and all(int(c) == _lib.VRT_EINVAL for c in codes), r.stdout
    assert null_out == "True"


def test_regular_oracle_lambda_iteration_is_well_posed(raster, tmp_path):
    """The synthetic raster case keeps the loop physical: finite fields, positive populations that sum to the atom
    density, a contracting criterion, line centre optically thick and the wings thin across the height."""
    z, x, y, case = raster
    J, S, pops, hist = _oracle_lambda(case, z, x, y, "ul7n12.dat", 3)
    assert np.isfinite(J).all() and np.isfinite(S).all() and (pops > 0).all()
    assert np.allclose(pops.sum(axis=0), case.atom_density, rtol=1e-12)
    assert hist[2] < hist[1] < hist[0]
    assert np.abs(pops[1] / case.lte[1] - 1).max() > 1e-3          # the radiation field moved the populations
    strength = case.strength_const * (case.lte[0] * case.Bij - case.lte[1] * case.Bji)
    al = orc.line_opacity(orc.direction(180.0, 0.0), case.lam, case.lambda0, case.c0, case.velocity, case.doppler,
                          case.gamma(case.lte), strength, case.alpha_cont)
    tau = al.mean(axis=0) * (z[-1] - z[0])
    assert tau[10] > 10 and tau[0] < 1 and tau[20] < 1
    # the ghost border holds the wrapped interior (get_atmos(...; periodic=true))
    T = case.temperature.reshape(y.size, x.size, z.size)
    assert np.array_equal(T[0], T[-2]) and np.array_equal(T[:, 0], T[:, -2]) and np.array_equal(T[:, -1], T[:, 1])


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _case_struct(case):
    return case.c_struct()


@pytest.mark.gpu
def test_gpu_regular_lambda_rejects_bad_arguments_before_launch(raster):
    z, x, y, case = raster
    L = _lib.load()
    solver = vrt.RegularSolver(z, x, y)
    d = lambda a: a.ctypes.data_as(_lib.p_dbl)
    lc, keep = _case_struct(case)
    k = vrt.quadrature_directions([150.0, 30.0], [10.0, 200.0])
    w = np.array([0.5, 0.5])
    dirs = np.array([1, -1], dtype=np.int32)
    pi = lambda a: a.ctypes.data_as(_lib.p_int)
    h = ctypes.c_void_p()

    def create(n_angles=2, kk=k, dd=dirs, lcs=lc, n_sweeps=3):
        return L.vrt_regular_lambda_create(solver._h, n_angles, d(kk), pi(dd), d(w), ctypes.byref(lcs), n_sweeps,
                                           ctypes.byref(h))

    assert create(n_angles=0) == _lib.VRT_EINVAL
    bad = k.copy()
    bad[0] *= 1.1
    assert create(kk=bad) == _lib.VRT_EINVAL                      # |k| != 1
    flat = k.copy()
    flat[1] = [0.0, 1.0, 0.0]
    assert create(kk=flat) == _lib.VRT_EINVAL                     # k_z = 0 with dirs != 0 ...
    assert create(kk=flat, dd=np.array([1, 0], dtype=np.int32)) == 0     # ... is fine for a skipped angle
    L.vrt_regular_lambda_destroy(h)
    h = ctypes.c_void_p()
    assert create(dd=np.array([1, 2], dtype=np.int32)) == _lib.VRT_EINVAL
    assert create(n_sweeps=0) == _lib.VRT_EINVAL
    lc1, _ = _case_struct(case)
    lc1.nlam = 1
    assert create(lcs=lc1) == _lib.VRT_EINVAL                     # nlam < 2
    lc2, _ = _case_struct(case)
    lc2.blocks[1] = lc2.nlam + 1
    assert create(lcs=lc2) == _lib.VRT_EINVAL                     # bad blocks
    lc3, _ = _case_struct(case)
    lc3.blocks[3] = lc3.blocks[2] + 1
    assert create(lcs=lc3) == _lib.VRT_EINVAL
    assert h.value is None
    n, nlam = case.doppler.size, keep["lam"].size
    S, J, v = np.ones((n, nlam)), np.zeros((n, nlam)), np.ones(3 * n)

    def line(n_angles=2, kk=k, nl=nlam):
        return L.vrt_regular_execute_line(solver._h, n_angles, d(kk), pi(dirs), d(w), nl, d(keep["lam"]), 1.0, 1.0, d(v),
                                          d(v), d(v), d(v), d(v), d(S), None, 3, d(J))

    assert line(n_angles=0) == _lib.VRT_EINVAL
    assert line(kk=bad) == _lib.VRT_EINVAL
    assert line(kk=flat) == _lib.VRT_EINVAL
    assert line(nl=0) == _lib.VRT_EINVAL
    # the handle still works: a whole J and one iteration
    pops = case.lte
    J_ok = vrt.J_lambda_regular_line(case.B0, pops, z, x, y, case, "ul7n12.dat")
    assert np.isfinite(J_ok).all() and (J_ok > 0).any()
    assert create() == 0
    diff = ctypes.c_double()
    assert L.vrt_regular_lambda_iterate(h, ctypes.byref(diff)) == 0 and np.isfinite(diff.value)
    L.vrt_regular_lambda_destroy(h)
    solver.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quad", ["mixed", "steep"])
def test_gpu_J_lambda_regular_line_matches_oracle(raster, tmp_path, quad):
    """Σ_a w_a I_a of ups, downs and a θ = 90 angle that adds nothing (mixed), and of a batch of steep rays only (the
    split xy path), against the oracle's α_tot + short characteristics"""
    z, x, y, case = raster
    q = _quad(tmp_path, "mixn5.dat", MIXED) if quad == "mixed" else _quad(tmp_path, "steepn4.dat", STEEP)
    rng = np.random.default_rng(3)
    S = case.B0 * (0.5 + rng.random(case.B0.shape))
    pops = case.lte * (1 + 0.1 * rng.random(case.lte.shape))
    J = vrt.J_lambda_regular_line(S, pops, z, x, y, case, q)
    J_ref, _ = _oracle_J(S, pops, z, x, y, case, q)
    assert np.abs(J - J_ref).max() < 1e-10 * np.abs(J_ref).max()
    if quad == "mixed":                                # the θ = 90 angle adds nothing: the set without it gives the same J
        w, th, ph, _ = vrt.read_quadrature(q)
        rows = [ln for ln in MIXED.splitlines() if float(ln.split()[1]) != 90.0]
        J4 = vrt.J_lambda_regular_line(S, pops, z, x, y, case, _quad(tmp_path, "mixn4.dat", "\n".join(rows) + "\n"))
        assert np.array_equal(J4, J)


@pytest.mark.gpu
def test_gpu_execute_line_reads_I0_up_in_the_documented_layout(raster, tmp_path):
    """vrt_regular_execute_line called directly: I0_up is (nx, ny, nλ) in the header's column-major convention, element
    [ix + nx (iy + ny l)] -- numpy (nλ, ny, nx) -- here random and different per wavelength on a raster with nx != ny,
    against the oracle's up solves from the same planes"""
    z, x, y, case = raster
    nz, nx, ny = z.size, x.size, y.size
    assert nx != ny
    q = _quad(tmp_path, "mixn5.dat", MIXED)
    w, th, ph, nq = vrt.read_quadrature(q)
    k = vrt.quadrature_directions(th, ph)
    dirs = np.array([1 if t > 90 else (-1 if t < 90 else 0) for t in th], dtype=np.int32)
    rng = np.random.default_rng(11)
    n, nlam = case.B0.shape
    S = case.B0 * (0.5 + rng.random((n, nlam)))
    I0 = np.ascontiguousarray(2.0 * rng.random((nlam, ny, nx)))     # (nx, ny, nλ) column-major
    pops = case.lte
    gamma, strength = orc.line_terms(case.gamma_static, case.gamma_unsold, pops, case.strength_const, case.Bij, case.Bji)
    J = np.zeros((n, nlam))
    d = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_lib.p_dbl)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (k, w, case.lam, case.velocity, case.doppler, gamma, strength,
                                                               case.alpha_cont, S)]
    solver = vrt.RegularSolver(z, x, y)
    rc = _lib.load().vrt_regular_execute_line(solver._h, nq, d(keep[0]), dirs.ctypes.data_as(_lib.p_int), d(keep[1]), nlam,
                                               d(keep[2]), float(case.lambda0), float(case.c0), d(keep[3]), d(keep[4]),
                                               d(keep[5]), d(keep[6]), d(keep[7]), d(keep[8]), d(I0), 3,
                                               J.ctypes.data_as(_lib.p_dbl))
    solver.close()
    assert rc == 0
    J_ref, _ = _oracle_J(S, pops, z, x, y, case, q, I0_up=I0)
    assert np.abs(J - J_ref).max() < 1e-10 * np.abs(J_ref).max()
    # the planes do matter: the transposed reading of them is far off
    J_t, _ = _oracle_J(S, pops, z, x, y, case, q, I0_up=I0.reshape(ny, nx, nlam).transpose(2, 0, 1))
    assert np.abs(J_t - J_ref).max() > 1e-3 * np.abs(J_ref).max()


@pytest.mark.gpu
def test_gpu_lambda_regular_matches_oracle_loop(raster):
    z, x, y, case = raster
    J, S, pops, hist = vrt.Lambda_regular(0.0, 4, z, x, y, case, "ul7n12.dat")
    J_ref, S_ref, pops_ref, hist_ref = _oracle_lambda(case, z, x, y, "ul7n12.dat", 4)
    assert len(hist) == 4
    assert np.abs(J - J_ref).max() < 1e-9 * np.abs(J_ref).max()
    assert np.abs(S / S_ref - 1).max() < 1e-9
    assert np.abs(pops / pops_ref - 1).max() < 1e-9
    assert np.allclose(hist, hist_ref, rtol=1e-8)
    # a tolerance of 1 or more runs no iteration: B_0 and the LTE populations come back
    J0, S0, p0, h0 = vrt.Lambda_regular(1.0, 10, z, x, y, case, "ul7n12.dat")
    assert h0 == [] and np.array_equal(S0, case.B0) and np.array_equal(p0, case.lte) and not J0.any()
    # a tolerance just above history[k] stops after the iteration the oracle stops at
    below = [i for i, h in enumerate(hist) if h < 1.0]
    assert below
    eps = hist[below[0]] * 1.0001
    expect = next(i for i, h in enumerate(hist_ref) if h <= eps) + 1
    J2, S2, p2, h2 = vrt.Lambda_regular(eps, 10, z, x, y, case, "ul7n12.dat")
    assert len(h2) == expect
    assert len(_oracle_lambda(case, z, x, y, "ul7n12.dat", 10, eps_conv=eps)[3]) == expect
    assert np.array_equal(S2, vrt.Lambda_regular(0.0, expect, z, x, y, case, "ul7n12.dat")[1])


@pytest.mark.gpu
def test_gpu_lambda_regular_bit_identical_under_chunking(raster, tmp_path, monkeypatch):
    """One-solve chunks (VRT_REG_LAMBDA_BYTES = 1, read when the regular handle is created) and the default chunking give
    the same J, S and populations bit for bit; the mixed set puts steep and shallow solves into the same default chunk"""
    z, x, y, case = raster
    q = _quad(tmp_path, "mixn5.dat", MIXED)
    ref = vrt.Lambda_regular(0.0, 3, z, x, y, case, q)
    monkeypatch.setenv("VRT_REG_LAMBDA_BYTES", "1")
    one = vrt.Lambda_regular(0.0, 3, z, x, y, case, q)
    for a, b in zip(ref[:3], one[:3]):
        assert np.array_equal(a, b)
    assert ref[3] == one[3]
    S = case.B0 * 1.1
    J1 = vrt.J_lambda_regular_line(S, case.lte, z, x, y, case, q)
    monkeypatch.delenv("VRT_REG_LAMBDA_BYTES")
    assert np.array_equal(J1, vrt.J_lambda_regular_line(S, case.lte, z, x, y, case, q))
