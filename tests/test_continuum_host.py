"""The continuum scattering Λ-iteration (src/lambda_continuum.jl), host side (no GPU): the entry points are declared,
exported and bound, their argument checks answer VRT_EINVAL before a device is touched, and the loop driven by the
oracle alone -- orc.J_voronoi on a BCC grid, orc.short_characteristics_up/down on a raster -- is well posed on the
synthetic cases of synth.continuum_case / synth.regular_continuum_case.  The oracle-driven loops defined here are the
reference of tests/test_continuum.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD = "ul7n12.dat"
NEW = ("vrt_continuum_case_check", "vrt_continuum_create", "vrt_continuum_iterate", "vrt_continuum_get",
       "vrt_continuum_set_source", "vrt_continuum_set_acceleration", "vrt_continuum_last_acceleration",
       "vrt_continuum_destroy", "vrt_regular_continuum_create", "vrt_regular_continuum_iterate",
       "vrt_regular_continuum_get", "vrt_regular_continuum_set_source", "vrt_regular_continuum_set_acceleration",
       "vrt_regular_continuum_last_acceleration", "vrt_regular_continuum_destroy", "vrt_continuum_update_dev")


# ---- the loops with the oracle's restatements (src/lambda_continuum.jl) ---------------------------------------------------
def oracle_J_voronoi(case, so, S, quadrature=QUAD, I0_up=None):
    """J_λ_voronoi (:27-56): I_0 of the up solves is B_0 of the bottom layer perm_up[1 : layers_up[2] - 1] (:45-47)"""
    w, th, ph, _ = vrt.read_quadrature(quadrature)
    n1 = int(so.layers_up[1] - 1)
    if I0_up is None:
        I0_up = case.B0[so.perm_up[:n1] - 1]
    return orc.J_voronoi(w, th, ph, S, case.alpha, so, I0_up=I0_up)


def oracle_J_regular(case, z, x, y, S, quadrature=QUAD):
    """J_λ_regular (:1-24): I_0 of the up solves is B_0's bottom plane (:16), the down solves start from zeros (:19)"""
    w, th, ph, nq = vrt.read_quadrature(quadrature)
    nz, nx, ny = z.size, x.size, y.size
    J = np.zeros_like(S)
    for a in range(nq):
        if th[a] == 90:
            continue
        k = orc.direction(th[a], ph[a])
        for l in range(S.shape[1]):
            S_l, a_l = S[:, l].reshape(ny, nx, nz), case.alpha[:, l].reshape(ny, nx, nz)
            if th[a] > 90:
                I = orc.short_characteristics_up(k, S_l, case.B0[:, l].reshape(ny, nx, nz)[:, :, 0], a_l, z, x, y, 3)
            else:
                I = orc.short_characteristics_down(k, S_l, np.zeros((ny, nx)), a_l, z, x, y, 3)
            J[:, l] += w[a] * I.ravel()
    return J


def oracle_loop(case, J_of, maxiter, eps_conv=0.0, S0=None):
    """Λ_voronoi / Λ_regular (:145-150, :92-97) and criterion (:162-198).  Returns J, S, the history of the masked maximum
    and that of the unmasked one."""
    thick = case.thick()
    S_new = case.B0.copy() if S0 is None else np.array(S0, dtype=np.float64)
    hist, hist_all, diff, i, J = [], [], np.inf, 0, np.zeros_like(case.B0)
    while diff > eps_conv and i < maxiter:
        S_old = S_new.copy()
        J = J_of(S_old)
        S_new = (1 - case.eps) * J + case.eps * case.B0
        rel = np.abs(1 - S_old / S_new)
        diff = float(rel[thick].max())
        hist.append(diff)
        hist_all.append(float(rel.max()))
        i += 1
    return J, S_new, hist, hist_all


def bcc_case(nlam, seed=11):
    pos, nbr, bounds = synth.bcc_grid(6, 9, seed=11)
    return pos, nbr, bounds, vrt.ContinuumCase(**synth.continuum_case(pos, bounds, nlam, seed))


def raster_case(nlam=2, seed=7):
    z, x, y, kw = synth.regular_continuum_case(16, 10, 9, seed, nlam)
    return z, x, y, vrt.ContinuumCase(**kw)


# ---- symbols ---------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_continuum_symbols_declared_and_exported():
    text, code = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert "vrt_continuum_case;" in code and "vrt_regular_continuum;" in code
    # no multi-device continuum session, and the header says so
    assert not re.search(r"vrt_multi_continuum", code)
    assert "NO multi-device continuum session" in text
    for name in ("ContinuumCase", "Lambda_continuum", "Lambda_continuum_regular", "continuum_update_dev"):
        assert hasattr(vrt, name), name


def test_continuum_case_struct_agrees_with_the_header():
    _, code = _header()
    m = re.search(r"typedef struct vrt_continuum_case \{(.*?)\} vrt_continuum_case;", code, flags=re.S)
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int64_t nlam", "const double *alpha", "const double *eps", "const double *B0", "double eps_thick"]
    assert [f for f, _ in _lib.ContinuumCaseStruct._fields_] == ["nlam", "alpha", "eps", "B0", "eps_thick"]


# ---- argument checks ------------------------------------------------------------------------------------------------------
def test_continuum_refuses_bad_arguments_without_a_device():
    """NULL pointers, nlam < 1, eps_thick not finite, the direction checks of the regular session, the acceleration
    settings' NULL session: VRT_EINVAL in a child process that sees no device (the handles are never dereferenced)."""
    script = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from voronoirt_amd import _lib
L = _lib.load()
d = lambda a: a.ctypes.data_as(_lib.p_dbl)
v = np.ones(8); w = np.ones(1); k = np.array([-1.0, 0.0, 0.0]); dirs = np.ones(1, dtype=np.int32)
pi = lambda a: a.ctypes.data_as(_lib.p_int)
fake = ctypes.c_void_p(8)
def case(nlam=1, alpha=v, eps=v, B0=v, thick=1e-4):
    cc = _lib.ContinuumCaseStruct()
    cc.nlam = nlam
    cc.alpha, cc.eps, cc.B0 = (d(a) if a is not None else None for a in (alpha, eps, B0))
    cc.eps_thick = thick
    return cc
ok = case()
h = ctypes.c_void_p()
rc = []
rc.append(L.vrt_continuum_create(None, ctypes.byref(ok), d(w), ctypes.byref(h)))
rc.append(L.vrt_continuum_create(fake, None, d(w), ctypes.byref(h)))
rc.append(L.vrt_continuum_create(fake, ctypes.byref(ok), None, ctypes.byref(h)))
rc.append(L.vrt_continuum_create(fake, ctypes.byref(ok), d(w), None))
for bad in (case(nlam=0), case(alpha=None), case(eps=None), case(B0=None), case(thick=float("nan")), case(thick=float("inf"))):
    rc.append(L.vrt_continuum_create(fake, ctypes.byref(bad), d(w), ctypes.byref(h)))
    rc.append(L.vrt_regular_continuum_create(fake, 1, d(k), pi(dirs), d(w), ctypes.byref(bad), 3, ctypes.byref(h)))
rc.append(L.vrt_regular_continuum_create(None, 1, d(k), pi(dirs), d(w), ctypes.byref(ok), 3, ctypes.byref(h)))
rc.append(L.vrt_regular_continuum_create(fake, 1, None, pi(dirs), d(w), ctypes.byref(ok), 3, ctypes.byref(h)))
rc.append(L.vrt_regular_continuum_create(fake, 1, d(k), None, d(w), ctypes.byref(ok), 3, ctypes.byref(h)))
rc.append(L.vrt_regular_continuum_create(fake, 1, d(k), pi(dirs), None, ctypes.byref(ok), 3, ctypes.byref(h)))
rc.append(L.vrt_regular_continuum_create(fake, 1, d(k), pi(dirs), d(w), None, 3, ctypes.byref(h)))
rc.append(L.vrt_regular_continuum_create(fake, 1, d(k), pi(dirs), d(w), ctypes.byref(ok), 3, None))
rc.append(L.vrt_regular_continuum_create(fake, 1, d(k), pi(dirs), d(w), ctypes.byref(ok), 0, ctypes.byref(h)))      # n_sweeps
rc.append(L.vrt_regular_continuum_create(fake, 0, d(k), pi(dirs), d(w), ctypes.byref(ok), 3, ctypes.byref(h)))      # n_angles
rc.append(L.vrt_regular_continuum_create(fake, 1, d(1.1 * k), pi(dirs), d(w), ctypes.byref(ok), 3, ctypes.byref(h)))   # |k| != 1
flat = np.array([0.0, 1.0, 0.0])
rc.append(L.vrt_regular_continuum_create(fake, 1, d(flat), pi(dirs), d(w), ctypes.byref(ok), 3, ctypes.byref(h)))   # k_z = 0
rc.append(L.vrt_regular_continuum_create(fake, 1, d(k), pi(np.array([2], dtype=np.int32)), d(w), ctypes.byref(ok), 3, ctypes.byref(h)))
out = ctypes.c_double()
for pre in ("vrt_continuum_", "vrt_regular_continuum_"):
    rc.append(getattr(L, pre + "iterate")(None, ctypes.byref(out)))
    rc.append(getattr(L, pre + "iterate")(fake, None))
    rc.append(getattr(L, pre + "get")(None, None, None))
    rc.append(getattr(L, pre + "set_source")(None, d(v)))
    rc.append(getattr(L, pre + "set_source")(fake, None))
    rc.append(getattr(L, pre + "set_acceleration")(None, 2, 4, 4))
    for order, start, period in ((1, 4, 4), (2, 3, 4), (2, 4, 3)):
        rc.append(getattr(L, pre + "set_acceleration")(fake, order, start, period))
    rc.append(getattr(L, pre + "last_acceleration")(None, None, None, None))
    getattr(L, pre + "destroy")(None)
cnt = ctypes.c_int64()
upd = lambda g=fake, nlam=1, ld=1, J=fake, o=ctypes.byref(out), thick=1e-4: L.vrt_continuum_update_dev(
    g, nlam, ld, J, fake, fake, thick, fake, fake, o, ctypes.byref(cnt), None)
rc += [upd(g=None), upd(J=None), upd(o=None), upd(nlam=0), upd(nlam=2, ld=1), upd(thick=float("nan"))]
print(" ".join(str(r) for r in rc), h.value is None)
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    *codes, null_out = r.stdout.split()
    assert len(codes) > 40 and all(int(c) == _lib.VRT_EINVAL for c in codes), r.stdout
    assert null_out == "True"


def test_continuum_case_check_refuses_bad_arrays_without_a_device():
    """what create says about the arrays of a case (vrt_continuum_case_check, the same function): α not finite or <= 0, ε
    outside [0, 1] or not finite, B0 not finite, no thick entry"""
    pos, nbr, bounds, case = bcc_case(3)
    case.check()

    def code(**kw):
        c = vrt.ContinuumCase(**{**dict(alpha=case.alpha, eps=case.eps, B0=case.B0, eps_thick=case.eps_thick), **kw})
        try:
            c.check()
        except vrt.VrtError as e:
            return e.code
        return 0

    def planted(a, value, where=(5, 2)):
        b = a.copy()
        b[where] = value
        return b

    for bad in (0.0, -1.0, np.nan, np.inf):
        assert code(alpha=planted(case.alpha, bad)) == _lib.VRT_EINVAL, bad
    for bad in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
        assert code(eps=planted(case.eps, bad)) == _lib.VRT_EINVAL, bad
    assert code(eps=planted(planted(case.eps, 0.0), 1.0, (6, 0))) == 0             # the closed ends are fine
    for bad in (np.nan, np.inf, -np.inf):
        assert code(B0=planted(case.B0, bad)) == _lib.VRT_EINVAL, bad
    assert code(B0=planted(case.B0, -1.0)) == 0                                    # (finite is all B0 has to be)
    # no thick entry: strict comparison, so a threshold AT the largest ε leaves none
    assert code(eps_thick=float(case.eps.max())) == _lib.VRT_EINVAL
    assert code(eps_thick=float(np.nextafter(case.eps.max(), 0))) == 0
    assert code(eps_thick=-1.0) == 0                                               # everything thick
    cc = case.c_struct()
    assert _lib.load().vrt_continuum_case_check(ctypes.byref(cc), 0) == _lib.VRT_EINVAL
    assert _lib.load().vrt_continuum_case_check(None, case.n) == _lib.VRT_EINVAL


# ---- the oracle loop is well posed -----------------------------------------------------------------------------------------
def _well_posed(case, J_of, iters=6):
    thick = case.thick()
    assert thick.any(axis=0).all() and (~thick).any(axis=0).all()         # thin and thick entries at every wavelength
    J, S, hist, hist_all = oracle_loop(case, J_of, iters)
    assert np.isfinite(S).all() and (S > 0).all() and np.isfinite(J).all()
    assert all(b < a for a, b in zip(hist[1:], hist[2:])), hist          # decreasing after the first entries
    assert any(a != b for a, b in zip(hist[:3], hist_all[:3])), (hist, hist_all)   # the mask matters early on
    assert all(a <= b for a, b in zip(hist, hist_all))
    return hist, hist_all


@pytest.mark.parametrize("nlam", [1, 3])
def test_oracle_continuum_loop_on_the_bcc_grid_is_well_posed(nlam):
    pos, nbr, bounds, case = bcc_case(nlam)
    so = orc.make_sites(pos, nbr, bounds)
    hist, hist_all = _well_posed(case, lambda S: oracle_J_voronoi(case, so, S))
    # α puts τ = 1 inside the box: the column of the mean opacity is a few
    z = pos[:, 0]
    order = np.argsort(z)
    a0 = case.alpha[order, 0]
    tau = float((0.5 * (a0[1:] + a0[:-1]) * np.diff(z[order])).sum())
    assert 1.0 < tau < 30.0
    assert 0.5 < case.eps.max() <= 1.0 and case.eps.min() < 1e-5


def test_oracle_continuum_loop_on_the_raster_is_well_posed():
    z, x, y, case = raster_case(2)
    _well_posed(case, lambda S: oracle_J_regular(case, z, x, y, S), iters=5)
    # the ghost border holds the wrapped interior exactly
    for a in (case.alpha, case.eps, case.B0):
        f = a.reshape(y.size, x.size, z.size, case.nlam)
        assert np.array_equal(f[0], f[-2]) and np.array_equal(f[-1], f[1])
        assert np.array_equal(f[:, 0], f[:, -2]) and np.array_equal(f[:, -1], f[:, 1])
