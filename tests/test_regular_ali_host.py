"""Accelerated Λ-iteration with the diagonal operator Λ* on the regular-grid continuum session, host side (no GPU): the
entry points are declared, exported and bound, their argument checks answer VRT_EINVAL before a device is touched, and the
ALI loop driven by the oracle alone is well posed and pays on a thick case.

The reference of Λ* restates none of the six plane kernels: it is the oracle's own unit response,
    ref[p, l] = J(S = e_p, I_0 = 0)[p]    from orc.short_characteristics_up/down with ONE sweep
(`lambda_star_regular_ref`), the diagonal of the one-sweep Λ.  In an xy plane that is Σ_a w_a b(Δτ) alone.  In a yz / xz
plane the point's S also comes back within the sweep through the row marched just before it (whose upwind source function
is interpolated in the point's row and whose intensity is the carried row of the point's update), and xz_down_ray reads
its centre S from the plane above, so there the point's own S has no b term at all: what include/voronoirt.h writes as
c_a(p, l).  `lambda_star_regular_ref` and `oracle_J_regular_sweeps` are the reference of tests/test_regular_ali.py."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import _lib
from test_continuum_host import QUAD, oracle_J_regular, oracle_loop, raster_case
from test_ali_host import oracle_ali_loop, scaled_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrt_regular_lambda_diagonal_dev", "vrt_regular_lambda_diagonal", "vrt_regular_continuum_select_operator",
       "vrt_regular_continuum_get_operator")


# ---- the reference ------------------------------------------------------------------------------------------------------------
def oracle_J_regular_sweeps(alpha, B0, z, x, y, S, quadrature=QUAD, n_sweeps=3, I0_up=None):
    """oracle_J_regular (tests/test_continuum_host.py) with the sweep count and I_0 of the up solves as parameters
    (I0_up None: B_0's bottom plane, as there; else an (ny, nx) plane used at every wavelength)"""
    w, th, ph, nq = vrt.read_quadrature(quadrature)
    nz, nx, ny = z.size, x.size, y.size
    J = np.zeros_like(S)
    for a in range(nq):
        if th[a] == 90:
            continue
        k = orc.direction(th[a], ph[a])
        for l in range(S.shape[1]):
            S_l, a_l = S[:, l].reshape(ny, nx, nz), alpha[:, l].reshape(ny, nx, nz)
            if th[a] > 90:
                I0 = B0[:, l].reshape(ny, nx, nz)[:, :, 0] if I0_up is None else I0_up
                I = orc.short_characteristics_up(k, S_l, I0, a_l, z, x, y, n_sweeps)
            else:
                I = orc.short_characteristics_down(k, S_l, np.zeros((ny, nx)), a_l, z, x, y, n_sweeps)
            J[:, l] += w[a] * I.ravel()
    return J


def unit_response(alpha, z, x, y, quadrature=QUAD, n_sweeps=1):
    """[p, l] -> J(S = e_p, I_0 = 0)[p] at wavelength l: the diagonal of the oracle's Λ with that many sweeps"""
    alpha = np.asarray(alpha, dtype=np.float64)
    n, nlam = alpha.shape
    zero = np.zeros((y.size, x.size))
    out = np.zeros((n, nlam))
    for l in range(nlam):
        a_l = np.ascontiguousarray(alpha[:, l:l + 1])
        for p in range(n):
            S = np.zeros((n, 1))
            S[p, 0] = 1.0
            out[p, l] = oracle_J_regular_sweeps(a_l, None, z, x, y, S, quadrature, n_sweeps, I0_up=zero)[p, 0]
    return out


@functools.lru_cache(maxsize=None)
def lambda_star_regular_ref(nlam=1, factor=1.0, quadrature=QUAD, n_sweeps=1):
    """the unit response of raster_case(nlam) with α × factor, computed once per process; read-only"""
    z, x, y, case = raster_case(nlam)
    ref = unit_response(case.alpha * factor, z, x, y, quadrature, n_sweeps)
    ref.setflags(write=False)
    return ref


def ghost_mask(z, x, y):
    g = np.ones((y.size, x.size, z.size), dtype=bool)
    g[1:-1, 1:-1, :] = False
    return g.ravel()


def cut_kinds(z, x, y, quadrature=QUAD):
    """per direction (True up, False down) the set of argmin(r_z, r_x, r_y) over the angles and planes (characteristics.jl:71-72;
    1 xy, 2 yz, 3 xz; the first minimum wins)"""
    w, th, ph, nq = vrt.read_quadrature(quadrature)
    kinds = {True: set(), False: set()}
    for a in range(nq):
        if th[a] == 90:
            continue
        k = orc.direction(th[a], ph[a])
        with np.errstate(divide="ignore"):
            r_x, r_y = abs((x[1] - x[0]) / k[1]), abs((y[1] - y[0]) / k[2])
        for dz in np.diff(z):
            kinds[bool(th[a] > 90)].add(1 + int(np.argmin([abs(dz / k[0]), r_x, r_y])))
    return kinds


# ---- 1: symbols ------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_regular_ali_symbols_declared_exported_and_bound():
    text, code = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    for name in ("lambda_diagonal_regular", "Lambda_continuum_regular"):
        assert hasattr(vrt, name), name
    import inspect
    assert inspect.signature(vrt.Lambda_continuum_regular).parameters["operator"].default is None
    with pytest.raises(ValueError, match="operator must be None or 'diagonal'"):
        vrt.Lambda_continuum_regular(0.0, 1, None, None, None, None, QUAD, operator="jacobi")
    # what stays out of scope is said next to the entries: the raster's exact n_sweeps diagonal, the line sessions and any
    # multi-device form; no line or multi-device operator entry exists
    scope = text[text.index("Out of scope:"):]
    scope = " ".join(scope[:scope.index("*/")].replace("*", " ").split())
    assert "one-sweep diagonal" in scope and "the line sessions" in scope and "any multi-device form" in scope
    assert not re.search(r"vrt_(lambda|regular_lambda|multi\w*)_(set|select)_operator", code)


def test_regular_ali_prototypes_agree_with_the_header():
    _, code = _header()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        res, bound = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(bound) == len(args), (name, args)
        for a, b in zip(args, bound):
            if re.fullmatch(r"int \w+", a):
                want = ctypes.c_int
            elif re.fullmatch(r"int64_t \w+", a):
                want = ctypes.c_int64
            elif re.fullmatch(r"(const )?int \*\w+", a):
                want = _lib.p_int
            elif re.fullmatch(r"(const )?double \*d_\w+", a):             # device arrays
                want = ctypes.c_void_p
            elif re.fullmatch(r"(const )?double \*\w+", a):
                want = _lib.p_dbl
            else:                                                          # handles
                assert re.fullmatch(r"(vrt_regular|vrt_regular_continuum) \*\w+", a), (name, a)
                want = ctypes.c_void_p
            assert b is want, (name, a, b)


# ---- 2: argument checks ------------------------------------------------------------------------------------------------------
def test_regular_ali_refuses_bad_arguments_without_a_device():
    """NULL pointers, nlam < 1, ld < nlam, the direction checks, an operator other than 0 or 1: VRT_EINVAL in a child process
    that sees no device (the handles are never dereferenced).  The host form's check of α needs the point count, that is a
    real handle: tests/test_regular_ali.py makes that check on one."""
    script = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from voronoirt_amd import _lib
L = _lib.load()
d = lambda a: a.ctypes.data_as(_lib.p_dbl)
pi = lambda a: a.ctypes.data_as(_lib.p_int)
v = np.ones(8); w = np.ones(1); k = np.array([-1.0, 0.0, 0.0]); dirs = np.ones(1, dtype=np.int32)
fake = ctypes.c_void_p(8)
op = ctypes.c_int()
rc = []
dev = lambda r=fake, na=1, k_=d(k), di=pi(dirs), wt=d(w), nlam=1, ld=1, a=fake, o=fake: \
    L.vrt_regular_lambda_diagonal_dev(r, na, k_, di, wt, nlam, ld, a, o)
host = lambda r=fake, na=1, k_=d(k), di=pi(dirs), wt=d(w), nlam=1, ld=1, a=d(v), o=d(v): \
    L.vrt_regular_lambda_diagonal(r, na, k_, di, wt, nlam, ld, a, o)
flat = np.array([0.0, 1.0, 0.0]); two = np.array([2], dtype=np.int32)
for f in (dev, host):
    rc += [f(r=None), f(k_=None), f(di=None), f(wt=None), f(a=None), f(o=None), f(nlam=0), f(nlam=-1), f(nlam=2, ld=1),
           f(na=0), f(k_=d(1.1 * k)), f(k_=d(flat)), f(di=pi(two))]
rc += [L.vrt_regular_continuum_select_operator(None, 0), L.vrt_regular_continuum_select_operator(None, 1),
       L.vrt_regular_continuum_select_operator(fake, 2), L.vrt_regular_continuum_select_operator(fake, -1)]
rc += [L.vrt_regular_continuum_get_operator(None, ctypes.byref(op), None), L.vrt_regular_continuum_get_operator(fake, None, None)]
print(" ".join(str(r) for r in rc))
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    codes = r.stdout.split()
    assert len(codes) == 32 and all(int(c) == _lib.VRT_EINVAL for c in codes), r.stdout


# ---- 3: the reference is a local operator ----------------------------------------------------------------------------------
def test_unit_response_is_zero_on_the_ghost_border_and_positive_inside():
    z, x, y, case = raster_case(1)
    ref = lambda_star_regular_ref(1)
    ghost = ghost_mask(z, x, y)
    assert np.isfinite(ref).all() and (ref[ghost] == 0.0).all()
    inner = ref.reshape(y.size, x.size, z.size)[1:-1, 1:-1, 1:-1]          # off both boundary planes
    assert (inner > 0).all() and (ref >= 0).all() and (ref < 1).all()
    assert abs(ref[~ghost].mean() - 0.131) < 2e-3 and abs(ref.max() - 0.495) < 2e-3     # (the issue's measurement)


def test_unit_response_is_a_lower_bound_of_the_three_sweep_diagonal():
    """every coefficient of Λ is >= 0 and three sweeps repeat what one sweep does: the bound tests/test_ali.py uses"""
    z, x, y, case = raster_case(1)
    ref, exact = lambda_star_regular_ref(1), lambda_star_regular_ref(1, n_sweeps=3)
    assert (ref <= exact * (1 + 1e-12)).all()
    print(f"exact - ref: max {np.max(exact - ref):.3g}; sum ratio {ref.sum() / exact.sum():.6f}")
    assert ref.sum() > 0.9 * exact.sum()


def test_the_case_exercises_all_six_plane_kinds():
    z, x, y, _ = raster_case(1)
    kinds = cut_kinds(z, x, y)
    assert kinds[True] == {1, 2, 3} and kinds[False] == {1, 2, 3}, kinds
    # one vertical ray: r_x = r_y = inf, every plane is an xy plane
    assert cut_kinds(z, x, y, "n1.dat") == {True: {1}, False: set()}


# ---- 4: the oracle-driven ALI loop on the thick case --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thick100():
    """raster_case(1) with α × 100, its unit response, and both oracle loops run to 1e-8 (the iterate at which each passes
    1e-4 is read off its history: the loops are deterministic)"""
    z, x, y, case = raster_case(1)
    case100 = scaled_case(case, 100.0)
    diag = lambda_star_regular_ref(1, 100.0)
    J_of = lambda S: oracle_J_regular(case100, z, x, y, S)
    return {"case": case100, "diag": diag, "plain": oracle_loop(case100, J_of, 2000, 1e-8),
            "ali": oracle_ali_loop(case100, J_of, diag, 2000, 1e-8)}


def count_to(hist, tol):
    return next(i for i, h in enumerate(hist) if h <= tol) + 1


def test_oracle_regular_ali_loop_is_well_posed_and_needs_fewer_than_half_the_iterates(thick100):
    case, diag = thick100["case"], thick100["diag"]
    _, S0, h0, _ = thick100["plain"]
    _, S1, h1, _, smin = thick100["ali"]
    n0, n1 = count_to(h0, 1e-4), count_to(h1, 1e-4)
    print(f"raster_case(1), alpha x 100: to 1e-4 plain {n0} iterates, ALI {n1}; to 1e-8 plain {len(h0)}, ALI {len(h1)}; "
          f"min S over the ALI iterates {min(smin):.3g}; min den {np.min(1 - (1 - case.eps) * diag):.3g}; "
          f"S_ali / S_plain - 1: {np.abs(S1 / S0 - 1).max():.3g}")
    assert 2 * n1 < n0                                             # (measured 59 against 157)
    assert min(smin) > 0
    assert h0[-1] <= 1e-8 and h1[-1] <= 1e-8
    assert np.abs(S1 / S0 - 1).max() < 1e-6                        # the same fixed point (measured 1.6e-7)

