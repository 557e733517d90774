"""Accelerated Λ-iteration with the diagonal operator Λ* on the regular-grid LINE session, host side (no GPU): the entry
points are declared, exported and bound, their argument checks answer VRT_EINVAL before a device is touched, and the ALI
loop driven by the oracle alone is well posed, ends at the plain loop's fixed point and needs fewer iterates.

The reference of Λ* restates none of the six plane kernels: it is the oracle's own unit response with an α per angle,
    ref[p, l] = Σ_a w_a I_a(S = e_p, α = α_a[:, l], I_0 = 0)[p]    from orc.short_characteristics_up/down with ONE sweep
(`line_unit_response`).  `oracle_regular_line_loop`, `line_case_644`, `hard_case` and the iterate counts measured here are
the reference of tests/test_regular_line_ali.py."""
import ctypes
import functools
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import _lib, synth
from test_line_ali_host import fixed_point_bound, hard_case, oracle_alpha
from test_regular_ali_host import cut_kinds, ghost_mask, unit_response

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD = "ul7n12.dat"
NEW = ("vrt_regular_line_lambda_diagonal_dev", "vrt_regular_line_lambda_diagonal", "vrt_regular_lambda_use_operator",
       "vrt_regular_lambda_get_operator")
TARGET = 1e-3               # the tolerance the loops of the iterate-count comparison run to
# iterates of the oracle loops on line_case_644 to TARGET, measured by this file: standard case plain / ALI,
# hard variant plain / ALI.  The caps the tests apply are these counts plus a margin of two iterates.
COUNTS = {"standard": (33, 17), "hard": (178, 35)}
MARGIN = 2


# ---- the case and the reference ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def line_case_644():
    """a 6 x 6 x 6 raster with its ghost border, 216 points, 9 wavelengths: the smallest neighbourhood of shapes on which
    ul7n12 takes all six plane kinds (test_the_case_covers_all_six_plane_kinds)"""
    z, x, y, kw = synth.regular_line_case(6, 4, 4, seed=7, nbb=5, nbf=2)
    return z, x, y, vrt.LineCase(**kw)


def still_case(case):
    """the case with zero velocity: every angle sees the same α"""
    kw = {k: getattr(case, k) for k in vrt.LineCase.FIELDS}
    kw["velocity"] = np.zeros_like(np.asarray(case.velocity))
    return vrt.LineCase(**kw)


def line_unit_response(alpha, z, x, y, quadrature=QUAD):
    """[p, l] -> Σ_a w_a I_a(S = e_p, α_a[:, l], I_0 = 0)[p] with one sweep: the diagonal of the oracle's one-sweep Λ of the
    line loop.  alpha (n_angles, n, nlam), one α per angle of the quadrature (θ = 90 entries are not read)."""
    w, th, ph, nq = vrt.read_quadrature(quadrature)
    alpha = np.asarray(alpha, dtype=np.float64)
    _, n, nlam = alpha.shape
    ny, nx, nz = y.size, x.size, z.size
    zero = np.zeros((ny, nx))
    out = np.zeros((n, nlam))
    for a in range(nq):
        if th[a] == 90:
            continue
        k = orc.direction(th[a], ph[a])
        solve = orc.short_characteristics_up if th[a] > 90 else orc.short_characteristics_down
        for l in range(nlam):
            a_l = np.ascontiguousarray(alpha[a][:, l]).reshape(ny, nx, nz)
            for p in range(n):
                S = np.zeros(n)
                S[p] = 1.0
                out[p, l] += w[a] * solve(k, S.reshape(ny, nx, nz), zero, a_l, z, x, y, 1).ravel()[p]
    return out


def oracle_J_per_angle(S, alpha, B0, z, x, y, quadrature=QUAD, n_sweeps=3):
    """J_λ_regular's line method (test_regular_lambda._oracle_J) from the per-angle α it would form"""
    w, th, ph, nq = vrt.read_quadrature(quadrature)
    ny, nx, nz = y.size, x.size, z.size
    J = np.zeros_like(S)
    for a in range(nq):
        if th[a] == 90:
            continue
        k = orc.direction(th[a], ph[a])
        for l in range(S.shape[1]):
            S_l, a_l = S[:, l].reshape(ny, nx, nz), alpha[a][:, l].reshape(ny, nx, nz)
            if th[a] > 90:
                I = orc.short_characteristics_up(k, S_l, B0[:, l].reshape(ny, nx, nz)[:, :, 0], a_l, z, x, y, n_sweeps)
            else:
                I = orc.short_characteristics_down(k, S_l, np.zeros((ny, nx)), a_l, z, x, y, n_sweeps)
            J[:, l] += w[a] * I.ravel()
    return J


def oracle_regular_line_loop(case, z, x, y, maxiter, eps_conv=0.0, ali=False, quadrature=QUAD):
    """Λ_regular's loop (test_regular_lambda._oracle_lambda); ali: with Λ* = line_unit_response of this iterate's α and the
    update of test_line_ali_host.oracle_line_loop: t = 1 - ε, S_new = (t (J - Λ* S_old) + ε B0) / (1 - t Λ*), the plain
    update where the denominator is not > 0.  Returns J, S, populations, the history and what the iterates saw."""
    pops = case.lte.copy()
    S_new = case.B0.copy()
    B0 = np.asarray(case.B0)
    e = np.asarray(case.eps)[:, None]
    t = 1 - e
    seen = {"diag_min": np.inf, "diag_max": -np.inf, "den_min": np.inf, "fallback": 0, "S_min": np.inf}
    hist, diff, i, J = [], np.inf, 0, np.zeros_like(B0)
    while diff > eps_conv and i < maxiter:
        S_old = S_new.copy()
        gamma, alpha = oracle_alpha(case, pops, quadrature)
        J = oracle_J_per_angle(S_old, alpha, B0, z, x, y, quadrature)
        plain = (1 - e) * J + e * B0
        if ali:
            diag = line_unit_response(alpha, z, x, y, quadrature)
            den = 1 - t * diag
            with np.errstate(divide="ignore", invalid="ignore"):
                S_new = np.where(den > 0, (t * (J - diag * S_old) + e * B0) / den, plain)
            seen["diag_min"], seen["diag_max"] = min(seen["diag_min"], diag.min()), max(seen["diag_max"], diag.max())
            seen["den_min"] = min(seen["den_min"], den.min())
            seen["fallback"] += int((~(den > 0)).sum())
        else:
            S_new = plain
        seen["S_min"] = min(seen["S_min"], S_new.min())
        diff = float(np.abs(1 - S_old / S_new).max())
        R = orc.calculate_R(case.lam, case.blocks, J, case.planck2, case.lambda0, case.c0, case.doppler, gamma,
                            case.sigma_bb_const, case.sigma_bf1, case.sigma_bf2, case.temperature, case.lte,
                            case.hc_over_kB, case.pref_ij, case.pref_ji)
        pops = orc.revised_populations(R, case.C, case.atom_density)
        hist.append(diff)
        i += 1
    return J, S_new, pops, hist, seen


@functools.lru_cache(maxsize=None)
def first_iterate_reference():
    """the per-angle α of the loop's first iterate on line_case_644 (LTE populations) and its unit response; computed once,
    read-only"""
    z, x, y, case = line_case_644()
    _, alpha = oracle_alpha(case, case.lte, QUAD)
    ref = line_unit_response(alpha, z, x, y)
    alpha.setflags(write=False)
    ref.setflags(write=False)
    return alpha, ref


@functools.lru_cache(maxsize=None)
def oracle_loops():
    """line_case_644 and its hard variant, each through the plain and the ALI oracle loop to TARGET; computed once"""
    z, x, y, standard = line_case_644()
    out = {}
    for name, case in (("standard", standard), ("hard", hard_case(standard))):
        cap = max(COUNTS[name]) + 50
        out[name] = {"case": case, "plain": oracle_regular_line_loop(case, z, x, y, cap, TARGET),
                     "ali": oracle_regular_line_loop(case, z, x, y, cap, TARGET, ali=True)}
    return out


# ---- 1: symbols ------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_regular_line_ali_symbols_declared_exported_and_bound():
    text, code = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert hasattr(vrt, "line_lambda_diagonal_regular")
    assert inspect.signature(vrt.Lambda_regular).parameters["operator"].default is None
    # the entries are documented in a block of their own after vrt_lambda_get_operator, which names the session
    block = text[text.index("int vrt_lambda_get_operator("):text.index("int vrt_regular_line_lambda_diagonal_dev(")]
    assert "regular-grid line session" in " ".join(block.replace("*", " ").split())
    assert not re.search(r"vrt_regular_lambda_(set|select)_operator", code)


def test_regular_line_ali_prototypes_agree_with_the_header():
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
            elif re.fullmatch(r"int64_t \*\w+", a):
                want = _lib.p_i64
            elif re.fullmatch(r"(const )?double \*d_\w+", a):             # device arrays
                want = ctypes.c_void_p
            elif re.fullmatch(r"(const )?double \*\w+", a):
                want = _lib.p_dbl
            else:                                                          # handles, the stream
                assert re.fullmatch(r"(const )?(vrt_regular|vrt_regular_lambda|void) \*\w+", a), (name, a)
                want = ctypes.c_void_p
            assert b is want, (name, a, b)


def test_lambda_regular_refuses_an_unknown_operator_before_any_device_work():
    with pytest.raises(ValueError, match="operator must be None or 'diagonal'"):
        vrt.Lambda_regular(1e-3, 3, None, None, None, None, QUAD, operator="jacobi")


# ---- 2: argument checks ------------------------------------------------------------------------------------------------------
def test_regular_line_ali_refuses_bad_arguments_without_a_device():
    """NULL pointers, nlam < 1, ld < nlam, the direction checks, an operator other than 0 or 1: VRT_EINVAL in a child process
    that sees no device (the handles are never dereferenced).  The host form's check of α needs the point count, that is a
    real handle: tests/test_regular_line_ali.py makes that check on one."""
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
dev = lambda r=fake, na=1, k_=d(k), di=pi(dirs), wt=d(w), nlam=1, a=fake, o=fake: \
    L.vrt_regular_line_lambda_diagonal_dev(r, na, k_, di, wt, nlam, a, o, None)
host = lambda r=fake, na=1, k_=d(k), di=pi(dirs), wt=d(w), nlam=1, ld=1, a=d(v), o=d(v): \
    L.vrt_regular_line_lambda_diagonal(r, na, k_, di, wt, nlam, ld, a, o)
flat = np.array([0.0, 1.0, 0.0]); two = np.array([2], dtype=np.int32)
rc = []
for f in (dev, host):
    rc += [f(r=None), f(k_=None), f(di=None), f(wt=None), f(a=None), f(o=None), f(nlam=0), f(nlam=-1),
           f(na=0), f(k_=d(1.1 * k)), f(k_=d(flat)), f(di=pi(two))]
rc += [host(nlam=2, ld=1)]
rc += [L.vrt_regular_lambda_use_operator(None, 0), L.vrt_regular_lambda_use_operator(None, 1),
       L.vrt_regular_lambda_use_operator(fake, 2), L.vrt_regular_lambda_use_operator(fake, -1)]
rc += [L.vrt_regular_lambda_get_operator(None, ctypes.byref(op), None), L.vrt_regular_lambda_get_operator(fake, None, None)]
print(" ".join(str(r) for r in rc))
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    codes = r.stdout.split()
    assert len(codes) == 31 and all(int(c) == _lib.VRT_EINVAL for c in codes), r.stdout


# ---- 3: the reference ----------------------------------------------------------------------------------------------------------
def test_the_case_covers_all_six_plane_kinds():
    z, x, y, case = line_case_644()
    assert (z.size, x.size, y.size) == (6, 6, 6) and case.B0.shape == (216, 9)
    kinds = cut_kinds(z, x, y, QUAD)
    assert kinds[True] == {1, 2, 3} and kinds[False] == {1, 2, 3}, kinds


def test_line_unit_response_is_a_local_operator():
    """0 on the ghost border, >= 0 and < 1 everywhere, > 0 off the two boundary planes"""
    z, x, y, _ = line_case_644()
    _, ref = first_iterate_reference()
    ghost = ghost_mask(z, x, y)
    assert np.isfinite(ref).all() and (ref[ghost] == 0.0).all()
    assert (ref >= 0).all() and (ref < 1).all()
    inner = ref.reshape(y.size, x.size, z.size, -1)[1:-1, 1:-1, 1:-1]
    assert (inner > 0).all()
    print(f"first iterate: Λ* max {ref.max():.4g}, interior mean {ref[~ghost].mean():.4g}")


def test_line_unit_response_with_zero_velocity_is_the_continuum_unit_response():
    """every angle then reads the same α, and the per-angle reference is test_regular_ali_host.unit_response of it"""
    z, x, y, case = line_case_644()
    still = still_case(case)
    _, alpha = oracle_alpha(still, still.lte, QUAD)
    assert all(np.array_equal(alpha[a], alpha[0]) for a in range(1, alpha.shape[0]))
    two = alpha[:, :, [0, 2]]                               # a wing and the line centre
    assert np.array_equal(line_unit_response(two, z, x, y), unit_response(two[0], z, x, y, QUAD))
    # with the case's velocities the angles differ, and so does the operator
    moving = first_iterate_reference()[0]
    assert not np.array_equal(moving[0], moving[1])


# ---- 4: the oracle-driven loops ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["standard", "hard"])
@pytest.mark.parametrize("form", ["plain", "ali"])
def test_oracle_regular_line_loops_are_well_posed(name, form):
    run = oracle_loops()[name]
    case, (J, S, pops, hist, seen) = run["case"], run[form]
    print(f"{name} {form}: {len(hist)} iterates to {TARGET:g}; Λ* max {seen['diag_max']:.6g}, min den {seen['den_min']:.3g}, "
          f"{seen['fallback']} fallback entries, min S {seen['S_min']:.3g}")
    assert seen["S_min"] > 0 and np.isfinite(J).all() and np.isfinite(S).all()
    assert (pops > 0).all() and np.allclose(pops.sum(axis=0), case.atom_density, rtol=1e-12)
    assert hist[-1] <= TARGET
    if form == "ali":
        assert 0 <= seen["diag_min"] and seen["diag_max"] < 1
        assert seen["den_min"] > 0 and seen["fallback"] == 0


@pytest.mark.parametrize("name", ["standard", "hard"])
def test_oracle_regular_line_ali_needs_fewer_iterates_and_the_counts_stand(name):
    run = oracle_loops()[name]
    n_plain, n_ali = len(run["plain"][3]), len(run["ali"][3])
    print(f"{name}: plain {n_plain} iterates, ALI {n_ali} to {TARGET:g}")
    assert n_ali < n_plain
    assert abs(n_plain - COUNTS[name][0]) <= MARGIN and abs(n_ali - COUNTS[name][1]) <= MARGIN


@pytest.mark.parametrize("name", ["standard", "hard"])
def test_oracle_regular_plain_and_ali_loops_end_at_one_fixed_point(name):
    run = oracle_loops()[name]
    _, S0, _, h0, _ = run["plain"]
    _, S1, _, h1, _ = run["ali"]
    bound = fixed_point_bound(h0, h1)
    dist = np.abs(S1 / S0 - 1).max()
    print(f"{name}: |S_ali / S_plain - 1| = {dist:.3g}, bound {bound:.3g}")
    assert dist < bound
