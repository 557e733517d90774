"""Accelerated Λ-iteration of the LINE session with the diagonal operator Λ* formed from every iterate's per-angle α, host
side (no GPU): the entry points are declared, exported and bound, their argument checks answer VRT_EINVAL before a device
is touched, and the ALI loop driven by the oracle alone -- test_physics._oracle_lambda_iteration's body with Λ* restated
in numpy (test_ali_host.lambda_star_ref, one angle at a time) and the ALI update -- is well posed, ends at the fixed point
of the plain loop and needs fewer iterates where ε is small.  `oracle_line_loop`, `hard_case` and the iterate counts
measured here are the reference of tests/test_line_ali.py."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import _lib
from test_ali_host import lambda_star_ref, oracle_table
from test_physics import _lambda_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD = "ul7n12.dat"
NEW = ("vrt_line_lambda_diagonal_dev", "vrt_lambda_ali_update_dev", "vrt_lambda_ali_update_native_dev",
       "vrt_lambda_use_operator", "vrt_lambda_get_operator")
TARGET = 1e-3               # the tolerance both loops of the iterate-count comparison run to
# iterates of the oracle loops on voro_small to TARGET, measured by this file: standard case plain / ALI, hard
# variant plain / ALI.  The caps the tests apply are these counts plus a margin of two iterates.
COUNTS = {"standard": (31, 23), "hard": (351, 142)}
MARGIN = 2
# δ / (1 - ρ) of those four oracle runs (fixed_point_bound, one term per run): how far from its fixed point a run that
# stopped at TARGET can be.  tests/test_line_ali.py bounds the distance between two device runs by the sum of their terms;
# test_oracle_plain_and_ali_loops_end_at_one_fixed_point keeps these constants to what the oracle runs give.
BOUND_TERMS = {"standard": (5.05e-3, 3.59e-3), "hard": (9.24e-2, 2.55e-2)}


# ---- the numpy restatement ------------------------------------------------------------------------------------------------
def line_lambda_star_ref(so, table, alpha, w):
    """Λ* of the line loop: Σ_a lambda_star_ref(so, the table of angle a alone, alpha[a], w), added in angle order.
    alpha (n_angles, n, nlam), one α per angle."""
    diag = np.zeros_like(alpha[0])
    for a in range(len(table)):
        only = [entry if b == a else None for b, entry in enumerate(table)]
        diag = diag + lambda_star_ref(so, only, alpha[a], w)
    return diag


def hard_case(case):
    """the case with ε × 1e-2 and strength_const × 10: the regime where plain Λ-iteration crawls"""
    kw = {k: getattr(case, k) for k in vrt.LineCase.FIELDS}
    kw["eps"] = np.asarray(case.eps) * 1e-2
    kw["strength_const"] = case.strength_const * 10.0
    return vrt.LineCase(**kw)


def oracle_alpha(case, pops, quadrature=QUAD):
    """γ and the per-angle α_tot (n_angles, n, nlam) of the populations, as the loop forms them"""
    _, th, ph, nq = vrt.read_quadrature(quadrature)
    gamma, strength = orc.line_terms(case.gamma_static, case.gamma_unsold, pops, case.strength_const, case.Bij, case.Bji)
    alpha = np.stack([orc.line_opacity(orc.direction(th[a], ph[a]), case.lam, case.lambda0, case.c0, case.velocity,
                                       case.doppler, gamma, strength, case.alpha_cont) for a in range(nq)])
    return gamma, alpha


def oracle_line_loop(case, so, table, maxiter, eps_conv=0.0, ali=False, S0=None, pops0=None, quadrature=QUAD, ng=None):
    """test_physics._oracle_lambda_iteration's body; ali: with Λ* of this iterate's α and, t = 1 - ε, the update
    S_new = (t (J - Λ* S_old) + ε B0) / (1 - t Λ*) in the operation order of test_ali_host.oracle_ali_loop (where the
    denominator is not > 0 the entry takes the plain update).  Returns J, S, populations, the history and a dict of what the
    iterates saw: the range of Λ*, the smallest denominator, the entries that fell back, the smallest S."""
    w, th, ph, nq = vrt.read_quadrature(quadrature)
    pops = case.lte.copy() if pops0 is None else np.array(pops0, dtype=np.float64)
    S_new = case.B0.copy() if S0 is None else np.array(S0, dtype=np.float64)
    bottom = so.perm_up[: so.layers_up[1] - 1] - 1
    e = np.asarray(case.eps)[:, None]
    t = 1 - e
    seen = {"diag_min": np.inf, "diag_max": -np.inf, "den_min": np.inf, "fallback": 0, "S_min": np.inf}
    hist, diff, i, J = [], np.inf, 0, np.zeros_like(case.B0)
    while diff > eps_conv and i < maxiter:
        S_old = S_new.copy()
        gamma, alpha = oracle_alpha(case, pops, quadrature)
        J = orc.J_voronoi(w, th, ph, S_old, alpha, so, I0_up=case.B0[bottom], nthreads=8)
        plain = (1 - e) * J + e * case.B0
        if ali:
            diag = line_lambda_star_ref(so, table, alpha, w)
            den = 1 - t * diag
            with np.errstate(divide="ignore", invalid="ignore"):
                S_new = np.where(den > 0, (t * (J - diag * S_old) + e * case.B0) / den, plain)
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


def fixed_point_bound(*histories):
    """Σ over the runs of δ / (1 - ρ): a linearly converging run whose last change is δ and whose contraction is ρ is
    within δ ρ / (1 - ρ) < δ / (1 - ρ) of its fixed point (the tail of the geometric series); ρ is read off the last
    three entries of the run's own history, the larger of the two ratios."""
    return sum(fixed_point_term(h) for h in histories)


def fixed_point_term(h):
    rho = max(h[-1] / h[-2], h[-2] / h[-3])
    assert rho < 1, h[-3:]
    return h[-1] / (1 - rho)


# ---- 1: symbols ------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_line_ali_symbols_declared_exported_and_bound():
    text, code = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    for name in ("line_lambda_diagonal", "lambda_ali_update_dev", "lambda_ali_update_native_dev"):
        assert hasattr(vrt, name), name
    for fn in (vrt.Lambda_voronoi, vrt.Lambda_voronoi_host):
        assert inspect.signature(fn).parameters["operator"].default is None
    assert hasattr(vrt.FormalPlan, "line_lambda_diagonal_dev")
    # what stays out of scope is said next to the entries, and no such entry exists
    assert "Out of scope: the float-storage, the multi-device and the regular-grid line sessions" in text
    assert not re.search(r"vrt_(regular_lambda|multi\w*)_(set|select)_operator", code)
    from voronoirt_amd import build
    assert "vrt_line_ali.hip" in build.SOURCES


def test_line_ali_prototypes_agree_with_the_header():
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
            elif re.fullmatch(r"int \*\w+", a):
                want = _lib.p_int
            elif re.fullmatch(r"int64_t \*\w+", a):
                want = _lib.p_i64
            elif re.fullmatch(r"(const )?double \*(weights_host|max_rel_change)", a):
                want = _lib.p_dbl
            else:                                   # device arrays, handles, the stream
                assert re.fullmatch(r"(const )?(double|void|vrt_plan|vrt_grid|vrt_lambda) \*\w+", a), (name, a)
                want = ctypes.c_void_p
            assert b is want, (name, a, b)


def test_line_ali_python_refuses_before_any_device_work():
    """storage="f32" with the operator, and an unknown operator: ValueError before a site handle is even looked at"""
    for fn, kw in ((vrt.Lambda_voronoi_host, {}), (vrt.Lambda_voronoi, {"native": True})):
        with pytest.raises(ValueError, match="operator"):
            fn(1e-3, 3, None, None, QUAD, storage="f32", operator="diagonal", **kw)
        with pytest.raises(ValueError, match="operator"):
            fn(1e-3, 3, None, None, QUAD, operator="jacobi", **kw)


# ---- 2: argument checks ------------------------------------------------------------------------------------------------------
def test_line_ali_refuses_bad_arguments_without_a_device():
    """NULL pointers, nlam < 1, ld < nlam, an operator other than 0 or 1: VRT_EINVAL in a child process that sees no device
    (the handles are never dereferenced).  The checks that need a real handle -- a plan with a θ = 90 angle, a float-storage
    session -- are made on one in tests/test_line_ali.py."""
    script = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from voronoirt_amd import _lib
L = _lib.load()
w = np.ones(12)
wd = w.ctypes.data_as(_lib.p_dbl)
fake = ctypes.c_void_p(16)
out, cnt, op = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int()
rc = []
diag = lambda p=fake, nlam=1, a=fake, wt=wd, ld=1, o=fake: L.vrt_line_lambda_diagonal_dev(p, nlam, a, wt, ld, o, None)
rc += [diag(p=None), diag(a=None), diag(wt=None), diag(o=None), diag(nlam=0), diag(nlam=-1), diag(nlam=2, ld=1)]
upd = lambda g=fake, nlam=1, ld=1, J=fake, B=fake, e=fake, dg=fake, So=fake, Sn=fake, o=ctypes.byref(out), c=ctypes.byref(cnt): \
    L.vrt_lambda_ali_update_dev(g, nlam, ld, J, B, e, dg, So, Sn, o, c, None)
rc += [upd(g=None), upd(J=None), upd(B=None), upd(e=None), upd(dg=None), upd(So=None), upd(Sn=None), upd(o=None), upd(c=None),
       upd(nlam=0), upd(nlam=2, ld=1)]
nat = lambda g=fake, nlam=1, Ju=fake, Jd=fake, B=fake, e=fake, dg=fake, Su=fake, Sd=fake, o=ctypes.byref(out), c=ctypes.byref(cnt): \
    L.vrt_lambda_ali_update_native_dev(g, nlam, Ju, Jd, B, e, dg, Su, Sd, o, c, None)
rc += [nat(g=None), nat(Ju=None, Jd=None), nat(B=None), nat(e=None), nat(dg=None), nat(Su=None), nat(Sd=None), nat(o=None),
       nat(c=None), nat(nlam=0)]
rc += [L.vrt_lambda_use_operator(None, 0), L.vrt_lambda_use_operator(None, 1), L.vrt_lambda_use_operator(fake, 2),
       L.vrt_lambda_use_operator(fake, -1)]
rc += [L.vrt_lambda_get_operator(None, ctypes.byref(op), None), L.vrt_lambda_get_operator(fake, None, None)]
print(" ".join(str(r) for r in rc))
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    codes = r.stdout.split()
    assert len(codes) == 34 and all(int(c) == _lib.VRT_EINVAL for c in codes), r.stdout


# ---- 3: the oracle-driven line ALI loop -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loops(voro_small):
    """voro_small (1500 sites, 33 wavelengths, ul7n12): the standard _lambda_case and its hard variant, each through the
    plain and the ALI oracle loop to TARGET; computed once"""
    pos, nbr, bounds = voro_small
    so = orc.make_sites(pos, nbr, bounds)
    table, _ = oracle_table(so, QUAD)
    standard = _lambda_case(pos, bounds, 11)
    out = {"so": so}
    for name, case in (("standard", standard), ("hard", hard_case(standard))):
        cap = max(COUNTS[name]) + 50
        out[name] = {"case": case, "plain": oracle_line_loop(case, so, table, cap, TARGET),
                     "ali": oracle_line_loop(case, so, table, cap, TARGET, ali=True)}
    return out


@pytest.mark.parametrize("name", ["standard", "hard"])
def test_oracle_line_ali_loop_is_well_posed(loops, name):
    case, (J, S, pops, hist, seen) = loops[name]["case"], loops[name]["ali"]
    print(f"{name}: Λ* in [{seen['diag_min']:.3g}, {seen['diag_max']:.6g}], min den {seen['den_min']:.3g}, "
          f"{seen['fallback']} fallback entries, min S {seen['S_min']:.3g}, {len(hist)} iterates to {TARGET:g}")
    assert 0 <= seen["diag_min"] and seen["diag_max"] < 1
    assert seen["den_min"] > 0 and seen["fallback"] == 0
    assert seen["S_min"] > 0 and np.isfinite(J).all() and np.isfinite(S).all()
    assert (pops > 0).all() and np.allclose(pops.sum(axis=0), case.atom_density, rtol=1e-12)
    assert hist[-1] <= TARGET


@pytest.mark.parametrize("name", ["standard", "hard"])
def test_oracle_plain_and_ali_loops_end_at_one_fixed_point(loops, name):
    _, S0, _, h0, _ = loops[name]["plain"]
    _, S1, _, h1, _ = loops[name]["ali"]
    bound = fixed_point_bound(h0, h1)
    dist = np.abs(S1 / S0 - 1).max()
    print(f"{name}: plain {len(h0)} iterates, ALI {len(h1)} to {TARGET:g}; |S_ali / S_plain - 1| = {dist:.3g}, bound {bound:.3g}")
    assert h0[-1] <= TARGET and h1[-1] <= TARGET
    assert dist < bound
    for h, const in zip((h0, h1), BOUND_TERMS[name]):            # the constants are these runs' terms, rounded up
        assert fixed_point_term(h) <= const <= 1.01 * fixed_point_term(h)


def test_oracle_line_ali_needs_fewer_iterates_on_the_hard_variant(loops):
    """the counts measured here stand in COUNTS (and in DESIGN §7n); asserted: fewer, and within the cap"""
    n_plain, n_ali = len(loops["hard"]["plain"][3]), len(loops["hard"]["ali"][3])
    print(f"hard variant to {TARGET:g}: plain {n_plain} iterates, ALI {n_ali}; "
          f"standard: plain {len(loops['standard']['plain'][3])}, ALI {len(loops['standard']['ali'][3])}")
    assert n_ali < n_plain
    assert n_ali <= COUNTS["hard"][1] + MARGIN
    assert len(loops["standard"]["ali"][3]) <= COUNTS["standard"][1] + MARGIN
