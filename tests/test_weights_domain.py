"""Every device copy of linear_weights (voronoirt_amd/csrc/vrt_weights.h), its two exponentials and the wave-uniform
branch dispatch of the patch kernels, judged PER COEFFICIENT against a 40-digit evaluation of the reference's
three-branch formula (oracle/weights_ref.py) over the whole Δτ domain -- not through J at 1e-10 after a sweep.
The copies are called directly through tests/probes/weights_probe.hip (voronoirt_amd/build.py: build_probe).

CPU part (-m "not gpu"): the references themselves -- orc.linear_weights and pyref.linear_weights against the
formula; their measured maxima per decade are the yardstick E_oracle printed beside the device's.
GPU part (-m gpu): exponentials, weights, branch edges, special values, agreement of the MODEs, lane independence.

ERROR BUDGETS (derived here, not tuned; u = 2^-53 = 1.11e-16 is the unit roundoff, "exact" the 40-digit value)

 exp_neg (5e-4 <= x <= 50; 13 Horner steps on |r| <= ln2/2 = 0.3466):  E = 2.5 u
   * reduction: k ln2_hi is exact (ln2_hi has 32 trailing zero bits, |k| <= 73) and so is t - k ln2_hi (a multiple of
     2^-54 below 0.5); the second fma rounds once: |δr| <= 0.35 u, which is the relative error of exp(r);
   * remainder r^14/14! relative to exp(r) >= 0.707:  < 4e-18 = 0.04 u (the source's figure);
   * Horner: the last fma rounds p in [0.707, 1.414] -> <= u relative; the one before errs by <= u, carried by
     |r| -> 0.35 u; the earlier ones by <= (u/2) r^2 + (u/8) r^3 + ... < 0.07 u; the rounded coefficients 1/6, 1/24, ...
     by < 0.01 u; together 0.43 u absolute, 0.61 u relative to p >= 0.707;   ldexp is exact (no subnormal result).
   Sum 0.35 + 0.04 + 1 + 0.61 = 2.0 u; budget 2.5 u.
 exp_neg_tab (0 <= x <= 745; degree 5 on |r| <= ln2/64 = 0.01083, 32-entry table):  E = 2.3e-15 + 3.1 u = 2.64e-15
   * remainder r^6/720 (1 + r/7 + ...) / exp(r) <= 2.27e-15 at |r| = ln2/64: the source's "< 2.3e-15";
     for x <= ln2/64 the reduction has N = 0 and r = -x, so there the remainder is x^6/720 * 1.02: negligible below 5e-3;
   * reduction: N hi exact (hi has 29 bits, |N| <= 34394), second fma |δr| <= 0.011 u;
   * Horner: last fma <= u, the earlier ones 0.011 u;  table entry rounded: u;  product p T[j]: u;
     ldexp exact for normal results; a subnormal result is rounded to the grid of 2^-1074 once more: <= 1 unit absolute.
   Sum of the roundings 3.03 u; budget 3.1 u.
 libm exp of the reference-order copy: 1 ulp = 2 u (the documented bound of the device library and of glibc).

 reciprocals:  IEEE division (reference order)                 ε = u
               v_rcp_f64 + 2 Newton steps (lin_weights)        ε = 2.1 u  (each step squares the error and rounds once: u + ε1²;
                                                                           plus u for the unfused product (1 - e) rc)
               v_rcp_f64 + 1 Newton step (lin_weights_fma)     ε = 1e-14  (the source's own statement, vrt_weights.h)

 weights, absolute error against the formula, REST = 2.1 u of the result for the two or three remaining roundings:
   Taylor branch (Δτ < 5e-4, negative values included), every coefficient x:   REST |x| + 2^-1074
       (e: 1 - Δτ and the final sum round near 1: 2 u; a, b: Δτ/3 or the constant 1/3, the difference near 1/2 and the
        product: 2.001 u of the result; results below 2^-1022 land on the subnormal grid)
   exponential branch:  e:  E e
       a = (1 - e)/Δτ - e:   E e (1/Δτ + 1)  +  (u/2)/Δτ [1 - e rounds near 1]  +  ε (1 - e)/Δτ  +  REST |a|
       b = (1 - a) - e:      E e / Δτ        +  (u/2)/Δτ                        +  ε (1 - e)/Δτ  +  REST |a| + u/2 + REST |b|
     Both are ill-conditioned towards 5e-4: (u/2)/Δτ against a = Δτ/2 is u/Δτ² = 4.4e-10 relative AT the edge in EVERY copy,
     the fp64 oracle included; an exponential at E instead of u costs E/Δτ² on top.
   thick branch (Δτ > 50):  e = 0 exactly;  a: (ε + REST) |a| + 2 units of 2^-1074;  b: that + u/2.

OBSERVED on MI355X (max relative error against the formula per decade of Δτ, coefficient a / b / e; "oracle" is
orc.linear_weights on the CPU, the yardstick E_oracle; pyref gives the same figures):

  Δτ decade      oracle (CPU)              reference order           lin_weights               lin_weights_fma<2>
  <= 1e-5    1.6e-16 1.6e-16 1.1e-16   (the same)                (the same)                1.6e-16 1.6e-16 5.6e-17
  1e-4       4.2e-10 4.1e-10 1.0e-16   4.2e-10 4.1e-10 1.0e-16   4.2e-10 4.1e-10 1.0e-16   4.2e-10 4.1e-10 5.6e-17   <- above 5e-4: (u/2)/Δτ
  1e-3       1.1e-10 1.1e-10 5.6e-17   1.1e-10 1.1e-10 5.6e-17   1.1e-10 1.1e-10 5.6e-17   1.1e-10 1.1e-10 1.4e-15
  1e-2       1.1e-12 1.1e-12 6.1e-17   1.1e-12 1.1e-12 6.9e-17   1.1e-12 1.1e-12 6.4e-17   4.0e-11 4.0e-11 2.4e-15   <- r^6/720 of the table exp / Δτ²
  1e-1       1.3e-14 1.2e-14 1.1e-16   1.5e-14 1.3e-14 1.3e-16   1.4e-14 1.2e-14 1.2e-16   3.4e-13 2.9e-13 2.4e-15
  1e+0       5.6e-16 4.9e-16 1.1e-16   7.1e-16 5.5e-16 1.3e-16   5.8e-16 4.9e-16 1.3e-16   5.7e-15 2.2e-15 2.4e-15
  1e+1       2.6e-16 1.3e-16 1.1e-16   2.6e-16 1.3e-16 1.3e-16   3.7e-16 1.2e-16 1.3e-16   1.8e-15 2.1e-16 2.4e-15
  > 50       1.1e-16 5.7e-17 0         1.1e-16 5.7e-17 0         1.1e-16 5.7e-17 0         2.0e-15 5.7e-17 0         <- one Newton step
 lin_weights_fma<0> and <1> equal <2> wherever they may be called (bit for bit: test_modes_of_lin_weights_fma_agree_bitwise).
 exp_neg: 1.20 u (bound 2.5 u).  exp_neg_tab: 2.44e-15 on normal results (bound 2.64e-15), 0.68 u on 5e-4 … 5e-3, subnormal
 results up to 9 units of 2^-1074 (the relative bound at the top of the subnormal range is 12 units).
 v_rcp_f64 + one Newton step: 2.0e-15, i.e. the instruction itself is good to ~2^-24.5; the source's 1e-14 holds.

THE THREE PREDICTIONS of the issue this module answers, as found on the device BEFORE the fixes in vrt_weights.h:
 1. confirmed: lin_weights_fma<1>/<2> differed from <0> in a at every thick point from Δτ = 5.24e5 upwards (17 210 of 25 006
    thick points), a = -1.9e-22 at DBL_MAX.  It did not reach J or I (the deep end-to-end case was bitwise equal before the fix
    too: the difference is <= 1.9e-22 S against I of order 1).  Fixed by setting the exponential itself to 0 on thick lanes.
 2. confirmed: Δτ = +∞ gave NaN in lin_weights and lin_weights_fma (the steps, tiles and all patch forms failed
    test_non_finite_opacity_…, the level path passed); a NaN Δτ left e finite (0.9995 in lin_weights, exp(-50) or 0 in
    lin_weights_fma).  Fixed: fmin on the Newton residual, NaN sent down the Taylor select.
 3. confirmed: exp_neg_tab is at rounding level (0.68 u) where the weights amplify it most; the amplified remainder shows
    one decade higher (4e-11 in a at Δτ ~ 0.01-0.02, inside the derived budget, below the 1e-10 contract).
 Cost of the fixes on the headline benchmark step (parent / branch library alternating on one MI355X, ms per step):
 parent 6.929 6.930 6.835, branch 6.975 6.891 6.895: +0.3 % in the mean, the parent's own spread is 1.4 %.
 The GPU tests of this module take 10 s of a 259 s `pytest -m gpu` run.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import pyref
from oracle import weights_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -53
UNIT = 5e-324                       # 2^-1074
REST = 2.1 * U
E_LIBM = 2.0 * U
E_EXP_NEG = 2.5 * U
E_TAB_ROUND = 3.1 * U
E_TAB = 2.3e-15 + E_TAB_ROUND
LN2_64 = math.log(2.0) / 64


def e_tab(x):
    """exp_neg_tab's bound at argument x: below ln2/64 the reduction has N = 0, r = -x and the remainder is x^6/720."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        small = np.minimum(np.abs(x), LN2_64) ** 6 / 720 * 1.02
    return np.where(np.abs(x) <= LN2_64, small, 2.3e-15) + E_TAB_ROUND


#               name                      probe id   exponential's bound           reciprocal
COPIES = {
    "linear_weights_ref_order": dict(which=0, E=lambda x: E_LIBM + 0 * x, eps=U),
    "lin_weights":              dict(which=1, E=lambda x: E_EXP_NEG + 0 * x, eps=2.1 * U),
    "lin_weights_fma<0>":       dict(which=2, E=e_tab, eps=1e-14),
    "lin_weights_fma<1>":       dict(which=3, E=e_tab, eps=1e-14),
    "lin_weights_fma<2>":       dict(which=4, E=e_tab, eps=1e-14),
}
HOST = dict(E=lambda x: E_LIBM + 0 * x, eps=U)          # orc / pyref: glibc exp, IEEE division


def budgets(dtau, ref, E, eps):
    """Absolute error budgets (B_a, B_b, B_e) of the module docstring at the finite points dtau; ref = the formula's
    (a, b, e) as fp64 (their leading parts)."""
    d = np.asarray(dtau, dtype=np.float64)
    a, b, e = (np.abs(r) for r in ref)
    thin, thick = d < W.THIN, d > W.THICK
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Ee = E(d) * e
        common = (U / 2) / d + eps * (1 - e) / d + REST * a
        Ba = np.where(thin, REST * a + UNIT, np.where(thick, (eps + REST) * a + 2 * UNIT, Ee * (1 / d + 1) + common))
        Bb = np.where(thin, REST * b + UNIT, np.where(thick, (eps + REST) * a + 2 * UNIT + U / 2,
                                                      Ee / d + common + U / 2 + REST * b))
        Be = np.where(thin, REST * e + UNIT, np.where(thick, 0.0, Ee))
    return Ba, Bb, Be


def err(got, ref):
    """|got - (hi + lo)| formed in fp64: got - hi is exact for close values."""
    hi, lo = ref
    with np.errstate(invalid="ignore"):
        return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


@pytest.fixture(scope="module")
def points():
    x = W.point_set()
    fin = np.isfinite(x)
    return {"x": x, "fin": fin, "ref": W.formula_arrays(x)}


def decade_table(x, errs, ref):
    """max relative error of (a, b, e) per decade of Δτ (finite positive points): {decade: (ra, rb, re)}."""
    out = {}
    pos = (x > 0) & np.isfinite(x)
    dec = np.full(x.shape, -999, dtype=np.int64)
    dec[pos] = np.floor(np.log10(x[pos])).astype(np.int64)
    dec = np.clip(dec, -10, 13)                      # ... <= 1e-10 and >= 1e13 are one row each
    for k in sorted(set(dec[pos].tolist())):
        m = pos & (dec == k)
        row = []
        for g, (hi, _) in zip(errs, ref):
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(hi[m] != 0, g[m] / np.abs(hi[m]), np.where(g[m] == 0, 0.0, np.inf))
            row.append(float(np.nanmax(r)))
        out[k] = tuple(row)
    return out


def print_table(title, table):
    print(f"\n{title}")
    print("  decade      a          b          e")
    for k, (ra, rb, re_) in table.items():
        lab = "<=1e-10" if k == -10 else ">=1e13 " if k == 13 else f"1e{k:+03d}  "
        print(f"  {lab}  {ra:9.2e}  {rb:9.2e}  {re_:9.2e}")


def check_copy(name, x, got, ref, E, eps):
    """every finite point within its budget; returns the per-coefficient absolute errors"""
    fin = np.isfinite(x)
    errs = [err(g, r) for g, r in zip(got, ref)]
    B = budgets(x, [r[0] for r in ref], E, eps)
    for c, g, bud in zip("abe", errs, B):
        bad = fin & ~(g <= bud)
        if bad.any():
            i = int(np.flatnonzero(bad)[np.argmax((g / np.maximum(bud, UNIT))[bad])])
            raise AssertionError(f"{name}: {c} misses its budget at {int(bad.sum())} points; worst Δτ = {x[i]!r}: "
                                 f"error {g[i]:.3e}, budget {bud[i]:.3e}, got {got['abe'.index(c)][i]!r}")
    return errs


# ---- CPU: the references themselves ----------------------------------------------------------------------------------
def test_formula_reference_is_the_three_branch_formula():
    """weights_formula_mp at points whose value is known in closed form, and its distance from the integral."""
    a, b, e = W.weights_formula_mp(0.0)
    assert (a, b, e) == (0, 0, 1)
    assert W.weights_formula_mp(math.inf) == (0, 1, 0)
    assert all(math.isnan(float(v)) for v in W.weights_formula_mp(math.nan))
    a, b, e = W.weights_formula_mp(100.0)
    assert e == 0 and abs(a - W.MP.mpf(1) / 100) < 1e-38 and abs(b - W.MP.mpf(99) / 100) < 1e-38
    a, b, e = W.weights_formula_mp(1.0)
    assert abs(e - W.MP.exp(-1)) < 1e-38 and abs(a - (1 - 2 * W.MP.exp(-1))) < 1e-38 and abs(a + b + e - 1) < 1e-38
    x = W.MP.mpf(2.0 ** -12)
    a, b, e = W.weights_formula_mp(2.0 ** -12)
    assert a == x * (W.MP.mpf(1) / 2 - x / 3) and b == x * (W.MP.mpf(1) / 2 - x / 6) and e == 1 - x + x * x / 2
    # the branch follows the fp64 comparisons: 5e-4 and 50 themselves are on the exponential branch, negatives on Taylor's
    assert [W.branch(v) for v in (-1e-3, 0.0, math.nextafter(5e-4, 0), 5e-4, 50.0, math.nextafter(50.0, 99), math.inf)] \
        == [0, 0, 0, 1, 1, 2, 2]
    # how far the formula is from the integral it approximates (documented, orders only)
    below, above = math.nextafter(5e-4, 0), 5e-4
    fa, fb, fe = W.weights_formula_mp(below)
    ia, ib, ie = W.weights_integral_mp(below)
    rel_a = float(abs(fa - ia) / ia)
    print(f"\nformula vs integral just below 5e-4: a {rel_a:.2e} rel, b {float(abs(fb - ib) / ib):.2e} rel, e {float(abs(fe - ie)):.2e} abs")
    assert 3e-8 < rel_a < 1e-7                              # Δτ³/8 over Δτ/2 = Δτ²/4 = 6e-8
    assert 1e-11 < float(abs(fe - ie)) < 3e-11              # Δτ³/6 = 2e-11: the jump of e at the edge
    ja, _, je = W.weights_formula_mp(above)
    ka, _, ke = W.weights_integral_mp(above)
    assert abs(ja - ka) < 1e-36 and abs(je - ke) < 1e-38    # on the exponential branch the formula IS the integral
    ta, _, te = W.weights_formula_mp(math.nextafter(50.0, 99))
    ua, _, ue = W.weights_integral_mp(math.nextafter(50.0, 99))
    assert te == 0 and 1.9e-22 < float(ue) < 1.93e-22 and float(abs(ta - ua)) < 2e-22      # e dropped above 50


def test_host_references_against_the_formula(points):
    """orc.linear_weights (C) and pyref.linear_weights (Python) over the whole point set: within the budget of a
    reference-order evaluation (libm exp at 1 ulp, IEEE division), a + b + e = 1 to rounding, (0, 0, 1) at 0, NaN and +∞
    as the formula.  The printed maxima per decade are the yardstick E_oracle of the device tables."""
    x, ref = points["x"], points["ref"]
    for name, fn in (("orc.linear_weights", orc.linear_weights), ("pyref.linear_weights", pyref.linear_weights)):
        got = np.array([fn(float(d)) for d in x]).T           # rows a, b, e
        got = (got[0], got[1], got[2])
        errs = check_copy(name, x, got, ref, **HOST)
        print_table(f"{name}: max relative error against the formula", decade_table(x, errs, ref))
        i0 = int(np.flatnonzero(x == 0.0)[0])
        assert (got[0][i0], got[1][i0], got[2][i0]) == (0.0, 0.0, 1.0)
        inf = np.isposinf(x)
        assert (got[0][inf] == 0).all() and (got[1][inf] == 1).all() and (got[2][inf] == 0).all()
        nan = np.isnan(x)
        assert nan.any() and all(np.isnan(g[nan]).all() for g in got)
        # a + b + e = 1: exactly the roundings of b = 1 - a - e (thick, exponential) or of the three Taylor values
        fin = np.isfinite(x)
        s = got[0][fin] + got[1][fin] + got[2][fin]
        taylor = x[fin] < W.THIN
        assert np.abs(s[~taylor] - 1).max() <= 4 * U
        assert (np.abs(s[taylor] - 1) <= np.abs(x[fin][taylor]) ** 3 / 6 * 1.01 + 4 * U).all()     # the Taylor truncation


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    import torch
    from voronoirt_amd import build
    lib = ctypes.CDLL(build.build_probe())
    p, ll = ctypes.c_void_p, ctypes.c_longlong
    lib.probe_exp.argtypes = [ctypes.c_int, ll, p, p]
    lib.probe_weights.argtypes = [ctypes.c_int, ll, p, p, p, p]
    lib.probe_entry.argtypes = [ctypes.c_int, ll, p, p]
    dev = torch.device("cuda", 0)

    class Probe:
        def exp(self, which, x):
            xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
            out = torch.full_like(xd, float("nan"))
            torch.cuda.synchronize()
            assert lib.probe_exp(which, xd.numel(), xd.data_ptr(), out.data_ptr()) == 0
            return out.cpu().numpy()

        def weights(self, which, x):
            xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
            o = torch.full((3, xd.numel()), float("nan"), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            assert lib.probe_weights(which, xd.numel(), xd.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr()) == 0
            o = o.cpu().numpy()
            return o[0], o[1], o[2]

        def entry(self, which, rows):
            """rows: [11][n] (d1, d2, w1, w2, in1, in2, S_c, S_1, S_2, I_1, I_2), n a multiple of 64 -> [3][n] (c, g1, g2)"""
            rd = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64)).to(dev)
            n = rd.shape[1]
            assert rd.shape[0] == 11 and n % 64 == 0
            o = torch.full((3, n), float("nan"), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            assert lib.probe_entry(which, n, rd.data_ptr(), o.data_ptr()) == 0
            return o.cpu().numpy()

    return Probe()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.gpu
def test_exponentials_against_mpmath(probe):
    """exp_neg on 5e-4 … 50 and exp_neg_tab on 0 … 745 within the bounds their construction gives (module docstring);
    subnormal results of exp_neg_tab carry one more rounding to the grid of 2^-1074.  Where the weights amplify the
    exponential's error by 1/x (5e-4 <= x <= 5e-3) exp_neg_tab reduces with N = 0, r = -x and must be at rounding level:
    there the bound is 3.1 u + x^6/720, and the observed maximum is printed."""
    x = W.point_set()
    x = x[(x >= W.THIN) & (x <= W.THICK)]
    ref = W.split([W.exp_neg_mp(v) for v in x])
    rel = err(probe.exp(0, x), ref) / ref[0]
    print(f"\nexp_neg: max relative error {rel.max():.3e} = {rel.max() / U:.2f} u over {len(x)} points (bound {E_EXP_NEG / U} u)")
    assert rel.max() <= E_EXP_NEG
    xt = W.exp_tab_points()
    ref = W.split([W.exp_neg_mp(v) for v in xt])
    got = probe.exp(1, xt)
    g = err(got, ref)
    sub = ref[0] < np.finfo(np.float64).tiny
    bound = e_tab(xt) * ref[0] + np.where(sub, UNIT, 0.0)
    rel = g[~sub] / ref[0][~sub]
    small = (xt >= W.THIN) & (xt <= 5e-3)
    print(f"exp_neg_tab: max relative error (normal results) {rel.max():.3e} (bound {E_TAB:.3e}); "
          f"subnormal results: max {(g[sub] / UNIT).max():.2f} units of 2^-1074; "
          f"on 5e-4 … 5e-3: {(g[small] / ref[0][small]).max() / U:.2f} u over {int(small.sum())} points")
    bad = ~(g <= bound)
    assert not bad.any(), (xt[bad][:5], got[bad][:5], g[bad][:5], bound[bad][:5])
    assert got[xt == 0.0] == 1.0


@pytest.mark.gpu
def test_weights_of_every_copy(probe, points):
    """Each copy, each of a, b, e, at every point of the set against the formula, within the derived budget.  A copy is
    judged where it may be called: lin_weights_fma<0> off the exponential branch, <1> off the Taylor branch.  Prints the
    observed maxima per decade beside nothing else -- the oracle's are printed by test_host_references_against_the_formula."""
    x, ref = points["x"], points["ref"]
    br = np.array([W.branch(v) for v in x])
    for name, c in COPIES.items():
        legal = np.ones(len(x), dtype=bool)
        if name.endswith("<0>"):
            legal = (br != 1) | np.isnan(x)
        if name.endswith("<1>"):
            legal = (br != 0) & ~np.isnan(x)                  # a NaN lane counts as thin in the dispatch
        xs = x[legal]
        rs = tuple((hi[legal], lo[legal]) for hi, lo in ref)
        got = probe.weights(c["which"], xs)
        errs = check_copy(name, xs, got, rs, c["E"], c["eps"])
        print_table(f"{name}: max relative error against the formula", decade_table(xs, errs, rs))


@pytest.mark.gpu
def test_branch_edges_and_special_values(probe):
    """Within ±4 ulp of 5e-4 and of 50 every copy takes the branch the reference's fp64 comparison takes (read from e, where
    the two formulas differ by Δτ³/6 = 2e-11 at 5e-4 and by exp(-50) against exactly 0 at 50);  Δτ = 0 -> exactly (0, 0, 1);
    NaN -> NaN in all three;  +∞ -> exactly (0, 1, 0);  the largest finite values -> e = 0, b = 1 and a within budget."""
    edge = np.array(W._ulp_neighbours(5e-4) + W._ulp_neighbours(50.0))
    dmax = np.finfo(np.float64).max
    special = np.array([0.0, math.nan, math.inf, dmax, 1e308, 1.5e308])
    for name, c in COPIES.items():
        for x in (edge, special):
            keep = np.ones(len(x), dtype=bool)
            if name.endswith("<0>"):
                keep = np.array([W.branch(v) != 1 or math.isnan(v) for v in x])
            if name.endswith("<1>"):
                keep = np.array([W.branch(v) != 0 and not math.isnan(v) for v in x])
            xs = x[keep]
            a, b, e = probe.weights(c["which"], xs)
            for i, v in enumerate(xs):
                tag = (name, float(v).hex(), a[i], b[i], e[i])
                if math.isnan(v):
                    assert math.isnan(a[i]) and math.isnan(b[i]) and math.isnan(e[i]), tag
                    continue
                if v == 0.0:
                    assert (a[i], b[i], e[i]) == (0.0, 0.0, 1.0), tag
                    continue
                if math.isinf(v):
                    assert (a[i], b[i], e[i]) == (0.0, 1.0, 0.0), tag
                    continue
                want = W.branch(v)
                fa, fb, fe = W.weights_formula_mp(v)
                Ba, Bb, Be = budgets(np.array([v]), [np.array([float(t)]) for t in (fa, fb, fe)], c["E"], c["eps"])
                if want == 2:
                    assert e[i] == 0.0, tag                                   # exactly 0 <=> the thick branch
                else:
                    assert e[i] != 0.0 and abs(W.MP.mpf(e[i]) - fe) <= Be[0], tag
                    other = W.weights_formula_mp(v, force_branch=1 - want)[2] if v < 1 else None
                    if other is not None:                                     # near 5e-4: far from the other branch's e
                        assert abs(W.MP.mpf(e[i]) - other) > 1e-11, tag
                assert abs(W.MP.mpf(a[i]) - fa) <= Ba[0] and abs(W.MP.mpf(b[i]) - fb) <= Bb[0], tag
                if v >= 1e308:
                    assert b[i] == 1.0, tag


@pytest.mark.gpu
def test_modes_of_lin_weights_fma_agree_bitwise(probe, points):
    """The wave-uniform MODE changes which code a lane runs, never its result: thin lanes under <0> and <2>, thick lanes
    under <0>, <1> and <2> for every thick point up to DBL_MAX (and +∞), mid lanes under <1> and <2> -- bit for bit."""
    x = points["x"]
    br = np.array([W.branch(v) for v in x])
    nan = np.isnan(x)
    for sel, modes in ((br == 0, (2, 4)), ((br == 2) & ~nan, (2, 3, 4)), ((br == 1) & ~nan, (3, 4)), (nan, (2, 4))):
        xs = x[sel]
        assert len(xs)
        base = probe.weights(modes[0], xs)
        for m in modes[1:]:
            got = probe.weights(m, xs)
            for c, p, q in zip("abe", base, got):
                d = bits(p) != bits(q)
                if d.any():
                    i = int(np.flatnonzero(d)[np.argmax(xs[d])])
                    raise AssertionError(f"lin_weights_fma<{modes[0] - 2}> and <{m - 2}> differ in {c} at {int(d.sum())} of {len(xs)} "
                                         f"points, smallest Δτ {xs[d].min()!r}; at Δτ = {xs[i]!r}: {p[i]!r} vs {q[i]!r}")


def _lane_cases(rng):
    """(d1, d2) of the probe lanes: every pairing of the three branches, optical depths up to 1e15, both edges."""
    thin = [0.0, 1e-12, 3e-7, 4.9e-4, math.nextafter(5e-4, 0)]
    mid = [5e-4, 6e-4, 0.03, 1.0, 17.0, 50.0]
    thick = [math.nextafter(50.0, 99), 51.0, 3e3, 6e5, 1e8, 1e12, 1e15]
    out = []
    for A in (thin, mid, thick):
        for B in (thin, mid, thick):
            for _ in range(6):
                out.append((A[rng.integers(len(A))], B[rng.integers(len(B))]))
    out += [(v, v) for v in thin + mid + thick]
    return out


@pytest.mark.gpu
def test_dispatch_is_lane_independent(probe):
    """entry_lambda, entry_lambda_seq and late_lambda + late_apply choose MODE 0 / 1 / 2 from a ballot over the wave.  One
    lane's eleven inputs are held fixed (lane 17) while the other 63 lanes are all thin, all thick, thin + thick (MODE 0 for
    a thin or thick probe), mid + thick (MODE 1 unless the probe is thin), thick with a single thin or single mid lane at 0,
    31, 32 or 63, and thick with one thin AND one mid lane (MODE 2): its (c, g1, g2) must not change by a bit.  The sequential
    and the late form agree bitwise on every lane of every wave, and every form lies within the propagated budget of
    c = Σ_r w_r (e_r I_r + a_r S_r + b_r S_c), g_r = [in_r] e_r w_r formed from the 40-digit formula."""
    rng = np.random.default_rng(77)
    THIN_F, MID_F, THICK_F = 2e-5, 0.7, 4e3
    comps = [[THIN_F] * 64, [THICK_F] * 64, [THIN_F, THICK_F] * 32, [MID_F, THICK_F] * 32]
    for special in (THIN_F, MID_F):
        for lane in (0, 31, 32, 63):
            w = [THICK_F] * 64
            w[lane] = special
            comps.append(w)
    w = [THICK_F] * 64
    w[0], w[63] = THIN_F, MID_F
    comps.append(w)
    w = [THIN_F] * 64
    w[32] = MID_F
    comps.append(w)
    cases = _lane_cases(rng)
    PL = 17
    nc, nw = len(cases), len(comps)
    rows = np.empty((11, nc * nw * 64))
    filler = rng.random((11, 64))
    for ci, (d1, d2) in enumerate(cases):
        own = rng.random(11)
        own[0], own[1] = d1, d2
        own[4], own[5] = ci & 1, (ci >> 1) & 1
        own[6:9] += 1.0                                        # S in 1 … 2, I in 0 … 1, w in 0 … 1
        for wi, comp in enumerate(comps):
            blk = filler.copy()
            blk[0] = comp
            blk[1] = np.roll(comp, 2 * (wi % 2))               # the second upwind: the same kinds (an even shift keeps the alternations)
            blk[4:6] = np.round(blk[4:6])
            blk[:, PL] = own
            o = (ci * nw + wi) * 64
            rows[:, o:o + 64] = blk
    out = [probe.entry(which, rows) for which in range(3)]
    names = ("entry_lambda", "entry_lambda_seq", "late_lambda + late_apply")
    idx = (np.arange(nc)[:, None] * nw + np.arange(nw)[None, :]) * 64 + PL          # [case][composition]
    for name, o in zip(names, out):
        for k, lab in enumerate(("c", "g1", "g2")):
            v = bits(o[k])[idx]
            d = (v != v[:, :1]).any(axis=1)
            if d.any():
                ci = int(np.flatnonzero(d)[0])
                raise AssertionError(f"{name}: {lab} of a lane with Δτ = {cases[ci]} depends on its wave: "
                                     f"{[float(t) for t in o[k][idx[ci]]]} over the compositions; {int(d.sum())} of {nc} probe lanes differ")
    assert np.array_equal(bits(out[1]), bits(out[2])), "entry_lambda_seq and late_lambda + late_apply differ"
    # accuracy of every form at the probe lanes (composition 0), against the formula
    c_fma = COPIES["lin_weights_fma<2>"]
    for ci, (d1, d2) in enumerate(cases):
        r = rows[:, idx[ci, 0]]
        cref, cb, g = W.MP.mpf(0), 0.0, []
        for d, wq, inq, S_u, I_u in ((d1, r[2], r[4], r[7], r[9]), (d2, r[3], r[5], r[8], r[10])):
            fa, fb, fe = W.weights_formula_mp(d)
            Ba, Bb, Be = (float(t[0]) for t in budgets(np.array([d]), [np.array([float(t)]) for t in (fa, fb, fe)],
                                                        c_fma["E"], c_fma["eps"]))
            mag = float(fe) * I_u + float(fa) * S_u + float(fb) * r[6]
            cref += W.MP.mpf(wq) * (fe * W.MP.mpf(I_u) + fa * W.MP.mpf(S_u) + fb * W.MP.mpf(r[6]))
            cb += wq * (Be * I_u + Ba * S_u + Bb * r[6] + 4 * U * mag)           # product, two fmas, the weight
            g.append((fe * W.MP.mpf(wq) if inq else W.MP.mpf(0), Be * wq + U * float(fe) * wq))
        cb += U * float(abs(cref))                                             # the final sum
        for name, o in zip(names, out):
            got = o[:, idx[ci, 0]]
            assert abs(W.MP.mpf(got[0]) - cref) <= cb, (name, cases[ci], got[0], float(cref), cb)
            for k in (0, 1):
                assert abs(W.MP.mpf(got[1 + k]) - g[k][0]) <= g[k][1], (name, cases[ci], k, got[1 + k], float(g[k][0]))


# ---- end-to-end fields that reach every MODE ---------------------------------------------------------------------------
# tests/conftest.random_fields and test_patches._case draw α independently per site from 10**U(-3, 3): neighbouring lanes
# are uncorrelated, almost nothing is thin and MODE 0 (no lane on the exponential branch) never runs.  The fields below
# are stratified like an atmosphere, sit on a branch edge, or are deep enough for 1/Δτ to meet exp(-50).
RTOL = 1e-10


def _all_dtau(so, th, ph, alpha):
    """Δτ = r (α_c + α_u) / 2 of every (angle, site, upwind) with a valid upwind, from the oracle's tables (host only)."""
    import voronoirt_amd as vrt
    out = []
    for t, p in zip(th, ph):
        up, _, _, r, _ = orc.upwind_table(so, vrt.direction(t, p))
        ok = up > 0
        a_u = alpha[np.where(ok, up - 1, 0)]
        out.append(np.where(ok, r * (alpha[:, None] + a_u) / 2, np.nan))
    return np.stack(out)                                     # [angle][site][2]


def _median_r(so, th, ph):
    import voronoirt_amd as vrt
    up, _, _, r, _ = orc.upwind_table(so, vrt.direction(th[0], ph[0]))
    return float(np.median(r[up > 0]))


# log10 of the neighbour Δτ at the top and at the bottom of the box: the uniform bcc grid spreads 19 decades evenly over
# its layers; the density-stratified Voronoi grid (scale height 0.35 of the box) holds most of its sites near the bottom,
# so a steeper field is needed for a fifth of the (site, upwind) pairs to be thin.
STRATIFIED = {"bcc": (-10.0, 9.0), "voronoi": (-20.0, 8.5)}


def stratified_alpha(so, th, ph, seed, lg_top=-10.0, lg_bottom=9.0):
    """α = α0 exp(-z/H) (1 + 0.1 u): the neighbour Δτ runs from 10^lg_top at the top of the box to 10^lg_bottom at
    its bottom (z = bounds[0]), linearly in log Δτ."""
    rng = np.random.default_rng(seed)
    z = so.positions[:, 0]
    z0, z1 = so.bounds[0], so.bounds[1]
    lg = lg_bottom + (lg_top - lg_bottom) * (z - z0) / (z1 - z0)
    return 10.0 ** lg / _median_r(so, th, ph) * (1 + 0.1 * rng.random(so.n))


def edge_alpha(so, th, ph, seed, edge):
    """α uniform up to a 1e-12 relative jitter, the median Δτ of all (angle, site, upwind) ON the branch edge."""
    rng = np.random.default_rng(seed)
    al = np.ones(so.n) * (1 + 1e-12 * rng.random(so.n))
    return al * edge / float(np.nanmedian(_all_dtau(so, th, ph, al)))


def _oracle_grids(bcc_small, voro_small):
    return {"bcc": orc.make_sites(*bcc_small), "voronoi": orc.make_sites(*voro_small)}


@pytest.mark.parametrize("grid", ["bcc", "voronoi"])
def test_stratified_and_edge_fields_reach_every_branch(grid, bcc_small, voro_small):
    """Conditions on the INPUTS of the end-to-end cases, checked on the host: of the stratified field's Δτ each of thin / mid /
    thick holds >= 20 %, the range is <= 1e-9 … >= 1e7, and for every angle at least two BFS layers of >= 64 sites are
    entirely thin and two entirely thick (whole waves run MODE 0); the deep field reaches 1e9 … 1e12 and beyond 6e5 in bulk;
    the edge fields put >= 10 % of the Δτ on either side of their edge within a factor 2."""
    import voronoirt_amd as vrt
    so = _oracle_grids(bcc_small, voro_small)[grid]
    w, th, ph, nq = vrt.read_quadrature("ul7n12.dat")
    al = stratified_alpha(so, th, ph, 1, *STRATIFIED[grid])
    d = _all_dtau(so, th, ph, al)
    v = d[np.isfinite(d)]
    frac = [(v < W.THIN).mean(), ((v >= W.THIN) & (v <= W.THICK)).mean(), (v > W.THICK).mean()]
    assert min(frac) >= 0.2, frac
    assert v.min() <= 1e-9 and v.max() >= 1e7, (v.min(), v.max())
    for ai in range(nq):
        up = th[ai] > 90
        perm, lay = (so.perm_up, so.layers_up) if up else (so.perm_down, so.layers_down)
        n_thin = n_thick = 0
        for L in range(1, len(lay) - 1):                     # the first layer is the boundary: no visit
            sites = perm[lay[L] - 1: lay[L + 1] - 1] - 1
            if len(sites) < 64:
                continue
            dl = d[ai][sites]
            dl = dl[np.isfinite(dl)]
            n_thin += bool((dl < W.THIN).all())
            n_thick += bool((dl > W.THICK).all())
        assert n_thin >= 2 and n_thick >= 2, (ai, n_thin, n_thick)
    if grid == "bcc":                                        # the grid of the deep case
        deep = _all_dtau(so, th, ph, stratified_alpha(so, th, ph, 1, lg_top=-7.0, lg_bottom=12.0))
        dv = deep[np.isfinite(deep)]
        assert dv.max() >= 1e11 and (dv > 6e5).mean() >= 0.2 and ((dv >= W.THIN) & (dv <= W.THICK)).mean() >= 0.2
    for edge in (W.THIN, W.THICK):
        e = _all_dtau(so, th, ph, edge_alpha(so, th, ph, 2, edge))
        ev = e[np.isfinite(e)]
        assert ((ev < edge) & (ev > edge / 2)).mean() >= 0.1 and ((ev > edge) & (ev < 2 * edge)).mean() >= 0.1


@pytest.fixture(scope="module")
def grids(bcc_small, voro_small):
    import voronoirt_amd as vrt
    out = {}
    for name, (pos, nbr, bounds) in (("bcc", bcc_small), ("voronoi", voro_small)):
        out[name] = (vrt.VoronoiSites(pos, nbr, bounds, device=0), orc.make_sites(pos, nbr, bounds))
    yield out
    for hs, _ in out.values():
        hs.close()


from oracle.parity import rel as _rel     # element-wise: |a - b| < tol (|b| + smallest non-zero |b|) for EVERY element

#          name          VRT_PATH   environment read at plan creation
FORMS = (("levels",     "levels",  {}),
         ("steps",      "steps",   {}),
         ("tiles",      "tiles",   {}),
         ("per-layer",  "patches", {"VRT_PATCH_CHAIN": "0", "VRT_CHAIN_DATAFLAG": "0"}),
         ("chain",      "patches", {"VRT_PATCH_CHAIN": "1", "VRT_CHAIN_DATAFLAG": "0"}),
         ("chain-df",   "patches", {"VRT_PATCH_CHAIN": "1", "VRT_CHAIN_DATAFLAG": "1"}))


def _field(so, th, ph, kind, nlam, per_angle, seed, grid):
    rng = np.random.default_rng(seed)
    n = so.n
    S = 1 + rng.random((n, nlam))
    if kind == "stratified":
        a1 = stratified_alpha(so, th, ph, seed, *STRATIFIED[grid])
    else:
        a1 = edge_alpha(so, th, ph, seed, W.THIN if kind == "edge5e-4" else W.THICK)
    jit = 1e-12 if kind.startswith("edge") else 0.1
    al = a1[:, None] * (1 + jit * rng.random((n, nlam)))
    if per_angle:
        al = np.stack([al * (1 + jit * rng.random((n, nlam))) for _ in range(per_angle)])
    return S, al, rng.random((so.layers_up[1] - 1, nlam)), rng.random((so.layers_down[1] - 1, nlam))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["stratified", "edge5e-4", "edge50"])
@pytest.mark.parametrize("name", ["bcc", "voronoi"])
def test_fields_that_reach_every_mode_on_every_path(grids, name, kind, monkeypatch):
    """J and the per-angle I of ul7n12 x 1, 4 and 7 wavelengths, shared and per-angle α, on the stratified field (whole waves
    thin, whole waves thick, the exponential branch between) and on the two edge fields (neighbouring lanes either side of
    5e-4, of 50): the level, layer-step and tile paths and the patch path as per-layer launches, chained and chained with the
    data-as-flag hand-off at 1e-10 of the oracle; fp32 storage on the pair and the four-wavelength kernel at 5e-6 of the
    oracle on the rounded inputs."""
    import torch
    import voronoirt_amd as vrt
    from voronoirt_amd import _lib
    hs, so = grids[name]
    w, th, ph, nq = vrt.read_quadrature("ul7n12.dat")
    ks = vrt.quadrature_directions(th, ph)
    dirs = [1 if t > 90 else -1 for t in th]
    monkeypatch.setenv("VRT_PATCH_OWN", "150")
    for nlam in (1, 4, 7):
        for per_angle in (0, nq):
            S, al, I0u, I0d = _field(so, th, ph, kind, nlam, per_angle, 10 + nlam, name)
            ref = orc.J_voronoi(w, th, ph, S, al, so, I0_up=I0u, I0_down=I0d, nthreads=4)
            for form, path, env in FORMS:
                monkeypatch.setenv("VRT_PATH", path)
                for k in ("VRT_PATCH_CHAIN", "VRT_CHAIN_DATAFLAG"):
                    monkeypatch.delenv(k, raising=False)
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                plan = vrt.FormalPlan(hs, ks, 3, dirs=dirs)
                J, _ = plan.execute(S, al, weights=w, I0_up=I0u, I0_down=I0d)
                assert plan.last_path == path, (form, plan.last_path)
                if path == "patches":
                    assert (plan.last_launches == 1) == (form != "per-layer"), form
                plan.close()
                e = _rel(J, ref)
                assert e < RTOL, (form, nlam, per_angle, float(e))
            # fp32 storage: the pair kernel, and the four-wavelength kernel where the pair count is even
            dev = torch.device("cuda", 0)
            st = torch.cuda.current_stream().cuda_stream
            r32 = lambda x: np.asarray(x, dtype=np.float32)
            back = lambda x: r32(x).astype(np.float64)
            ref32 = orc.J_voronoi(w, th, ph, back(S), back(al), so, I0_up=back(I0u), I0_down=back(I0d), nthreads=4)
            Sd, Ad, Ud, Dd = (torch.from_numpy(np.ascontiguousarray(r32(x))).to(dev) for x in (S, al, I0u, I0d))
            monkeypatch.setenv("VRT_PATH", "patches")
            for quad in ((0, 1) if nlam == 4 else (0,)):
                for chain in (0, 1):
                    monkeypatch.setenv("VRT_PATCH_QUAD", str(quad))
                    monkeypatch.setenv("VRT_PATCH_CHAIN", str(chain))
                    monkeypatch.setenv("VRT_CHAIN_DATAFLAG", "0")
                    plan = vrt.FormalPlan(hs, ks, 3, dirs=dirs)
                    Jd = torch.full((so.n, nlam), float("nan"), dtype=torch.float32, device=dev)
                    plan.execute_dev(nlam, nlam, Sd.data_ptr(), Ad.data_ptr(),
                                     _lib.ALPHA_ANGLE_SITE_LAM if per_angle else _lib.ALPHA_SITE_LAM, w, dJ=Jd.data_ptr(),
                                     dI0_up=Ud.data_ptr(), dI0_down=Dd.data_ptr(), stream=st, f32=True)
                    torch.cuda.synchronize()
                    assert plan.last_path == "patches"
                    plan.close()
                    e = _rel(Jd.cpu().numpy().astype(np.float64), ref32)
                    assert e < 5e-6, ("fp32", quad, chain, nlam, per_angle, float(e))
            monkeypatch.delenv("VRT_PATCH_QUAD", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True])
def test_deep_field_is_bitwise_the_same_in_every_form(bcc_small, f32, monkeypatch):
    """The stratified field with its bottom at Δτ = 1e9 … 1e12, where a = 1/Δτ is of the size of exp(-50) times its own
    rounding: the launch form (64- and 72-register kernels per layer, chained, data-as-flag, the four-wavelength kernel
    with fp32 storage), the patch size (VRT_PATCH_OWN 200 and 64) and the storage order (strips, Morton) change which lanes
    share a wave -- and with it the MODE a thick lane runs under -- never a bit of J or of the per-angle I."""
    import torch
    import voronoirt_amd as vrt
    from voronoirt_amd import _lib
    pos, nbr, bounds = bcc_small
    so = orc.make_sites(pos, nbr, bounds)
    n, nlam = so.n, 16
    w, th, ph, nq = vrt.read_quadrature("ul7n12.dat")
    rng = np.random.default_rng(23)
    S = 1 + rng.random((n, nlam))
    a1 = stratified_alpha(so, th, ph, 23, lg_top=-7.0, lg_bottom=12.0)
    al = np.stack([a1[:, None] * (1 + 0.1 * rng.random((n, nlam))) for _ in range(nq)])
    I0u, I0d = rng.random((so.layers_up[1] - 1, nlam)), rng.random((so.layers_down[1] - 1, nlam))
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    dt = torch.float32 if f32 else torch.float64
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt).contiguous()
    Sd, Ad, Ud, Dd = f(S), f(al), f(I0u), f(I0d)
    monkeypatch.setenv("VRT_PATH", "patches")
    got = {}
    for order in ("strips", "morton"):
        monkeypatch.setenv("VRT_STORE_ORDER", order)
        hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
        for own in (200, 64):
            monkeypatch.setenv("VRT_PATCH_OWN", str(own))
            for form, env in (("lean", {"VRT_PATCH_LEAN": "1"}), ("plain", {"VRT_PATCH_LEAN": "0"}),
                              ("chain", {"VRT_PATCH_LEAN": "1", "VRT_PATCH_CHAIN": "1"}),
                              ("chain-df", {"VRT_PATCH_LEAN": "1", "VRT_PATCH_CHAIN": "1", "VRT_CHAIN_DATAFLAG": "1"}),
                              ("chain-quad", {"VRT_PATCH_LEAN": "1", "VRT_PATCH_CHAIN": "1", "VRT_PATCH_QUAD": "1"}),
                              ("lean-quad", {"VRT_PATCH_LEAN": "1", "VRT_PATCH_QUAD": "1"})):
                if ("quad" in form and not f32) or (form == "chain-df" and f32):
                    continue
                for k in ("VRT_PATCH_LEAN", "VRT_PATCH_CHAIN", "VRT_PATCH_QUAD", "VRT_CHAIN_DATAFLAG"):
                    monkeypatch.setenv(k, env.get(k, "0"))
                plan = vrt.FormalPlan(hs, vrt.quadrature_directions(th, ph), 3, dirs=[1 if t > 90 else -1 for t in th])
                Jd = torch.full((n, nlam), float("nan"), dtype=dt, device=dev)
                Id = torch.full((nq, n, nlam), float("nan"), dtype=dt, device=dev)
                plan.execute_dev(nlam, nlam, Sd.data_ptr(), Ad.data_ptr(), _lib.ALPHA_ANGLE_SITE_LAM, w, dJ=Jd.data_ptr(),
                                 dI0_up=Ud.data_ptr(), dI0_down=Dd.data_ptr(), dI_out=Id.data_ptr(), stream=st, f32=f32)
                torch.cuda.synchronize()
                assert plan.last_path == "patches"
                got[(order, own, form)] = (Jd.cpu().numpy(), Id.cpu().numpy())
                plan.close()
        hs.close()
    base = got[("strips", 200, "lean")]
    assert np.isfinite(base[0]).all()
    for key, val in got.items():
        dJ, dI = int((val[0] != base[0]).sum()), int((val[1] != base[1]).sum())
        assert dJ == 0 and dI == 0, (key, dJ, dI)
    r = lambda x: x.astype(np.float32).astype(np.float64) if f32 else x
    ref = orc.J_voronoi(w, th, ph, r(S), r(al), so, I0_up=r(I0u), I0_down=r(I0d), nthreads=4)
    assert _rel(base[0].astype(np.float64), ref) < (5e-6 if f32 else RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
def test_non_finite_opacity_stays_where_the_reference_keeps_it(grids, form, monkeypatch):
    """One site with α = ∞ and one pair of neighbouring sites with α = 1.5e308 each (their sum overflows): Δτ = +∞ is the
    thick branch, a = 0, b = 1, e = 0 -- the site takes S_c and nothing else becomes non-finite.  Every path agrees with
    the oracle on WHICH sites are finite and within 1e-10 on those."""
    import voronoirt_amd as vrt
    hs, so = grids["voronoi"]
    path, env = next((p, e) for f, p, e in FORMS if f == form)
    monkeypatch.setenv("VRT_PATH", path)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = so.n
    rng = np.random.default_rng(17)
    S = 1 + rng.random((n, 2))
    al = (5 * 10 ** rng.uniform(-3, 1, n))[:, None] * (1 + rng.random((n, 2)))
    bad = int(so.perm_up[so.layers_up[3]] - 1)             # a site in the 4th layer
    al[bad] = np.inf
    k = vrt.direction(140.0, 70.0)
    up, _, _, _, _ = orc.upwind_table(so, k)
    c = int(so.perm_up[so.layers_up[5] + 3] - 1)           # a site further up and its first upwind
    assert up[c, 0] > 0 and up[c, 0] - 1 != bad
    al[c] = 1.5e308
    al[up[c, 0] - 1] = 1.5e308
    I0 = rng.random((so.layers_up[1] - 1, 2))
    with np.errstate(all="ignore"):
        ref = orc.J_voronoi(np.array([1.0]), np.array([140.0]), np.array([70.0]), S, al, so, I0_up=I0, nthreads=2)
    plan = vrt.FormalPlan(hs, [k], 3, dirs=[1])
    got, _ = plan.execute(S, al, weights=np.array([1.0]), I0_up=I0)
    assert plan.last_path == path
    plan.close()
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    m = np.isfinite(ref)
    assert m.mean() > 0.99
    assert _rel(got[m], ref[m]) < RTOL
