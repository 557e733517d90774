"""40-digit references for linear_weights (src/functions.jl:484-500 of the reference; test infrastructure only,
nothing in voronoirt_amd imports it).

  weights_formula_mp(dtau)    the reference's THREE-BRANCH FORMULA, evaluated exactly (40 digits) on the fp64 value of
                              Δτ, the branch chosen by the fp64 comparisons Δτ < 5e-4 and Δτ > 50:
                                  Δτ < 5e-4:  e = 1 - Δτ + Δτ²/2,  a = Δτ (1/2 - Δτ/3),  b = Δτ (1/2 - Δτ/6)
                                  Δτ > 50:    e = 0,  a = 1/Δτ,  b = 1 - a
                                  else:       e = exp(-Δτ),  a = (1 - e)/Δτ - e,  b = 1 - a - e
                              This is the contract of every device copy: the Taylor truncation and e = 0 included.
                              NaN takes the third branch like in the reference (no comparison holds) and gives NaN;
                              +∞ gives (0, 1, 0).
  weights_integral_mp(dtau)   what the formula approximates: e = exp(-Δτ), a = (1 - e)/Δτ - e, b = 1 - a - e for every
                              Δτ != 0 -- only to document how far the formula is from it.
  exp_neg_mp(x)               exp(-x).
  split(values)               mpmath numbers -> (hi, lo) fp64 arrays with hi + lo = value to ~32 digits, so that
                              errors of fp64 results can be formed with numpy: (got - hi) - lo.

Returned triples are ordered (a, b, e) like orc.linear_weights."""
from __future__ import annotations

import math

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 40
THIN, THICK = 5e-4, 50.0            # the reference's branch constants (fp64 literals)


def branch(dtau: float) -> int:
    """0 Taylor, 1 exponential, 2 thick -- by the reference's fp64 comparisons (NaN: 1, no comparison holds)."""
    return 0 if dtau < THIN else 2 if dtau > THICK else 1


def weights_formula_mp(dtau: float, force_branch: int | None = None):
    d = float(dtau)
    if math.isnan(d):
        return MP.nan, MP.nan, MP.nan
    br = branch(d) if force_branch is None else force_branch
    if math.isinf(d) and d > 0 and br == 2:
        return MP.mpf(0), MP.mpf(1), MP.mpf(0)
    x = MP.mpf(d)
    if br == 0:
        return x * (MP.mpf(1) / 2 - x / 3), x * (MP.mpf(1) / 2 - x / 6), 1 - x + x * x / 2
    if br == 2:
        a = 1 / x
        return a, 1 - a, MP.mpf(0)
    e = MP.exp(-x)
    a = (1 - e) / x - e
    return a, 1 - a - e, e


def weights_integral_mp(dtau: float):
    d = float(dtau)
    if d == 0.0:
        return MP.mpf(0), MP.mpf(0), MP.mpf(1)
    x = MP.mpf(d)
    e = MP.exp(-x)
    a = -MP.expm1(-x) / x - e
    return a, 1 - a - e, e


def exp_neg_mp(x: float):
    return MP.exp(-MP.mpf(float(x)))


def split(values):
    """(hi, lo) fp64 arrays of a sequence of mpmath numbers (NaN -> (nan, nan); exact for ±∞ and 0)."""
    hi = np.empty(len(values))
    lo = np.empty(len(values))
    for i, v in enumerate(values):
        h = float(v)
        hi[i] = h
        lo[i] = float(v - MP.mpf(h)) if math.isfinite(h) else (0.0 if math.isinf(h) else math.nan)
    return hi, lo


def formula_arrays(dtau, force_branch: int | None = None):
    """weights_formula_mp over an fp64 array: ((a_hi, a_lo), (b_hi, b_lo), (e_hi, e_lo))."""
    rows = [weights_formula_mp(d, force_branch) for d in np.asarray(dtau, dtype=np.float64)]
    return tuple(split([r[k] for r in rows]) for k in range(3))


def _ulp_neighbours(x: float, k: int = 4):
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo = math.nextafter(lo, -math.inf)
        hi = math.nextafter(hi, math.inf)
        out += [lo, hi]
    return sorted(out)


def point_set(seed: int = 20241) -> np.ndarray:
    """The Δτ values every copy is judged at (≈ 1.1e5, seeded): 0, the smallest subnormal, the smallest normal,
    1e-300 … 5e-4, every double within ±4 ulp of 5e-4 and of 50, 5e-4 … 50 log-spaced, linearly scanned and at the
    extremes of both exponentials' argument reductions (|r| at 0.994 of ln2/64 for every N of exp_neg_tab, of ln2/2 for
    every k of exp_neg), 50 … 1e12, 1e12 … DBL_MAX, +∞, NaN and a few negative values (the Taylor branch)."""
    rng = np.random.default_rng(seed)
    ln2 = math.log(2.0)
    dmax = np.finfo(np.float64).max
    parts = [
        [0.0, 5e-324, np.finfo(np.float64).tiny, dmax, math.inf, math.nan],
        [-1e-3, -1e-4, -1e-8, -1e-300, -5e-324],
        10.0 ** rng.uniform(-300, math.log10(5e-4), 20000),
        10.0 ** rng.uniform(-9, math.log10(5e-4), 5000),
        _ulp_neighbours(5e-4), _ulp_neighbours(50.0),
        10.0 ** rng.uniform(math.log10(5e-4), math.log10(50.0), 40000),
        np.linspace(5e-4, 50.0, 20001),
        [(N + 0.5 + s * 0.003) * ln2 / 32 for N in range(0, 2308) for s in (-1, 1)],
        [(k + 0.5 + s * 0.003) * ln2 for k in range(0, 72) for s in (-1, 1)],
        10.0 ** rng.uniform(math.log10(50.0), 12, 20000),
        10.0 ** rng.uniform(12, 308, 5000),
    ]
    x = np.concatenate([np.asarray(p, dtype=np.float64) for p in parts])
    return x


def exp_tab_points(seed: int = 20242) -> np.ndarray:
    """Arguments of exp_neg_tab over its whole range 0 … 745: the points of point_set() in [0, 50], 50 … 745 at random,
    the reduction's extremes for every 7th N up to 34394, and a dense scan of the subnormal results (708.4 … 745)."""
    rng = np.random.default_rng(seed)
    ln2 = math.log(2.0)
    p = point_set()
    p = p[(p >= 0) & (p <= 50.0)]
    ext = np.array([(N + 0.5 + s * 0.003) * ln2 / 32 for N in range(2308, 34394, 7) for s in (-1, 1)])
    return np.concatenate([p, rng.uniform(50.0, 745.0, 20000), ext[ext <= 745.0], np.linspace(708.0, 745.0, 4001), [745.0]])
