"""Extended-precision references for the physics kernels of voronoirt_amd/csrc/vrt_physics.hip (test
infrastructure only; nothing in voronoirt_amd imports it).

  w4_hp(x, y)        Re of Humlíček's w4 (JQSRT 27, 437, 1982) as vrt_oracle_physics.c states it -- the same
                     fp64 coefficients, the same rational forms -- evaluated in extended precision, exp and cos
                     included.  The REGION is chosen in fp64 with the comparisons of humlicek_w4_re
                     (|x| + y >= 15, >= 5.5, y >= 0.195 |x| - 0.176): that choice is part of the algorithm, so
                     the reference never disagrees with a kernel about it.  The caller may pass the fp64 values
                     the decision is made from separately (the kernel's own v and a) and evaluate at others.
  calculate_R_hp     orc_calculate_R (calculate_R, src/rates.jl:154-201) in extended precision: the same
                     trapezoid segments, σ_bb from w4_hp with the region taken from the rate kernel's fp64
                     a = γ (λ λ) r_a and v = (λ - λ0) r_dD, and G = n_ratio exp(-hc / (λ k T)) with an extended
                     exp that is 0 wherever libm's fp64 exp underflows to 0.

Extended precision is numpy's long double when it carries at least 63 mantissa bits (x87 80-bit, or binary128);
otherwise every value is an mpmath number at 30 significant digits (slow, but the same code)."""
from __future__ import annotations

import numpy as np

EXTENDED = np.finfo(np.longdouble).nmant >= 63

if EXTENDED:
    def ext(a):
        return np.asarray(a, dtype=np.longdouble)

    _exp, _cos, _sqrt = np.exp, np.cos, np.sqrt
    PI = np.longdouble(np.pi) + np.longdouble(1.2246467991473532e-16)       # π to 107 bits, rounded once
else:                                                                       # pragma: no cover (x86-64 has it)
    import mpmath

    mpmath.mp.dps = 30

    def ext(a):
        a = np.asarray(a)
        return np.vectorize(lambda v: mpmath.mpf(v), otypes=[object])(a.astype(np.float64)) if a.dtype != object else a

    _exp = np.vectorize(mpmath.exp, otypes=[object])
    _cos = np.vectorize(mpmath.cos, otypes=[object])
    _sqrt = np.vectorize(mpmath.sqrt, otypes=[object])
    PI = mpmath.pi

# fp64 underflow of exp(-x): libm returns exactly 0 once exp(-x) <= 2^-1075 (half the smallest subnormal)
EXP_UNDERFLOW = ext(2.0) ** -1075


def w4_region(x, y) -> np.ndarray:
    """Humlíček's region (1..4) of every point, decided in fp64 as humlicek_w4_re / orc_humlicek_w4 decide it."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    ax = np.abs(x)
    s = ax + y
    return np.where(s >= 15.0, 1, np.where(s >= 5.5, 2, np.where(y >= 0.195 * ax - 0.176, 3, 4))).astype(np.int8)


# w4's coefficients as the fp64 literals of the kernel and the oracle (highest power first)
_R3_NUM = (0.5642236, 3.778987, 11.96482, 20.20933, 16.4955)              # in t
_R3_DEN = (1.0, 6.699398, 21.69274, 39.27121, 38.82363, 16.4955)
_R4_NUM = (0.56419, -1.320522, 35.76683, -219.0313, 1540.787, -3321.9905, 36183.31)      # in u = t^2: the
_R4_DEN = (-1.0, 1.841439, -61.57037, 364.2191, -2186.181, 9022.228, -24322.84, 32066.6)  # c - u (...) steps


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def _horner(coeffs, zr, zi):
    """Σ c_k z^k, complex z, real coefficients highest power first."""
    pr, pi_ = ext(np.full(np.shape(zr), coeffs[0])), ext(np.zeros(np.shape(zr)))
    for c in coeffs[1:]:
        pr, pi_ = _cmul(pr, pi_, zr, zi)
        pr = pr + ext(c)
    return pr, pi_


def _re_div(ar, ai, br, bi):
    return (ar * br + ai * bi) / (br * br + bi * bi)


def w4_hp(x, y, region=None):
    """Re w4(x + i y) in extended precision, y >= 0.  x, y: float64 or extended arrays (v and a of a Voigt
    profile: H(a, v) = Re w4(v + i a)); region: the fp64 decision (w4_region) -- by default made from x, y."""
    shape = np.broadcast(np.asarray(x), np.asarray(y)).shape
    x = ext(np.broadcast_to(x, shape)).ravel()
    y = ext(np.broadcast_to(y, shape)).ravel()
    reg = (w4_region(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)) if region is None
           else np.broadcast_to(np.asarray(region), shape)).ravel()
    out = ext(np.zeros(x.size))
    tr, ti = y, -x                                                 # t = y - i x
    for r in (1, 2, 3, 4):
        m = reg == r
        if not m.any():
            continue
        a, b = tr[m], ti[m]
        if r == 1:                                                 # t 0.5641896 / (0.5 + t^2)
            ur, ui = _cmul(a, b, a, b)
            out[m] = _re_div(a * ext(0.5641896), b * ext(0.5641896), ur + ext(0.5), ui)
        elif r == 2:                                               # t (1.410474 + 0.5641896 u) / (0.75 + u (3 + u))
            ur, ui = _cmul(a, b, a, b)
            nr, ni = _cmul(a, b, ext(1.410474) + ur * ext(0.5641896), ui * ext(0.5641896))
            dr, di = _cmul(ur, ui, ur + ext(3.0), ui)
            out[m] = _re_div(nr, ni, dr + ext(0.75), di)
        elif r == 3:
            nr, ni = _horner(_R3_NUM, a, b)
            dr, di = _horner(_R3_DEN, a, b)
            out[m] = _re_div(nr, ni, dr, di)
        else:                                                      # exp(u) - t num(u) / den(u), u = t^2
            ur, ui = _cmul(a, b, a, b)
            nr, ni = _horner(_R4_NUM, ur, ui)
            dr, di = _horner(_R4_DEN, ur, ui)
            qr, qi = _cmul(a, b, nr, ni)
            out[m] = _exp(ur) * _cos(ui) - _re_div(qr, qi, dr, di)
    return out.reshape(shape)


def kernel_va(lam, lambda0, c0, doppler, gamma, shift=0.0):
    """(v, a) in fp64 exactly as the kernels form them (vrt_physics.hip, built with -ffp-contract=off):
    v = (λ - λ0 + shift) (1 / ΔλD), a = (γ / (4 π c0 ΔλD)) (λ λ) [opacity] -- per site (rows) and wavelength."""
    lam = np.asarray(lam, dtype=np.float64)[None, :]
    dD = np.asarray(doppler, dtype=np.float64)[:, None]
    g = np.asarray(gamma, dtype=np.float64)[:, None]
    shift = np.asarray(shift, dtype=np.float64)
    shift = shift[:, None] if shift.ndim else shift
    v = (lam - lambda0 + shift) * (1.0 / dD)
    a = (g / (4.0 * np.pi * c0 * dD)) * (lam * lam)
    return v, a


def rates_kernel_va(lam, lambda0, c0, doppler, gamma):
    """(v, a) of σ_bb as k_rates_populations forms them: a = γ (λ λ) r_a, r_a = 1 / (4 π c0 ΔλD); v = (λ - λ0) r_dD."""
    lam = np.asarray(lam, dtype=np.float64)[None, :]
    dD = np.asarray(doppler, dtype=np.float64)[:, None]
    g = np.asarray(gamma, dtype=np.float64)[:, None]
    a = g * (lam * lam) * (1.0 / (4.0 * np.pi * c0 * dD))
    v = (lam - lambda0) * (1.0 / dD)
    return v, a


def boltzmann_hp(hc_over_kB, lam, T):
    """exp(-hc / (λ k T)) per site (rows) and wavelength, extended, 0 where fp64 exp underflows to 0."""
    x = ext(hc_over_kB) / (ext(lam)[None, :] * ext(T)[:, None])
    e = _exp(-x)
    return np.where(e <= EXP_UNDERFLOW, ext(0.0), e)


def calculate_R_hp(lam, blocks, J, planck2, lambda0, c0, doppler, gamma, sigma_bb_const, sigma_bf1, sigma_bf2,
                   temperature, lte, hc_over_kB, pref_ij, pref_ji):
    """orc_calculate_R in extended precision; arguments as oracle.calculate_R (J (n, nlam), lte (3, n)).
    Returns R (n, 3, 3) extended, R[i, c, r] == Julia R[r+1, c+1, i+1]."""
    lam_e = ext(lam)
    J = ext(J)
    P = ext(planck2)
    lte = ext(lte)
    n = J.shape[0]
    R = ext(np.zeros((n, 3, 3)))

    def trapezoids(lo, hi, sig, G):
        """pref_ij Σ (λ σ J)_l + (λ σ J)_l+1) dl and pref_ji Σ (σ G λ (P + J))_l + ... ) dl over [lo, hi)."""
        l = lam_e[lo:hi][None, :]
        dl = lam_e[lo + 1:hi] - lam_e[lo:hi - 1]
        fij = l * sig * J[:, lo:hi]
        fji = sig * G * l * (P[lo:hi][None, :] + J[:, lo:hi])
        rij = (ext(pref_ij) * ((fij[:, :-1] + fij[:, 1:]) * dl[None, :])).sum(axis=1)
        rji = (ext(pref_ji) * ((fji[:, :-1] + fji[:, 1:]) * dl[None, :])).sum(axis=1)
        return rij, rji

    for level, sig in ((1, sigma_bf1), (2, sigma_bf2)):
        lo, hi = int(blocks[2 * level]), int(blocks[2 * level + 1])
        G = (lte[level - 1] / lte[2])[:, None] * boltzmann_hp(hc_over_kB, lam[lo:hi], temperature)
        rij, rji = trapezoids(lo, hi, ext(sig)[None, :], G)
        R[:, 2, level - 1] = rij                 # Julia R[level, 3]
        R[:, level - 1, 2] = rji                 # Julia R[3, level]
    lo, hi = int(blocks[0]), int(blocks[1])
    dD = ext(doppler)[:, None]
    l = lam_e[lo:hi][None, :]
    a = ext(gamma)[:, None] * (l * l) / (ext(4.0) * PI * ext(c0) * dD)
    v = (l - ext(lambda0)) / dD
    vk, ak = rates_kernel_va(lam[lo:hi], lambda0, c0, doppler, gamma)
    H = w4_hp(v, a, region=w4_region(vk, ak))
    sig = ext(sigma_bb_const) * (H / (_sqrt(PI) * dD))
    G = (lte[0] / lte[1])[:, None] * boltzmann_hp(hc_over_kB, lam[lo:hi], temperature)
    rij, rji = trapezoids(lo, hi, sig, G)
    R[:, 1, 0] = rij                             # Julia R[1, 2]
    R[:, 0, 1] = rji                             # Julia R[2, 1]
    return R
