"""References for the emergent-spectrum kernels (test infrastructure only; nothing in voronoirt_amd imports it).

  tau_exact(alpha, z, dx, dy, k)   the algorithm of include/voronoirt.h ("vrt_tau_unity_dev") in exact rational
                     arithmetic on the double inputs: a double is a rational, so floor, the bilinear blend and the
                     trapezoid are exact.  Returns the exact tau of every (wavelength, column, plane) and a forward
                     error bound of its fp64 evaluation,
                         B_j = 16 u sum_{i <= j} r_i (1 + |U_i| + |V_i|) Q_i,       u = 2^-53,
                     r_i the path step, U_i, V_i the lateral offsets in cells, Q_i the largest |alpha| among the
                     eight nodes of step i.  The kernel makes fewer than 16 roundings per step; the relative error of
                     U multiplies |U| before it reaches the fraction; a rounded U that lands on the other side of an
                     integer costs nothing, because the interpolant is continuous there.  Derived, not measured.
  tau_candidates(tau, B)           per column the planes whose exact |tau - 1| lies within 2 B_bottom of the exact
                     minimum: any fp64 evaluation within the bound returns one of them.  A column is DECIDED when the
                     set has one member.  A column with a NaN tau has one candidate: the first plane (from the top)
                     whose tau is NaN -- Julia's and numpy's argmin.
  synth_point_hp(...)              alpha_tot and S of k_synth_opacity per (point, wavelength) in mpmath, as the formula
                     is written (exp(x) - 1, not expm1), with the condition number of that formula.

Non-finite alpha is defined where the march reads grid values only (both lateral offsets whole cells, e.g. the
vertical directions): a node that is not read does not count, a NaN that is read makes tau NaN from its plane down,
an Inf makes it Inf.  With a fractional offset a non-finite alpha raises: which of Inf and NaN a blend gives there
depends on the form of the blend, which is not part of the algorithm."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

U_ROUND = 2.0 ** -53


def _frac_array(a):
    """object array of Fractions of a float64 array (non-finite entries become 0: see the special pass)"""
    a = np.asarray(a, dtype=np.float64)
    flat = [Fraction(v) if math.isfinite(v) else Fraction(0) for v in a.ravel().tolist()]
    out = np.empty(a.size, dtype=object)
    out[:] = flat
    return out.reshape(a.shape)


def _cell(U, n):
    """first node shift, second node shift (both mod n, as offsets from the column) and the fraction of an offset of
    U cells: exact"""
    f = math.floor(U)
    return f % n, (f + 1) % n, U - f


def tau_exact(alpha, z, dx, dy, k):
    """alpha (nlam, ny, nx, nz) INTERIOR float64, z (nz) ascending, dx, dy the spacings as the library forms them
    ((x[-1] - x[0]) / (nx - 1) in fp64), k = (k_z, k_x, k_y).
    Returns (tau, B): tau an object array (nlam, ny, nx, nz) of Fractions indexed by plane iz (tau[..., nz - 1] = 0 at
    the top), with float nan / inf entries where the column read a non-finite node; B float64 of the same shape."""
    alpha = np.asarray(alpha, dtype=np.float64)
    nl, ny, nx, nz = alpha.shape
    zf = [Fraction(float(v)) for v in z]
    kz, kx, ky = (Fraction(float(v)) for v in k)
    dxf, dyf = Fraction(float(dx)), Fraction(float(dy))
    akz = abs(kz)
    finite = np.isfinite(alpha)
    A = _frac_array(alpha)
    absA = np.where(finite, np.abs(alpha), 0.0)
    sp = np.where(finite, 0.0, alpha)                              # 0, nan or +-inf per node
    tau = np.empty(alpha.shape, dtype=object)
    B = np.zeros(alpha.shape)
    tau[..., nz - 1] = Fraction(0)
    tau_sp = np.zeros((nl, ny, nx))
    prev, prev_q, prev_sp = A[..., nz - 1], absA[..., nz - 1], sp[..., nz - 1]
    cur, cur_B = tau[..., nz - 1], B[..., nz - 1]
    special = np.zeros(alpha.shape)
    for iz in range(nz - 2, -1, -1):
        s = (zf[nz - 1] - zf[iz]) / akz
        U, V = s * kx / dxf, s * ky / dyf
        i0, i1, tx = _cell(U, nx)
        j0, j1, ty = _cell(V, ny)
        P, Q, Sp = A[..., iz], absA[..., iz], sp[..., iz]

        def at(F, dj, di):
            return np.roll(np.roll(F, -dj, axis=1), -di, axis=2)   # F[:, (iy + dj) % ny, (ix + di) % nx]
        a = at(P, j0, i0) * ((1 - tx) * (1 - ty))
        q, a_sp = at(Q, j0, i0), at(Sp, j0, i0)
        for w, dj, di in ((tx * (1 - ty), j0, i1), ((1 - tx) * ty, j1, i0), (tx * ty, j1, i1)):
            q = np.maximum(q, at(Q, dj, di))                       # (a rounded offset may reach it with weight ~ u |U|)
            if w == 0:
                continue                                           # not read
            a = a + at(P, dj, di) * w
            with np.errstate(invalid="ignore"):
                a_sp = a_sp + at(Sp, dj, di)
        if (tx != 0 or ty != 0) and not finite[..., iz].all():
            raise ValueError("non-finite alpha under a fractional offset is not defined by the algorithm")
        r = abs((zf[iz + 1] - zf[iz]) / kz)
        cur = cur + (a + prev) * (r / 2)
        with np.errstate(invalid="ignore"):
            tau_sp = tau_sp + (a_sp + prev_sp)
        cur_B = cur_B + 16.0 * U_ROUND * float(r) * (1.0 + abs(float(U)) + abs(float(V))) * np.maximum(q, prev_q)
        tau[..., iz], B[..., iz], special[..., iz] = cur, cur_B, tau_sp
        prev, prev_q, prev_sp = a, q, a_sp
    bad = special != 0                                             # nan != 0 is True
    tau[bad] = special[bad]
    return tau, B


def abs_tau_minus_one(tau):
    """|tau - 1| per entry: Fraction, or float nan / inf"""
    out = np.empty(tau.shape, dtype=object)
    flat_in, flat_out = tau.ravel(), out.ravel()
    for i, t in enumerate(flat_in):
        flat_out[i] = abs(t - 1)
    return out


def tau_candidates(tau, B):
    """list over (nlam, ny, nx) flattened in that order of the candidate planes (iz, ascending) of each column"""
    nl, ny, nx, nz = tau.shape
    d = abs_tau_minus_one(tau).reshape(-1, nz)
    Bb = B.reshape(-1, nz)[:, 0]
    out = []
    for c in range(d.shape[0]):
        row = d[c]
        nan = [iz for iz in range(nz - 1, -1, -1) if isinstance(row[iz], float) and math.isnan(row[iz])]
        if nan:
            out.append([nan[0]])                                   # the first NaN from the top
            continue
        fin = [iz for iz in range(nz) if not isinstance(row[iz], float)]         # (inf never wins: the top has d = 1)
        dmin = min(row[iz] for iz in fin)
        slack = Fraction(2.0 * float(Bb[c]))
        out.append([iz for iz in fin if row[iz] - dmin <= slack])
    return out


def first_argmin(tau):
    """the plane the exact algorithm returns: first minimum of |tau - 1| from the top, NaN first (Julia's argmin)"""
    nl, ny, nx, nz = tau.shape
    d = abs_tau_minus_one(tau).reshape(-1, nz)
    out = np.zeros(d.shape[0], dtype=np.int64)
    for c in range(d.shape[0]):
        best, arg = None, nz - 1
        for iz in range(nz - 1, -1, -1):
            v = d[c, iz]
            if isinstance(v, float) and math.isnan(v):
                arg = iz
                break
            if best is None or v < best:
                best, arg = v, iz
        out[c] = arg
    return out.reshape(nl, ny, nx)


# ---- k_synth_opacity ----------------------------------------------------------------------------------------------------
def synth_point_hp(k, lam, planck2, case, src_const, g_ratio, velocity, doppler, gamma_static, gamma_unsold, temperature,
                   alpha_cont, n1, n2):
    """alpha_tot, S and kappa, each (npoint, nlam) float64 (rounded once from 30 digits), of plotter's formulae as
    k_synth_opacity writes them, for flat per-point fields (velocity (npoint, 3) [z, x, y]):
        alpha_l = strength_const (n1 Bij - n2 Bji) H(a, v) / (sqrt(pi) dD),  a = gamma lam^2 / (4 pi c0 dD),
        v = (lam - lambda0 + lambda0 v_los / c0) / dD,  v_los = -k . velocity,  gamma = gamma_static + gamma_unsold (n1 + n2)
        S_l = src_const / (g n1 / n2 - 1),   S_c = planck2 / (exp(x) - 1),  x = hc_over_kB / (lam T)
        S = (alpha_l S_l + alpha_c S_c) / (alpha_l + alpha_c),   alpha_tot = alpha_l + alpha_c
    H = Re w4 from physics_ref.w4_hp in the region the kernel's own fp64 (v, a) choose.  IEEE's special values are kept:
    n2 = 0 < n1 gives S_l = 0, n1 = n2 = 0 gives S = NaN.
    kappa = max(1, 1/x for x < 1, (|al Sl| + |ac Sc|) / |al Sl + ac Sc|, (|al| + |ac|) / |al + ac|): the condition of the
    formula as written under roundings of its own terms."""
    import mpmath

    from oracle import physics_ref as pr

    mp = mpmath.mp.clone()
    mp.dps = 40
    f = mp.mpf
    lam = np.asarray(lam, dtype=np.float64)
    planck2 = np.asarray(planck2, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    flat = [np.asarray(a, dtype=np.float64).ravel() for a in (doppler, gamma_static, gamma_unsold, temperature,
                                                               alpha_cont, n1, n2)]
    dD, gs, gu, T, ac, n1, n2 = flat
    vel = np.asarray(velocity, dtype=np.float64).reshape(-1, 3)
    npnt, nl = dD.size, lam.size
    # the kernel's own fp64 v and a decide the region of w4 (statement order of k_synth_opacity)
    v_los64 = vel[:, 0] * (-k[0]) + vel[:, 1] * (-k[1]) + vel[:, 2] * (-k[2])
    gamma64 = gs + gu * (n1 + n2)
    vk, ak = pr.kernel_va(lam, case.lambda0, case.c0, dD, gamma64, shift=case.lambda0 * v_los64 / case.c0)
    region = pr.w4_region(vk, ak)
    # v and a in extended precision from the inputs, H there
    e = pr.ext
    v_los = e(vel[:, 0]) * e(-k[0]) + e(vel[:, 1]) * e(-k[1]) + e(vel[:, 2]) * e(-k[2])
    gamma = e(gs) + e(gu) * (e(n1) + e(n2))
    lam_e = e(lam)[None, :]
    v_e = (lam_e - e(case.lambda0) + e(case.lambda0) * v_los[:, None] / e(case.c0)) / e(dD)[:, None]
    a_e = gamma[:, None] * (lam_e * lam_e) / (e(4.0) * pr.PI * e(case.c0) * e(dD)[:, None])
    H = pr.w4_hp(v_e, a_e, region=region)

    def mpf(x):                                                    # a long double (or mpmath number) to mpmath, exactly
        if not pr.EXTENDED:
            return f(x)
        hi = float(x)
        return f(hi) + f(float(x - np.longdouble(hi)))
    A = np.zeros((npnt, nl))
    S = np.zeros((npnt, nl))
    K = np.ones((npnt, nl))
    sqrt_pi = mp.sqrt(mp.pi)
    for p in range(npnt):
        strength = f(case.strength_const) * (f(n1[p]) * f(case.Bij) - f(n2[p]) * f(case.Bji))
        if n2[p] == 0.0:
            S_l = f(0) if n1[p] > 0.0 else None                    # src / (inf - 1) = 0;  0/0: NaN
        else:
            S_l = f(src_const) / (f(g_ratio) * f(n1[p]) / f(n2[p]) - 1)
        for l in range(nl):
            al = strength * mpf(H[p, l]) / (sqrt_pi * f(dD[p]))
            a_c = f(ac[p])
            x = f(case.hc_over_kB) / (f(lam[l]) * f(T[p]))
            S_c = f(planck2[l]) / (mp.exp(x) - 1)
            tot = al + a_c
            A[p, l] = float(tot)
            kap = [f(1)]
            if x < 1:
                kap.append(1 / x)
            if tot != 0:
                kap.append((abs(al) + abs(a_c)) / abs(tot))
            if S_l is None:
                S[p, l] = np.nan
            else:
                num = al * S_l + a_c * S_c
                S[p, l] = float(num / tot) if tot != 0 else np.nan
                if num != 0:
                    kap.append((abs(al * S_l) + abs(a_c * S_c)) / abs(num))
            K[p, l] = float(max(kap))
    return A, S, K
