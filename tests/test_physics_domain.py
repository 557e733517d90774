"""The opacity and rate kernels (vrt_physics.hip) over the whole physical domain of their inputs, against the
extended-precision references of oracle/physics_ref.py.

test_physics.py checks both kernels against the oracle on a narrow slice: damping a < 0.013, the line core for
region 3 of w4, one wavelength-block layout, grids of 1 500 sites.  Here:
  * the references check themselves (CPU): w4_hp against mpmath at 40 digits, the oracle's w4 against w4_hp over
    |v| <= 1e4, 0 <= a <= 10, calculate_R_hp against the oracle on every rate case below;
  * the device's w4 is read out exactly (-m gpu): with velocity 0, α_cont 0, λ0 = c0 = 1 and line strength
    sqrt(π) ΔλD the opacity kernel's α_tot IS its H(a, v), at (v, a) recomputed here bit for bit;
  * the rate kernel runs block lengths 2 / 15 / 16 / 17 / 33, bf blocks before the bb block, ld > nλ with NaN
    padding, grids of 192 and 350 sites, damping up to 1, hc/λkT from 0.004 to past libm's underflow of exp.

Observed on MI355X, device H against w4_hp (relative): 3.9e-14 overall; region 1 1.0e-15, region 2 1.9e-15,
region 3 1.5e-15, region 4 3.9e-14, region 4 through cos_small's reduction branch 3.2e-14.  The rate kernel against
calculate_R_hp: <= 6.8e-15 on the SI cases, 1.2e-13 on the cold one (hc/λkT ~ 700 magnifies the argument's last bit)."""
import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from oracle import physics_ref as pr
from voronoirt_amd import api, synth

C0 = 2.99792458e8
H_PLANCK = 6.62607015e-34
K_B = 1.380649e-23
TINY = np.finfo(np.float64).tiny                    # smallest normal: below it a result is subnormal


def _rel_nonzero(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    m = ref != 0
    return float((np.abs(got[m] - ref[m]) / np.abs(ref[m])).max()) if m.any() else 0.0


def _check_R(R, R_ref, what):
    """Same zero pattern; relative 1e-12 where the reference is normal, 1e-320 absolute where it is subnormal."""
    R, R_ref = np.asarray(R, dtype=np.float64), np.asarray(R_ref, dtype=np.float64)
    assert np.array_equal(R == 0, R_ref == 0), (what, np.argwhere((R == 0) != (R_ref == 0))[:5])
    normal = np.abs(R_ref) >= TINY
    sub = (R_ref != 0) & ~normal
    err = float((np.abs(R[normal] / R_ref[normal] - 1)).max())
    assert err < 1e-12, (what, err)
    if sub.any():
        assert np.abs(R[sub] - R_ref[sub]).max() <= 1e-320, (what, np.abs(R[sub] - R_ref[sub]).max())
    return err


# ---- the references check themselves -----------------------------------------------------------------
def _w4_mp(x, y, region):
    """Independent transcription of orc_humlicek_w4 in mpmath complex arithmetic (40 digits), region given."""
    import mpmath
    with mpmath.workdps(40):
        c = lambda v: mpmath.mpf(float(v))
        t = mpmath.mpc(c(y), -c(x))
        if region == 1:
            w = t * c(0.5641896) / (c(0.5) + t * t)
        elif region == 2:
            u = t * t
            w = t * (c(1.410474) + u * c(0.5641896)) / (c(0.75) + u * (c(3.0) + u))
        elif region == 3:
            num = c(3.778987) + t * c(0.5642236)
            for k in (11.96482, 20.20933, 16.4955):
                num = c(k) + t * num
            den = c(6.699398) + t
            for k in (21.69274, 39.27121, 38.82363, 16.4955):
                den = c(k) + t * den
            w = num / den
        else:
            u = t * t
            num = c(1.320522) - u * c(0.56419)
            for k in (35.76683, 219.0313, 1540.787, 3321.9905, 36183.31):
                num = c(k) - u * num
            den = c(1.841439) - u
            for k in (61.57037, 364.2191, 2186.181, 9022.228, 24322.84, 32066.6):
                den = c(k) - u * den
            w = mpmath.exp(u) - t * num / den
        return w.real


def _boundary_points(rng, count):
    """(x, y) pairs within a few ulps either side of the three region boundaries of w4."""
    xs, ys = [], []
    for _ in range(count):
        b = rng.integers(3)
        if b < 2:
            s = (15.0, 5.5)[b]
            x = rng.uniform(0.01, s) * rng.choice([-1, 1])
            y = s - abs(x)
        else:
            x = rng.uniform(0.91, 4.6) * rng.choice([-1, 1])
            y = 0.195 * abs(x) - 0.176
        y = max(y, 0.0)
        for k in range(-2, 3):
            ys.append(y + k * np.spacing(max(y, 1.0)))
            xs.append(x)
    return np.array(xs), np.maximum(np.array(ys), 0.0)


def _domain_points(rng, count):
    """|v| <= 1e4 (log-spaced, both signs, and 0), a in {0} and 1e-8 .. 10."""
    v = np.concatenate([10 ** rng.uniform(-8, 4, count) * rng.choice([-1, 1], count), rng.uniform(-16, 16, count)])
    a = np.concatenate([10 ** rng.uniform(-8, 1, count), rng.uniform(0, 10, count)])
    a[rng.random(a.size) < 0.05] = 0.0
    return v, a


def test_w4_hp_against_mpmath():
    """w4_hp (extended) against mpmath at 40 digits on ~2 000 points: every region, both sides of every boundary,
    y = 0: 1e-17 relative, and exactly 0 where the mpmath value is 0 (y = 0 in regions 1 and 2)."""
    rng = np.random.default_rng(21)
    v, a = _domain_points(rng, 300)
    bx, by = _boundary_points(rng, 200)
    x = np.concatenate([v, bx, rng.uniform(-16, 16, 200), [0.0, 1.0, -3.0, 14.9, 20.0]])
    y = np.concatenate([a, by, np.zeros(200), [0.0, 0.0, 0.0, 0.0, 0.0]])
    reg = pr.w4_region(x, y)
    assert set(np.unique(reg)) == {1, 2, 3, 4}
    got = pr.w4_hp(x, y)
    ref = np.array([_w4_mp(xi, yi, r) for xi, yi, r in zip(x, y, reg)])
    import mpmath
    zero = np.array([r == 0 for r in ref])
    assert zero.sum() > 20 and (np.asarray(got[zero], dtype=np.float64) == 0).all()
    exact = lambda g: mpmath.mpf(float(g)) + mpmath.mpf(float(g - np.longdouble(float(g))))     # extended -> mpf
    with mpmath.workdps(40):
        err = max(abs((exact(g) - r) / r) for g, r, z in zip(got, ref, zero) if not z)
    assert err < 1e-17, float(err)


def test_oracle_w4_against_w4_hp_over_the_domain():
    """The oracle's restatement (fp64, libm) is the kernels' parity target: within 1e-13 of w4_hp over |v| <= 1e4,
    0 <= a <= 10, boundary neighbourhoods included (same fp64 region decision), and 0 exactly where w4_hp is 0."""
    rng = np.random.default_rng(22)
    v, a = _domain_points(rng, 6000)
    bx, by = _boundary_points(rng, 600)
    v, a = np.concatenate([v, bx]), np.concatenate([a, by])
    ref = np.asarray(pr.w4_hp(v, a), dtype=np.float64)
    got = np.array([orc.humlicek_w4(x, y).real for x, y in zip(v, a)])
    assert np.array_equal(got == 0, ref == 0)
    assert _rel_nonzero(got, ref) < 1e-13


# ---- rate cases at the edges ------------------------------------------------------------------------------
def _rate_case(name, n, seed):
    """Inputs of rates_populations_dev on n sites.  Every case: three blocks [lo, hi) covering the wavelengths."""
    rng = np.random.default_rng(seed)
    if name == "cold":
        # O(1) units: λ0 = 2, hc/k = 1, 1/T in [800, 880].  bf level 1 (16 λ in [0.6, 1.0]) has hc/λkT >= 800
        # everywhere: its G underflows to 0 in libm, so its reference R_ji is exactly 0; bf level 2 (17 λ in
        # [1.07, 1.17]) spans hc/λkT 684..822: its R_ji is normal, subnormal or 0 by site; bb (15 λ around 2): ~e^-420
        lambda0, c0 = 2.0, 1.0
        nbb, nb1, nb2 = 15, 16, 17
        lam_bb = lambda0 + np.linspace(-0.05, 0.05, nbb)
        lam_b1, lam_b2 = np.linspace(0.6, 1.0, nb1), np.linspace(1.07, 1.17, nb2)
        lam = np.concatenate([lam_b1, lam_b2, lam_bb])                      # bf blocks first in λ and in memory
        blocks = np.array([nb1 + nb2, nb1 + nb2 + nbb, 0, nb1, nb1, nb1 + nb2], dtype=np.int64)
        T = 1.0 / rng.uniform(800.0, 880.0, n)
        doppler = rng.uniform(5e-3, 2e-2, n)
        gamma = rng.uniform(0.0, 0.1, n)
        J = rng.uniform(0.5, 2.0, (n, lam.size))
        planck2 = 2.0 * (lambda0 / lam) ** 5
        lte = np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(0.2, 0.6, n), rng.uniform(0.005, 0.02, n)])
        sig1, sig2 = rng.uniform(0.5, 1.5, nb1), rng.uniform(0.5, 1.5, nb2)
        consts = dict(sigma_bb_const=0.3, hc_over_kB=1.0, pref_ij=2.0, pref_ji=3.0)
    else:
        lambda0, c0 = 121.567e-9, C0
        nbb, nb1, nb2 = {"lengths": (17, 2, 33), "order": (33, 16, 15), "damping": (51, 16, 17),
                         "hot": (16, 17, 2)}[name]
        q = np.concatenate([-np.geomspace(600, 0.05, nbb // 2), [0.0] * (nbb % 2), np.geomspace(0.05, 600, nbb // 2)])
        lam_bb = lambda0 * (1 + q * 2.5e3 / C0)
        lam_b1, lam_b2 = np.linspace(22.8e-9, 91.17e-9, nb1), np.linspace(91.2e-9, 364.7e-9, nb2)
        if name == "order":                                                 # bf blocks before bb, in λ and in memory
            lam_b1, lam_b2 = np.linspace(20.0e-9, 60.0e-9, nb1), np.linspace(61.0e-9, 115.0e-9, nb2)
            lam = np.concatenate([lam_b1, lam_b2, lam_bb])
            blocks = np.array([nb1 + nb2, nb1 + nb2 + nbb, 0, nb1, nb1, nb1 + nb2], dtype=np.int64)
        else:
            lam = np.concatenate([lam_bb, lam_b1, lam_b2])
            blocks = np.array([0, nbb, nbb, nbb + nb1, nbb + nb1, nbb + nb1 + nb2], dtype=np.int64)
        T = 10 ** rng.uniform(7.0, 8.0, n) if name == "hot" else rng.uniform(4e3, 2e4, n)
        doppler = lambda0 / C0 * np.sqrt(2 * K_B * T / 1.6735575e-27)
        a_target = 10 ** rng.uniform(-3, 0, n) if name == "damping" else 10 ** rng.uniform(-6, -2, n)
        gamma = a_target * 4 * np.pi * C0 * doppler / lambda0 ** 2
        J = 10 ** rng.uniform(-12, -3, (n, lam.size))
        planck2 = 2 * H_PLANCK * C0 ** 2 / lam ** 5
        n_i = 10 ** rng.uniform(14, 19, n)
        lte = np.stack([n_i, n_i * 10 ** rng.uniform(-9, -5, n), n_i * 10 ** rng.uniform(-6, 0, n)])
        sig1 = 7.9e-22 * (lam_b1 / lam_b1[-1]) ** 3
        sig2 = 1.4e-21 * (lam_b2 / lam_b2[-1]) ** 3
        consts = dict(sigma_bb_const=H_PLANCK * C0 / (4 * np.pi * lambda0) * 4.5e20, hc_over_kB=H_PLANCK * C0 / K_B,
                      pref_ij=2 * np.pi / (H_PLANCK * C0) / 1000.0, pref_ji=2 * np.pi / (H_PLANCK * C0))
    C = 10 ** rng.uniform(-2, 4, (n, 3, 3))
    for d in range(3):
        C[:, d, d] = 0.0
    return dict(lam=lam, blocks=blocks, lambda0=lambda0, c0=c0, T=T, doppler=doppler, gamma=gamma, J=J,
                planck2=planck2, lte=lte, sig1=sig1, sig2=sig2, C=C, atom=lte.sum(axis=0) * rng.uniform(0.9, 1.1, n),
                **consts)


def _R_args(c):
    return (c["lam"], c["blocks"], c["J"], c["planck2"], c["lambda0"], c["c0"], c["doppler"], c["gamma"],
            c["sigma_bb_const"], c["sig1"], c["sig2"], c["T"], c["lte"], c["hc_over_kB"], c["pref_ij"], c["pref_ji"])


RATE_CASES = [("lengths", 1500, 31), ("order", 192, 32), ("damping", 350, 33), ("hot", 1536, 34), ("cold", 350, 35)]


@pytest.mark.parametrize("name,n,seed", RATE_CASES)
def test_calculate_R_hp_against_oracle(name, n, seed):
    """The extended transcription of calculate_R and the oracle agree on every rate case (1e-12 where normal, 1e-320
    absolute where subnormal, the same zeros); each case covers what it is named for."""
    c = _rate_case(name, n, seed)
    R_hp = pr.calculate_R_hp(*_R_args(c))
    _check_R(R_hp, orc.calculate_R(*_R_args(c)), name)
    lo, hi = c["blocks"][0], c["blocks"][1]
    vk, ak = pr.rates_kernel_va(c["lam"][lo:hi], c["lambda0"], c["c0"], c["doppler"], c["gamma"])
    x = c["hc_over_kB"] / (c["lam"][None, :] * c["T"][:, None])
    if name == "damping":
        reg = pr.w4_region(vk, ak)
        assert ak.max() > 0.9 and ((reg == 4) & (2 * np.abs(vk) * ak > np.pi / 4)).sum() > 100
        assert ((reg == 3) & (np.abs(vk) > 1.5)).sum() > 100
    if name == "hot":
        assert x.max() < 0.1 and x.min() < 0.005
    if name == "cold":
        b1 = slice(c["blocks"][2], c["blocks"][3])
        b2 = slice(c["blocks"][4], c["blocks"][5])
        assert x[:, b1].min() > 746 and (R_hp[:, 0, 2] == 0).all()                      # bf level 1: R_ji = 0
        # clamping the exponent at 745 instead would leave n_ratio 2^-1074 in every G of that block: nonzero R_ji
        G745 = (c["lte"][0] / c["lte"][2])[:, None] * np.exp(-745.0) * np.ones((1, b1.stop - b1.start))
        f = c["sig1"][None, :] * G745 * c["lam"][None, b1] * (c["planck2"][None, b1] + c["J"][:, b1])
        assert (c["pref_ji"] * ((f[:, 1:] + f[:, :-1]) * np.diff(c["lam"][b1])[None, :]).sum(axis=1) > 0).all()
        sub = np.abs(np.asarray(R_hp[:, 1, 2], dtype=np.float64))
        assert (sub == 0).any() and ((sub > 0) & (sub < TINY)).any() and (sub >= TINY).any()   # bf 2: all three
        assert x[:, b2].min() < 708 and x[:, b2].max() > 746


# ---- device: w4 read out exactly through the opacity kernel -----------------------------------------------
ANGLES_TH, ANGLES_PH = [120.0, 60.0], [30.0, 200.0]          # one up, one down direction


def _opacity_dev(plan, hs, lam, doppler, gamma, strength=None, velocity=None, alpha_cont=None, lambda0=1.0, c0=1.0):
    """α_tot of both angles, rows back in SITE order: (2, n, nλ)."""
    import torch
    n = hs.n
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    strength = np.sqrt(np.pi) * doppler if strength is None else strength       # the kernel's own sqrt(π) ΔλD: sp == 1
    velocity = np.zeros((n, 3)) if velocity is None else velocity
    alpha_cont = np.zeros(n) if alpha_cont is None else alpha_cont
    args = [t(velocity), t(doppler), t(gamma), t(strength), t(alpha_cont)]
    native = torch.full((plan.native_alpha_count(lam.size),), float("nan"), dtype=torch.float64, device=dev)
    plan.line_opacity_dev(lam, lambda0, c0, *(x.data_ptr() for x in args), native.data_ptr(),
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    nat = plan.native_to_site_major(native.cpu().numpy(), lam.size, 2)
    out = np.empty_like(nat)
    for a, d in enumerate((1, -1)):
        out[a][hs.storage_order(d) - 1] = nat[a]
    return out


def _straddle(v_t, a_t, delta):
    """(ΔλD, γ_lo, γ_hi): at λ = 1 + delta the kernel's fp64 (v, a) of γ_lo and of the next double γ_hi lie in
    different regions of w4 (bisection on the bit patterns of γ; the region is monotone in a)."""
    lam = np.array([1.0 + delta])
    dD = delta / v_t
    reg = lambda g: pr.w4_region(*pr.kernel_va(lam, 1.0, 1.0, np.array([dD]), np.array([g])))[0, 0]
    g0 = a_t * 4 * np.pi * dD
    lo, hi = g0 * 0.999, g0 * 1.001
    assert reg(lo) != reg(hi)
    ilo, ihi = np.float64(lo).view(np.int64), np.float64(hi).view(np.int64)
    while ihi - ilo > 1:
        mid = (ilo + ihi) // 2
        if reg(np.int64(mid).view(np.float64)) == reg(lo):
            ilo = mid
        else:
            ihi = mid
    return dD, np.int64(ilo).view(np.float64), np.int64(ihi).view(np.float64)


@pytest.fixture(scope="module")
def w4_plan(bcc_small):
    pos, nbr, bounds = bcc_small
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    plan = vrt.FormalPlan(hs, vrt.quadrature_directions(ANGLES_TH, ANGLES_PH), 3, dirs=[1 if t > 90 else -1 for t in ANGLES_TH])
    yield hs, plan
    plan.close()
    hs.close()


def _w4_grid_sites(n, rng):
    """Per storage position (up direction) ΔλD and γ, and the wavelengths: a grid over |v| <= 1e4 x a in {0, 1e-8 .. 10},
    region 4 with 2|v|a > π/4, adjacent-double pairs straddling each boundary, every site also mirrored."""
    delta_b = 2.0 ** -12                                          # the wavelength the boundary pairs are placed at
    geo = np.geomspace(1e-10, 1e-2, 24)
    lam = np.concatenate([1 - geo[::-1], [1.0], 1 + geo, [1 + delta_b]])
    pairs = []
    for v_t in (14.5, 12.0, 8.0, 5.0, 2.0, 0.5):
        pairs.append(_straddle(v_t, 15.0 - v_t, delta_b))
    for v_t in (5.3, 4.5, 3.5, 2.0, 0.5):
        pairs.append(_straddle(v_t, 5.5 - v_t, delta_b))
    for v_t in (1.0, 2.0, 3.0, 4.0, 4.5):
        pairs.append(_straddle(v_t, 0.195 * v_t - 0.176, delta_b))
    dD_b = np.repeat([p[0] for p in pairs], 2)
    g_b = np.array([g for p in pairs for g in p[1:]])
    half = n // 2 - dD_b.size
    V = 10 ** rng.uniform(-2, 4, half)                            # largest |v| of the site
    a_site = rng.choice([0.0, 1e-8, 1e-6, 1e-4, 1e-3, 1e-2, 0.03, 0.1, 0.3, 0.6, 1.0, 2.0, 5.0, 10.0], half)
    k = half // 4                                                 # a quarter: region 4 with large |2 v a|
    V[:k] = rng.uniform(2.5, 5.2, k) / 1e-2 * geo[-1]
    a_site[:k] = rng.uniform(0.2, 0.9, k)
    dD = np.concatenate([geo[-1] / V, dD_b])
    gamma = np.concatenate([a_site * 4 * np.pi * dD[:half], g_b])
    # the mirror of a site: ΔλD, γ -> -ΔλD, -γ gives v -> -v exactly and the same a (strength follows: sp stays 1)
    return lam, np.concatenate([dD, -dD]), np.concatenate([gamma, -gamma]), dD_b.size


@pytest.mark.gpu
def test_gpu_w4_read_out_over_the_domain(w4_plan):
    """vrt_line_opacity_dev with velocity 0, α_cont 0, λ0 = c0 = 1, strength sqrt(π) ΔλD: α_tot is the device's
    H(a, v) at the (v, a) kernel_va recomputes bit for bit.  Against w4_hp: 1e-12 everywhere (regions decided in fp64
    from the same v, a -- a point one double the other side of a boundary would be off by ~1e-6), exactly 0 where
    w4_hp is 0; H(a, -v) == H(a, v) to 1e-14; both angles (other storage orders, other waves) agree to 1e-14."""
    hs, plan = w4_plan
    n = hs.n
    rng = np.random.default_rng(41)
    lam, dD_pos, g_pos, nb = _w4_grid_sites(n, rng)
    npos = dD_pos.size
    order = hs.storage_order(1) - 1                               # storage position -> site
    dD, gamma = np.full(n, 1e-3), np.zeros(n)                     # (positions past 2 * half: a plain filler site)
    dD[order[:npos]], gamma[order[:npos]] = dD_pos, g_pos
    H = _opacity_dev(plan, hs, lam, dD, gamma)
    v, a = pr.kernel_va(lam, 1.0, 1.0, dD, gamma)
    reg = pr.w4_region(v, a)
    ref = np.asarray(pr.w4_hp(v, a, region=reg), dtype=np.float64)
    for ang in (0, 1):
        assert np.array_equal(H[ang] == 0, ref == 0), ang
        assert _rel_nonzero(H[ang], ref) < 1e-12, ang
    assert _rel_nonzero(H[1], H[0]) < 1e-14
    half = npos // 2
    sp, sm = order[:half], order[half:npos]
    assert np.array_equal(v[sm], -v[sp]) and np.array_equal(a[sm], a[sp])
    assert _rel_nonzero(H[0][sm], H[0][sp]) < 1e-14
    # the boundary pairs straddle their boundary in fp64 (so the 1e-12 above pins the region choice)
    lb = lam.size - 1
    bs = sp[half - nb:]
    rb = reg[bs, lb].reshape(-1, 2)
    assert (rb[:, 0] != rb[:, 1]).all()
    jump = np.abs(ref[bs, lb].reshape(-1, 2) @ np.array([1.0, -1.0])) / ref[bs, lb].reshape(-1, 2)[:, 0]
    assert (jump > 1e-12).all(), jump.min()
    # coverage and the numbers for the record
    red = (reg == 4) & (2 * np.abs(v) * a > np.pi / 4)
    assert red.sum() > 400 and (a == 0).sum() > 500 and np.abs(v).max() > 9e3 and a.max() > 9.9
    print("\nw4 device vs w4_hp: all %.2e" % _rel_nonzero(H[0], ref) +
          "".join(" | region %d %.2e (%d pts)" % (r, _rel_nonzero(H[0][reg == r], ref[reg == r]), (reg == r).sum())
                  for r in (1, 2, 3, 4)) +
          " | reduction branch %.2e (%d pts)" % (_rel_nonzero(H[0][red], ref[red]), red.sum()))


@pytest.mark.gpu
def test_gpu_w4_cos_small_branch_does_not_depend_on_the_wave(w4_plan):
    """cos_small takes its Cody-Waite branch for the whole wave when ONE region-4 lane has |2 v a| > π/4.  The same
    small-|2 v a| points in waves whose lanes all stay below π/4 and in waves with one large lane: equal to 1e-14,
    each within 1e-12 of w4_hp; the large lanes too (where the Taylor polynomial alone would miss by far more).
    Observed: equal bit for bit (for |z| < π/4 the reduction has k = 0, r = z), large lanes 1.6e-14 from w4_hp."""
    hs, plan = w4_plan
    n = hs.n
    nw = n // 64
    rng = np.random.default_rng(42)
    lam = 1 + np.linspace(1e-3, 1.25e-3, 24)                      # v spans a factor 1.25 at every site
    v0 = rng.uniform(1.2, 4.3, 64 * (nw // 2))                    # small lanes: v in [v0, 1.25 v0], 2 v a < π/4
    a0 = rng.uniform(1e-3, 0.99, v0.size) * np.pi / (8 * 1.26 * v0)
    dS, gS = 1e-3 / v0, a0 * 4 * np.pi * (1e-3 / v0)
    dL, gL = 1e-3 / 3.5, 0.4 * 4 * np.pi * (1e-3 / 3.5)          # large lane: v in [3.5, 4.4], a 0.4: 2 v a >= 2.8, region 4
    order = hs.storage_order(1) - 1
    dpos, gpos = np.full(n, 1e-3), np.zeros(n)
    h = nw // 2
    dpos[:64 * h], gpos[:64 * h] = dS, gS                         # waves 0 .. h-1: uniform
    dpos[64 * h:128 * h], gpos[64 * h:128 * h] = dS, gS           # waves h .. 2h-1: the same points, lane 17 large
    big = 64 * h + 64 * np.arange(h) + 17
    dpos[big], gpos[big] = dL, gL
    dD, gamma = np.empty(n), np.empty(n)
    dD[order], gamma[order] = dpos, gpos
    H = _opacity_dev(plan, hs, lam, dD, gamma)[0][order]          # rows by storage position (up)
    v, a = pr.kernel_va(lam, 1.0, 1.0, dpos, gpos)
    reg = pr.w4_region(v, a)
    z = 2 * np.abs(v) * a
    small = np.setdiff1d(np.arange(128 * h), big)
    assert (reg[big] == 4).all() and (z[big] > np.pi / 4).all() and (z[small] <= np.pi / 4).all()
    assert (reg[:64 * h] == 4).sum() > 1000
    ref = np.asarray(pr.w4_hp(v, a, region=reg), dtype=np.float64)
    assert _rel_nonzero(H, ref) < 1e-12
    keep = np.setdiff1d(np.arange(64 * h), big - 64 * h)
    assert _rel_nonzero(H[64 * h + keep], H[keep]) < 1e-14
    print("\ncos_small: uniform vs mixed waves %.2e, large lanes vs w4_hp %.2e"
          % (_rel_nonzero(H[64 * h + keep], H[keep]), _rel_nonzero(H[big], ref[big])))


@pytest.mark.gpu
def test_gpu_line_opacity_strong_damping_end_to_end(w4_plan):
    """A ~ 0.05 .. 1 (strong resonance line in dense layers) with velocities and α_cont, SI numbers: the device's α_tot
    against the oracle (1e-12) and against an extended transcription of α_tot (1e-12)."""
    hs, plan = w4_plan
    n = hs.n
    rng = np.random.default_rng(43)
    lambda0 = 121.567e-9
    q = np.concatenate([-np.geomspace(60, 0.05, 25), [0.0], np.geomspace(0.05, 60, 25)])
    lam = lambda0 * (1 + q * 2.5e3 / C0)
    T = rng.uniform(4e3, 2e4, n)
    doppler = lambda0 / C0 * np.sqrt(2 * K_B * T / 1.6735575e-27)
    gamma = 10 ** rng.uniform(np.log10(0.05), 0.0, n) * 4 * np.pi * C0 * doppler / lambda0 ** 2
    velocity = rng.normal(0, 8e3, (n, 3))
    strength = 10 ** rng.uniform(-3, 1, n)
    alpha_cont = 10 ** rng.uniform(-6, -2, n)
    got = _opacity_dev(plan, hs, lam, doppler, gamma, strength, velocity, alpha_cont, lambda0, C0)
    kk = vrt.quadrature_directions(ANGLES_TH, ANGLES_PH)
    for ang in (0, 1):
        k = kk[ang]
        ref = orc.line_opacity(orc.direction(ANGLES_TH[ang], ANGLES_PH[ang]), lam, lambda0, C0, velocity, doppler,
                               gamma, strength, alpha_cont)
        assert _rel_nonzero(got[ang], ref) < 1e-12
        v_los = velocity[:, 0] * (-k[0]) + velocity[:, 1] * (-k[1]) + velocity[:, 2] * (-k[2])
        vk, ak = pr.kernel_va(lam, lambda0, C0, doppler, gamma, shift=lambda0 * v_los / C0)
        e = pr.ext
        ve = (e(lam)[None, :] - e(lambda0) + e(lambda0) * (e(velocity) @ -e(k))[:, None] / e(C0)) / e(doppler)[:, None]
        ae = e(gamma)[:, None] * e(lam)[None, :] ** 2 / (4 * pr.PI * e(C0) * e(doppler)[:, None])
        Hx = pr.w4_hp(ve, ae, region=pr.w4_region(vk, ak))
        alpha_x = e(strength)[:, None] * Hx / (np.sqrt(pr.PI) * e(doppler)[:, None]) + e(alpha_cont)[:, None]
        assert _rel_nonzero(got[ang], alpha_x) < 1e-12
        assert ak.min() > 0.04 and (pr.w4_region(vk, ak) == 4).sum() > 200


# ---- device: the rate kernel at the edges -------------------------------------------------------------------
_GRIDS = {1500: lambda: synth.voronoi_grid(1500, seed=5, bounds=(0.0, 2.0, 0.0, 1.0, 0.0, 1.0), scale_height=0.7),
          192: lambda: synth.bcc_grid(4, 6, seed=3), 350: lambda: synth.bcc_grid(5, 7, seed=3),
          1536: lambda: synth.bcc_grid(8, 12, seed=2)}


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,seed", RATE_CASES)
def test_gpu_rates_at_the_edges(name, n, seed):
    """rates_populations_dev on every rate case, J with ld = nλ + 5 and NaN padding: R against calculate_R_hp and the
    oracle (same zeros, 1e-12 where normal, 1e-320 absolute where subnormal); the populations are the oracle's 2 x 2
    solve of the device's R bit for bit.  The cold case's bf level 1 has R_ji exactly 0 (before boltzmann() returned
    0 past libm's underflow it came out n_ratio 2^-1074 σ λ (P + J) Δλ, ~1e-320).  On the "order" case also
    rates_populations_native_dev, J split into up and down sweep-order planes: bit for bit the caller-layout result."""
    import torch
    pos, nbr, bounds = _GRIDS[n]()
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    assert hs.n == n
    c = _rate_case(name, n, seed)
    nlam = c["lam"].size
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    ld = nlam + 5
    Jp = np.full((n, ld), np.nan)
    Jp[:, :nlam] = c["J"]
    d_J, d_dop, d_gam, d_T, d_lte, d_C, d_atom = (t(x) for x in (Jp, c["doppler"], c["gamma"], c["T"], c["lte"], c["C"], c["atom"]))
    d_R = torch.full((n, 3, 3), float("nan"), dtype=torch.float64, device=dev)
    d_pop = torch.full((3, n), float("nan"), dtype=torch.float64, device=dev)
    tail = (c["planck2"], c["lambda0"], c["c0"], d_dop.data_ptr(), d_gam.data_ptr(), c["sigma_bb_const"], c["sig1"], c["sig2"],
            d_T.data_ptr(), d_lte.data_ptr(), c["hc_over_kB"], c["pref_ij"], c["pref_ji"], d_C.data_ptr(), d_atom.data_ptr())
    api.rates_populations_dev(hs, c["lam"], c["blocks"], ld, d_J.data_ptr(), *tail, d_R.data_ptr(), d_pop.data_ptr(), stream=st)
    torch.cuda.synchronize()
    R, pops = d_R.cpu().numpy(), d_pop.cpu().numpy()
    R_hp = pr.calculate_R_hp(*_R_args(c))
    e_hp = _check_R(R, R_hp, name + " vs calculate_R_hp")
    e_orc = _check_R(R, orc.calculate_R(*_R_args(c)), name + " vs oracle")
    assert np.array_equal(pops, orc.revised_populations(R, c["C"], c["atom"]))
    if name == "cold":
        assert (R[:, 0, 2] == 0).all()
    print(f"\nrates {name}: n {n}, max rel vs calculate_R_hp {e_hp:.2e}, vs oracle {e_orc:.2e}")
    if name == "order":
        rng = np.random.default_rng(seed)
        Ja = c["J"] * rng.uniform(0.2, 0.8, c["J"].shape)
        Jb = c["J"] - Ja
        Jsum = Ja + Jb                                            # what the kernel forms from the two planes
        w, th, ph, _ = vrt.read_quadrature("ul2n3.dat")
        plan = vrt.FormalPlan(hs, vrt.quadrature_directions(th, ph), 3, dirs=[1 if x > 90 else -1 for x in th])
        cnt = plan.native_plane_count(nlam)
        J_up, J_dn = (torch.full((cnt,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        d_Ja, d_Jb, d_Js = t(Ja), t(Jb), t(Jsum)
        plan.to_native_dev(nlam, nlam, d_Ja.data_ptr(), J_up.data_ptr(), 0, stream=st)
        plan.to_native_dev(nlam, nlam, d_Jb.data_ptr(), 0, J_dn.data_ptr(), stream=st)
        d_R2, d_R3 = (torch.full((n, 3, 3), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        d_p2, d_p3 = (torch.full((3, n), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        api.rates_populations_native_dev(hs, c["lam"], c["blocks"], J_up.data_ptr(), J_dn.data_ptr(), *tail,
                                         d_R2.data_ptr(), d_p2.data_ptr(), stream=st)
        api.rates_populations_dev(hs, c["lam"], c["blocks"], nlam, d_Js.data_ptr(), *tail, d_R3.data_ptr(), d_p3.data_ptr(),
                                  stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(d_R2.cpu().numpy(), d_R3.cpu().numpy())
        assert np.array_equal(d_p2.cpu().numpy(), d_p3.cpu().numpy())
        plan.close()
    hs.close()
