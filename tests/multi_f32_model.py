"""What tests/test_multi_f32_host.py (CPU) and tests/test_multi_f32.py (GPU) share: the rate integrals regrouped per
wavelength restated in numpy (the shares a device of vrt_multi_lambda forms for its wavelength block), the wavelength
ranges and partitions both files walk, and the small line cases.  Nothing here touches the device."""
import numpy as np

import voronoirt_amd as vrt
from oracle import oracle as orc
from voronoirt_amd import distributed

REGROUPING = 1e-12              # the figure the project gives for the regrouped sums (tests/test_physics.py, voronoirt.h)
CASES = [(3, 2), (21, 6)]       # (nbb, nbf): 7 and 33 wavelengths


def rates_case(n, seed, nbb, nbf):
    """_rates_case of tests/test_physics.py for any block sizes (an even nbb: the first nbb line wavelengths), J as the
    float32 J_up and J_down of a float session"""
    from test_physics import C0, H_PLANCK, K_B, _line_case
    c = _line_case(n, seed, nbb, nbf)
    rng = c["rng"]
    lam = np.concatenate([c["lam"][:nbb], c["lam"][c["lam"].size - 2 * nbf:]])
    nlam = lam.size
    assert nlam == nbb + 2 * nbf == c["blocks"][5]
    r = dict(lam=lam, J_up=(10 ** rng.uniform(-12, -3, (n, nlam))).astype(np.float32),
             J_down=(10 ** rng.uniform(-12, -3, (n, nlam))).astype(np.float32), planck2=2 * H_PLANCK * C0 ** 2 / lam ** 5,
             lte=np.stack([c["n_i"], c["n_j"] * 3.0, c["n_i"] * 10 ** rng.uniform(-6, 0, n)]),
             sig1=7.9e-22 * (lam[nbb:nbb + nbf] / lam[nbb + nbf - 1]) ** 3, sig2=1.4e-21 * (lam[nbb + nbf:] / lam[-1]) ** 3,
             C=10 ** rng.uniform(-2, 4, (n, 3, 3)), sigma_bb_const=H_PLANCK * C0 / (4 * np.pi * c["lambda0"]) * c["Bij"],
             hc_over_kB=H_PLANCK * C0 / K_B, pref_ij=2 * np.pi / (H_PLANCK * C0) / 1000.0, pref_ji=2 * np.pi / (H_PLANCK * C0))
    for d in range(3):
        r["C"][:, d, d] = 0.0
    r["atom"] = r["lte"].sum(axis=0) * rng.uniform(0.9, 1.1, n)
    return c, r, C0


def rates_case_of(case, seed):
    """(c, r, C0) in the form of rates_case from a vrt.LineCase (tests/test_physics.py: _lambda_case, or small_lambda_case
    below) in LTE: the atmosphere the project's 1e-12 for the populations was established on.  J_up and J_down: float32, each
    about half of B_0.  Unlike rates_case -- whose random rates leave 1e-37 of the atoms in level 2, so that the ORACLE's own
    populations move by 1.4e-12 when its R changes by 1e-15 (tests/test_multi_f32_host.py prints the figure) -- every level
    here holds a fraction of the atoms that a rounding of R does not move."""
    rng = np.random.default_rng(seed)
    B0 = np.asarray(case.B0)
    c = dict(lambda0=case.lambda0, blocks=np.asarray(case.blocks, dtype=np.int64), doppler=np.asarray(case.doppler),
             gamma=case.gamma(case.lte), T=np.asarray(case.temperature))
    r = dict(lam=np.asarray(case.lam), planck2=np.asarray(case.planck2), lte=np.asarray(case.lte), sig1=np.asarray(case.sigma_bf1),
             sig2=np.asarray(case.sigma_bf2), C=np.asarray(case.C), atom=np.asarray(case.atom_density),
             sigma_bb_const=case.sigma_bb_const, hc_over_kB=case.hc_over_kB, pref_ij=case.pref_ij, pref_ji=case.pref_ji,
             J_up=(B0 * (0.3 + 0.4 * rng.random(B0.shape))).astype(np.float32),
             J_down=(B0 * (0.3 + 0.4 * rng.random(B0.shape))).astype(np.float32))
    return c, r, case.c0


def population_sensitivity(c, r, C0, delta=1e-15, seed=0):
    """the largest relative change of the ORACLE's populations when every entry of its R changes by +-delta (relative)"""
    R = oracle_R(c, r, C0, widened_J(r["J_up"], r["J_down"]))
    p = orc.revised_populations(R, r["C"], r["atom"])
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], R.shape)
    return float(np.abs(orc.revised_populations(R * (1 + delta * sign), r["C"], r["atom"]) / p - 1).max())


def widened_J(J_up, J_down):
    """J = f32(J_up + J_down) as float64, either None: what the float kernels form from the two plane sets"""
    j = np.zeros((J_up if J_up is not None else J_down).shape)
    if J_up is not None:
        j = j + np.asarray(J_up, dtype=np.float64)
    if J_down is not None:
        j = j + np.asarray(J_down, dtype=np.float64)
    return j.astype(np.float32).astype(np.float64)


def partition(nlam, world):
    """the contiguous wavelength blocks of vrt_multi_lambda: 33 over 4 -> 9, 8, 8, 8"""
    return [distributed.partition(nlam, world, r) for r in range(world)]


def partitions(nlam):
    """[0, nlam) in 1, 2, 3 and nlam ranges"""
    return [partition(nlam, w) for w in (1, 2, 3, nlam)]


def ranges(nbb, nbf):
    """the wavelength ranges of GPU test 1 as {name: (l0, l1)}"""
    nlam = nbb + 2 * nbf
    return {
        "whole": (0, nlam),
        "one wavelength": (1, 2),
        "odd, the bound-bound block": (0, nbb),                                 # nb = 3 or 21; no bound-free wavelength
        "even, from blocks[1]": (nbb, nlam),                                    # nb = 4 or 12; no bound-bound wavelength
        "inside the bound-bound block": (1, 2) if nbb == 3 else (5, 12),        # trapezoid neighbours elsewhere on both sides
        "across two block edges": (nbb - 1, nbb + nbf + 1),
        "empty": (2, 2),
    }


def sigma_bb(c, r, c0):
    """σ_ij (n, nbb) of the bound-bound block: the site's static Voigt profile (rates.jl:374-416)"""
    lo, hi = c["blocks"][0], c["blocks"][1]
    lam = r["lam"][lo:hi]
    a = c["gamma"][:, None] * lam[None, :] ** 2 / (4 * np.pi * c0 * c["doppler"][:, None])
    v = (lam[None, :] - c["lambda0"]) / c["doppler"][:, None]
    H = np.array([[orc.humlicek_w4(v[i, j], a[i, j]).real for j in range(lam.size)] for i in range(v.shape[0])])
    return r["sigma_bb_const"] * H / (np.sqrt(np.pi) * c["doppler"][:, None])


def shares_model(c, r, J, l0, l1, sig_bb):
    """shares (6, n) of the wavelengths [l0, l1): Σ_l W_l f_l with W_l = (λ_l - λ_l-1) [l > lo] + (λ_l+1 - λ_l) [l < hi - 1]
    inside each block [lo, hi), the prefactor applied last; rows (bf1 ij, bf1 ji, bf2 ij, bf2 ji, bb ij, bb ji).
    J: (n, nlam), ALL wavelengths (only columns [l0, l1) are read)."""
    lam, n = r["lam"], J.shape[0]
    out = np.zeros((6, n))
    for tr in range(3):
        b = 2 * (tr + 1) if tr < 2 else 0
        lo, hi = int(c["blocks"][b]), int(c["blocks"][b + 1])
        ratio = r["lte"][tr] / r["lte"][2] if tr < 2 else r["lte"][0] / r["lte"][1]
        rij, rji = np.zeros(n), np.zeros(n)
        for l in range(max(lo, l0), min(hi, l1)):
            s = (r["sig1"], r["sig2"])[tr][l - lo] if tr < 2 else sig_bb[:, l - lo]
            G = ratio * np.exp(-r["hc_over_kB"] / (lam[l] * c["T"]))
            W = (lam[l] - lam[l - 1] if l > lo else 0.0) + (lam[l + 1] - lam[l] if l < hi - 1 else 0.0)
            rij += (lam[l] * s * J[:, l]) * W
            rji += (s * G * lam[l] * (r["planck2"][l] + J[:, l])) * W
        out[2 * tr], out[2 * tr + 1] = r["pref_ij"] * rij, r["pref_ji"] * rji
    return out


def R_of_shares(shares):
    """R (n, 3, 3) in the oracle's layout (R[:, c, r] = Julia R[r + 1, c + 1, :]) from summed shares (6, n)"""
    R = np.zeros((shares.shape[1], 3, 3))
    for lev in (1, 2):
        R[:, 2, lev - 1] = shares[2 * (lev - 1)]
        R[:, lev - 1, 2] = shares[2 * (lev - 1) + 1]
    R[:, 1, 0], R[:, 0, 1] = shares[4], shares[5]
    return R


TRANSITIONS = [(2, 0), (0, 2), (2, 1), (1, 2), (1, 0), (0, 1)]      # the six entries of R[:, c, r] that hold a rate


def rel_per_transition(R, R_ref):
    """the largest relative difference of each of the six rates over the sites; every other entry must be equal"""
    mask = np.ones((3, 3), dtype=bool)
    out = []
    for cc, rr in TRANSITIONS:
        mask[cc, rr] = False
        out.append(float(np.abs(R[:, cc, rr] / R_ref[:, cc, rr] - 1).max()))
    assert np.array_equal(R[:, mask], R_ref[:, mask])
    return out


def oracle_R(c, r, c0, J):
    return orc.calculate_R(r["lam"], c["blocks"], J, r["planck2"], c["lambda0"], c0, c["doppler"], c["gamma"],
                           r["sigma_bb_const"], r["sig1"], r["sig2"], c["T"], r["lte"], r["hc_over_kB"], r["pref_ij"],
                           r["pref_ji"])


def small_lambda_case(pos, bounds, seed):
    """_lambda_case of tests/test_physics.py with nbb = 2, nbf = 2: six wavelengths (the first two line wavelengths -- the
    far blue wing and the line centre -- and two per bound-free block)"""
    from test_physics import C0, H_PLANCK, K_B, _line_case
    n = pos.shape[0]
    c = _line_case(n, seed, nbb=2, nbf=2)
    rng = c["rng"]
    lam = np.concatenate([c["lam"][:2], c["lam"][c["lam"].size - 4:]])
    nlam = lam.size
    assert nlam == 6 and (np.diff(lam[:2]) > 0).all()
    z = (pos[:, 0] - bounds[0]) / (bounds[1] - bounds[0])
    T = 6e3 + 6e3 * z + 200 * rng.random(n)
    doppler = c["lambda0"] / C0 * np.sqrt(2 * K_B * T / 1.6735575e-27)
    n1 = 1e16 * np.exp(-3 * z) * (1 + 0.1 * rng.random(n))
    lte = np.stack([n1, n1 * 1e-3 * (1 + rng.random(n)), n1 * 1e-2 * (1 + rng.random(n))])
    B0 = (1.0 + z)[:, None] * (1 + 0.05 * rng.random((n, nlam)))
    Cm = 10 ** rng.uniform(-1, 1, (n, 3, 3))
    for d in range(3):
        Cm[:, d, d] = 0.0
    box = bounds[1] - bounds[0]
    Bij = 1.0
    strength_const = 60.0 / box * doppler.mean() / n1.mean()
    return vrt.LineCase(
        lam=lam, blocks=c["blocks"], lambda0=c["lambda0"], c0=C0, velocity=rng.normal(0, 3e3, (n, 3)), doppler=doppler,
        gamma_static=4.702e8 + 10 ** rng.uniform(7, 8.7, n), gamma_unsold=10 ** rng.uniform(-8.5, -7.5, n),
        alpha_cont=0.05 / box * np.exp(-2 * z), eps=10 ** rng.uniform(-2.5, -0.5, n),
        temperature=T, atom_density=lte.sum(axis=0), B0=B0, lte=lte, C=Cm, planck2=2.0 * (c["lambda0"] / lam) ** 5,
        sigma_bf1=1e-21 * (lam[2:4] / lam[3]) ** 3, sigma_bf2=2e-21 * (lam[4:6] / lam[5]) ** 3,
        strength_const=strength_const, Bij=Bij, Bji=0.25 * Bij, sigma_bb_const=2e-32,
        hc_over_kB=H_PLANCK * C0 / K_B, pref_ij=2e36, pref_ji=2e37)
