"""The inputs of tests/test_synthesis_domain.py (GPU), shown on the CPU to be what they claim to be.

k_tau_unity decides, per plane, a cell (floor of the lateral offset, wrapped with fmod) and a fraction, and per column
the FIRST minimum of |tau - 1| from the top.  The reference is oracle/synth_ref.py: the algorithm in exact rational
arithmetic with a derived forward-error bound B; a column's answer must be one of the planes within 2 B of the exact
minimum (its candidates), and a column with one candidate is decided by the reference alone.  The rasters and
directions below put columns on every decision: all eight octants, exactly zero lateral components, offsets of many
periods, offsets on and beside integers (k = (-a, a, 0) on a raster with unit spacings), nx = 2 / ny = 2, a launch
with a partial last workgroup, dyadic columns whose tau is exact in fp64 (an exact 1.0, exact ties, an opaque first
step, a transparent column) and non-finite alpha in the column and beside it.

`kernel_tau` is a numpy transcription of the kernel's statement order (the library is built with -ffp-contract=off);
it passes the candidate check everywhere, and five mutations of it each fail somewhere: that is what shows that the
inputs can tell a wrong kernel from a right one (no mutation runs on the GPU).

The second half builds the field domain of k_synth_opacity as named cases and its shapes and wavelength counts."""
import functools

import numpy as np
import pytest

from oracle import synth_ref as ref
from voronoirt_amd import synth

# ---- tau = 1: rasters -------------------------------------------------------------------------------------------------------
SCALES = (0.05, 1.0, 30.0)          # vertical tau of the whole height about 0.13 (never reaches 1), 2.6 and 78
# (nz, nx, ny, nlam): 7 x 5 x 8 = 280 columns: two workgroups of 256 threads, the second partial
TAU_SHAPES = ((7, 2, 2, 3), (12, 5, 3, 3), (9, 3, 7, 4), (12, 7, 5, 8))


class TauRaster:
    def __init__(self, name, z, x, y, alpha):
        self.name, self.z, self.x, self.y = name, z, x, y
        self.alpha = alpha                                           # interior (nlam, ny, nx, nz)
        self.dx = (x[-1] - x[0]) / (x.size - 1)                      # uniform_spacing (csrc/vrt_synth.hip)
        self.dy = (y[-1] - y[0]) / (y.size - 1)
        alpha.setflags(write=False)

    @property
    def ghosted(self):
        return np.pad(self.alpha, [(0, 0), (1, 1), (1, 1), (0, 0)], mode="wrap")


def _atmosphere_tau_raster(nz, nx, ny, nlam):
    atm = synth.atmosphere_raster(nz, nx, ny, seed=3)
    z = atm["z"]
    base = 30.0 / (z[-1] - z[0]) * atm["N_H"] / atm["N_H"].max()     # alpha_cont of synth.line_raster
    rng = np.random.default_rng(100 * nx + ny)
    alpha = np.stack([SCALES[l % 3] * (1.0 + 0.25 * (l // 3)) * base * 2.0 ** rng.uniform(-1.0, 1.0, (ny, nx))[:, :, None]
                      for l in range(nlam)])
    return TauRaster("atm%dx%dx%d" % (nz, nx, ny), z, atm["x"], atm["y"], np.ascontiguousarray(alpha))


def _cubic_tau_raster():
    """integer z, unit spacings: at k = (-a, a, 0) the exact offsets are the integers z_top - z"""
    rng = np.random.default_rng(77)
    z = np.array([0.0, 1.0, 2.0, 4.0, 5.0, 7.0])
    alpha = 10.0 ** rng.uniform(-2.0, 0.5, (3, 3, 4, z.size))
    return TauRaster("cubic6x4x3", z, np.arange(4.0), np.arange(3.0), alpha)


@functools.lru_cache(maxsize=None)
def tau_rasters():
    out = {r.name: r for r in [_atmosphere_tau_raster(*s) for s in TAU_SHAPES]}
    out["cubic6x4x3"] = _cubic_tau_raster()
    return out


# ---- tau = 1: directions ------------------------------------------------------------------------------------------------------
THETAS_UP = (180.0, 179.9999, 150.0, 135.0, 130.0, 100.0, 91.0, 90.5)
QUADRANTS = (35.0, 125.0, 215.0, 305.0)
A_DIAG = float(np.float64(1.0) / np.sqrt(np.float64(2.0)))


def _k(theta, phi):
    t, p = np.radians(theta), np.radians(phi)
    return np.array([np.cos(t), np.sin(t) * np.cos(p), np.sin(t) * np.sin(p)])


@functools.lru_cache(maxsize=None)
def tau_directions():
    """[(label, k)]: every theta in the four lateral quadrants with k_z < 0, its mirror image theta' = 180 - theta
    (k_z > 0) in one quadrant each, exactly zero k_x or k_y, and the diagonals of the cubic raster"""
    out = []
    for th in THETAS_UP:
        for ph in QUADRANTS:
            out.append(("t%.7g_p%g" % (th, ph), _k(th, ph)))
    for i, th in enumerate(THETAS_UP):
        out.append(("t%.7g_p%g" % (180.0 - th, QUADRANTS[i % 4]), _k(180.0 - th, QUADRANTS[i % 4])))
    for th in (150.0, 100.0, 30.0):
        c, s = np.cos(np.radians(th)), np.sin(np.radians(th))
        out.append(("t%g_kx0" % th, np.array([c, 0.0, -s if th == 100.0 else s])))
        out.append(("t%g_ky0" % th, np.array([c, s if th == 100.0 else -s, 0.0])))
    return out


DIAGONALS = [("diag-a+a0", np.array([-A_DIAG, A_DIAG, 0.0])), ("diag-a-a0", np.array([-A_DIAG, -A_DIAG, 0.0])),
             ("diag+a0+a", np.array([A_DIAG, 0.0, A_DIAG])), ("diag-a0-a", np.array([-A_DIAG, 0.0, -A_DIAG]))]


def tau_pairs():
    """[(raster name, direction label, k)] of the inclined domain"""
    out = []
    for name in tau_rasters():
        dirs = list(tau_directions())
        if name.startswith("cubic"):
            dirs = DIAGONALS + [d for d in dirs if d[0] in ("t135_p35", "t135_p215", "t130_p125", "t91_p305", "t50_p35")]
        out += [(name, label, k) for label, k in dirs]
    return out


@functools.lru_cache(maxsize=None)
def tau_reference(name, label):
    """(exact tau, B, candidates per column) of one (raster, direction): computed once, shared, never written to"""
    ra = tau_rasters()[name]
    k = dict(tau_directions() + DIAGONALS)[label]
    tau, B = ref.tau_exact(ra.alpha, ra.z, ra.dx, ra.dy, k)
    return tau, B, ref.tau_candidates(tau, B)


# ---- the kernel's statement order in numpy ----------------------------------------------------------------------------------
MUTATIONS = ("le", "trunc", "swap_txty", "own_step", "flip_kx")
# the two departures from write_tau_unity(DATA) that the kernel had before the non-finite cases were run: `d < best`
# never accepts a NaN (the best finite plane above it was returned), and a zero fraction still blended with the
# neighbouring column (q + 0 (q' - q) is NaN for a NaN or Inf q')
FORMER = ("no_latch", "blend_always")


def kernel_tau(alpha, z, dx, dy, k, mutation=None):
    """k_tau_unity (csrc/vrt_synth.hip) statement by statement in fp64, all columns at once: alpha INTERIOR
    (nlam, ny, nx, nz).  Returns (arg planes (nlam, ny, nx), tau (nlam, ny, nx, nz) by plane)."""
    alpha = np.asarray(alpha, dtype=np.float64)
    nl, ny, nx, nz = alpha.shape
    kz, kx, ky = (float(v) for v in k)
    if mutation == "flip_kx":
        kx = -kx
    IY, IX = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    z = np.asarray(z, dtype=np.float64)
    z_top, akz = z[nz - 1], abs(kz)

    def cell(u, i, n):
        f = np.trunc(u) if mutation == "trunc" else np.floor(u)
        t = u - f
        i0 = (i + int(np.fmod(f, float(n)))) % n
        return i0, np.where(i0 + 1 == n, 0, i0 + 1), t
    prev = alpha[..., nz - 1].copy()
    tau = np.zeros((nl, ny, nx))
    best = np.ones((nl, ny, nx))
    arg = np.full((nl, ny, nx), nz - 1, dtype=np.int64)
    latched = np.zeros((nl, ny, nx), dtype=bool)
    taus = np.zeros(alpha.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for iz in range(nz - 2, -1, -1):
            r = abs((z[iz + 1] - z[iz]) / kz)
            s = r if mutation == "own_step" else (z_top - z[iz]) / akz
            i0, i1, tx = cell(s * kx / dx, IX, nx)
            j0, j1, ty = cell(s * ky / dy, IY, ny)
            if mutation == "swap_txty":
                tx, ty = ty, tx
            P = alpha[..., iz]

            def along_x(j):
                q0 = P[:, j, i0]
                return q0 + tx * (P[:, j, i1] - q0) if tx != 0.0 or mutation == "blend_always" else q0
            f0 = along_x(j0)
            a = f0 + ty * (along_x(j1) - f0) if ty != 0.0 or mutation == "blend_always" else f0
            tau = tau + 0.5 * r * (a + prev)
            d = np.abs(tau - 1.0)
            nan = np.isnan(d) & ~latched & (mutation != "no_latch")  # the first NaN is the minimum (Julia's argmin)
            arg[nan] = iz
            latched |= nan
            better = ((d <= best) if mutation == "le" else (d < best)) & ~latched
            best = np.where(better, d, best)
            arg[better] = iz
            prev = a
            taus[..., iz] = tau
    return arg, taus


def in_candidates(arg, cands):
    """per column (flattened (nlam, ny, nx)): is the returned plane one of the candidates"""
    return np.array([int(a) in c for a, c in zip(arg.ravel(), cands)])


def test_tau_domain_is_decided_by_the_reference_alone():
    """>= 99 % of the columns of every (raster, direction) have one candidate; the transcription stays inside 0.1 B."""
    pairs = tau_pairs()
    assert len(pairs) < 250
    worst_share, worst_err, periods, negative, octants = 0.0, 0.0, 0.0, False, set()
    for name, label, k in pairs:
        ra = tau_rasters()[name]
        tau, B, cands = tau_reference(name, label)
        undecided = np.mean([len(c) > 1 for c in cands])
        arg, taus = kernel_tau(ra.alpha, ra.z, ra.dx, ra.dy, k)
        exact = np.array([float(t) for t in tau.ravel()]).reshape(tau.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.nanmax(np.where(B > 0, np.abs(taus - exact) / B, 0.0))
        s = (ra.z[-1] - ra.z[0]) / abs(k[0])
        periods = max(periods, abs(s * k[1] / ra.dx) / ra.x.size, abs(s * k[2] / ra.dy) / ra.y.size)
        negative |= bool(k[1] < 0 or k[2] < 0)
        octants.add(tuple(np.sign(k).astype(int)))
        if undecided > 0 or err > 0.05:
            print("tau domain %-12s %-14s: undecided share %.4f, transcription |tau - exact| / B %.3f" % (name, label, undecided, err))
        worst_share, worst_err = max(worst_share, undecided), max(worst_err, err)
        assert undecided <= 0.01, (name, label, undecided)
        assert in_candidates(arg, cands).all(), (name, label)
    print("tau domain: %d (raster, direction) pairs, worst undecided share %.4f, worst transcription error %.3f B, "
          "offsets up to %.1f periods" % (len(pairs), worst_share, worst_err, periods))
    assert worst_err < 1.0                                           # the bound holds for the fp64 evaluation
    assert periods > 3 and negative
    assert len({o for o in octants if 0 not in o}) == 8              # all four lateral quadrants, both signs of k_z
    assert any(o[1] == 0 for o in octants) and any(o[2] == 0 for o in octants)


def test_tau_directions_are_what_they_claim():
    for label, k in tau_directions() + DIAGONALS:
        assert abs(np.sqrt((k * k).sum()) - 1.0) < 1e-6 and k[0] != 0.0, label           # tau_checks
    ks = dict(tau_directions())
    assert ks["t150_kx0"][1] == 0.0 and ks["t150_ky0"][2] == 0.0
    assert 0 < abs(ks["t180_p35"][1]) < 1e-15                        # the rounding residue of sin(pi)
    # k = (-a, a, 0) on the cubic raster: the exact offsets are the integers z_top - z; fp64 lands on or just below
    ra = tau_rasters()["cubic6x4x3"]
    k = DIAGONALS[0][1]
    u = np.array([(ra.z[-1] - zz) / abs(k[0]) * k[1] / ra.dx for zz in ra.z[:-1]])
    whole = np.array([ra.z[-1] - zz for zz in ra.z[:-1]])
    print("cubic raster, k = (-a, a, 0): fp64 offsets - integers", (u - whole).tolist())
    assert np.all(np.abs(u - whole) < 1e-14)
    assert np.any(u == whole)                                        # on an integer: floor(u) = u, fraction 0
    sizes = {(r.x.size, r.y.size) for r in tau_rasters().values()}
    assert {(2, 2), (5, 3), (3, 7), (7, 5)} <= sizes
    big = tau_rasters()["atm12x7x5"]
    assert 256 < big.alpha[..., 0].size < 512                        # a partial last workgroup


# ---- dyadic vertical columns: fp64 is exact ---------------------------------------------------------------------------------
# alpha top-down in eighths on z = 0..4 (steps 1): tau_j = sum 0.5 (a_j + a_j-1);  expected plane iz (4 = top)
DYADIC = (("hits_one", (0.5, 0.5, 0.5, 0.5, 0.5), 2),               # tau 0, .5, 1.0: exactly 1
          ("tie_half", (0.5, 0.5, 1.5, 1.0, 1.0), 3),               # tau 0, .5, 1.5: |tau - 1| ties, the upper plane wins
          ("first_is_2", (2.0, 2.0, 2.0, 2.0, 2.0), 4),             # tau 0, 2: ties with the top, the top stays
          ("first_gt_2", (3.0, 3.0, 3.0, 3.0, 3.0), 4),             # opaque in the first step
          ("all_zero", (0.0, 0.0, 0.0, 0.0, 0.0), 4),               # every plane ties, the top stays
          ("transparent", (0.125, 0.125, 0.125, 0.125, 0.125), 0))  # tau_bottom = .5: the bottom plane is closest


@functools.lru_cache(maxsize=None)
def dyadic_raster():
    """one wavelength per case; column (0, 0) carries the case, the other three columns random eighths"""
    rng = np.random.default_rng(5)
    z = np.arange(5.0)
    alpha = rng.integers(0, 17, (len(DYADIC), 2, 2, 5)) / 8.0
    for c, (_, prof, _) in enumerate(DYADIC):
        alpha[c, 0, 0, ::-1] = prof
    return TauRaster("dyadic", z, np.arange(2.0), np.arange(2.0), alpha)


@pytest.mark.parametrize("kz", [-1.0, 1.0])
def test_dyadic_columns_are_exact_and_tied_as_claimed(kz):
    ra = dyadic_raster()
    k = np.array([kz, 0.0, 0.0])
    tau, B = ref.tau_exact(ra.alpha, ra.z, ra.dx, ra.dy, k)
    arg_exact = ref.first_argmin(tau)
    arg, taus = kernel_tau(ra.alpha, ra.z, ra.dx, ra.dy, k)
    assert np.array_equal(taus, np.array([float(t) for t in tau.ravel()]).reshape(tau.shape))
    assert all(float(t) == t for t in tau.ravel())                   # fp64 holds every tau exactly
    assert np.array_equal(arg, arg_exact)
    for c, (name, _, want) in enumerate(DYADIC):
        assert arg_exact[c, 0, 0] == want, name
    d = ref.abs_tau_minus_one(tau)
    assert d[1, 0, 0, 3] == d[1, 0, 0, 2] == 0.5 and tau[0, 0, 0, 2] == 1 and tau[2, 0, 0, 3] == 2
    ties = [len(c) for c in ref.tau_candidates(tau, B)]
    assert max(ties) >= 5                                            # (the candidate rule alone does not pin a tie)


# ---- non-finite alpha, vertical ------------------------------------------------------------------------------------------------
NONFINITE = (("nan_top", (1, 1, 4), np.nan), ("nan_middle", (1, 1, 2), np.nan), ("nan_bottom", (1, 1, 0), np.nan),
             ("nan_beside_x", (1, 2, 2), np.nan), ("nan_beside_y", (2, 1, 2), np.nan),
             ("inf_beside_x", (1, 2, 3), np.inf), ("inf_beside_y", (2, 1, 3), np.inf))


@functools.lru_cache(maxsize=None)
def nonfinite_raster():
    """one wavelength per case on a 3 x 3 raster; wavelength 7 is the clean raster.  (iy, ix, iz) of the bad node: the
    centre column (1, 1), or the column the centre's i1 / j1 point at."""
    rng = np.random.default_rng(6)
    z = np.array([0.0, 0.5, 1.5, 2.0, 3.0])
    clean = rng.uniform(0.5, 0.9, (3, 3, 5))
    alpha = np.stack([clean] * (len(NONFINITE) + 1))
    for c, (_, (iy, ix, iz), v) in enumerate(NONFINITE):
        alpha[c, iy, ix, iz] = v
    return TauRaster("nonfinite", z, np.arange(3.0), np.arange(3.0), alpha)


@pytest.mark.parametrize("kz", [-1.0, 1.0])
def test_nonfinite_columns_follow_argmin_and_stay_in_their_column(kz):
    ra = nonfinite_raster()
    k = np.array([kz, 0.0, 0.0])
    tau, B = ref.tau_exact(ra.alpha, ra.z, ra.dx, ra.dy, k)
    want = ref.first_argmin(tau)
    clean = want[-1]
    assert 1 <= clean[1, 1] <= 2                                     # tau = 1 lies inside: every NaN case moves the answer
    assert want[0, 1, 1] == 3 and want[1, 1, 1] == 2 and want[2, 1, 1] == 0   # the first plane whose tau is NaN
    # numpy's argmin says the same (it takes the first NaN as Julia's does)
    for c in range(3):
        t = np.array([float(v) for v in tau[c, 1, 1, ::-1]])
        assert 4 - int(np.argmin(np.abs(t - 1.0))) == want[c, 1, 1]
    for c, (name, (iy, ix, iz), v) in enumerate(NONFINITE):
        if "beside" in name:
            assert want[c, 1, 1] == clean[1, 1]                      # the centre column computes from its own values
            assert want[c, iy, ix] == (iz if np.isnan(v) else 4)     # the bad column: its first NaN; Inf: the top stays
    arg, _ = kernel_tau(ra.alpha, ra.z, ra.dx, ra.dy, k)
    assert np.array_equal(arg, want)
    with pytest.raises(ValueError):
        ref.tau_exact(ra.alpha, ra.z, ra.dx, ra.dy, _k(130.0, 35.0))


# ---- the inputs tell a wrong kernel from a right one ----------------------------------------------------------------------
@pytest.mark.parametrize("mutation", MUTATIONS + FORMER)
def test_each_mutation_of_the_transcription_is_rejected(mutation):
    failed = []
    for name, label, k in tau_pairs():
        ra = tau_rasters()[name]
        arg, _ = kernel_tau(ra.alpha, ra.z, ra.dx, ra.dy, k, mutation)
        bad = int((~in_candidates(arg, tau_reference(name, label)[2])).sum())
        if bad:
            failed.append((name, label, bad))
    for ra, check in ((dyadic_raster(), True), (nonfinite_raster(), True)):
        for kz in (-1.0, 1.0):
            k = np.array([kz, 0.0, 0.0])
            arg, _ = kernel_tau(ra.alpha, ra.z, ra.dx, ra.dy, k, mutation)
            want = ref.first_argmin(ref.tau_exact(ra.alpha, ra.z, ra.dx, ra.dy, k)[0])
            if not np.array_equal(arg, want):
                failed.append((ra.name, "kz%+g" % kz, int((arg != want).sum())))
    print("mutation %-12s: rejected by %d cases, e.g. %s" % (mutation, len(failed), failed[:3]))
    assert failed
    if mutation in FORMER:                                           # identical wherever alpha is finite
        assert {f[0] for f in failed} == {"nonfinite"}


# ---- k_synth_opacity: shapes, wavelength counts, field domain -------------------------------------------------------------
SYNTH_SHAPES = ((3, 2, 2), (5, 3, 1), (4, 1, 3), (9, 5, 4))          # (nz, nx, ny); 9 x 7 x 6 = 378 ghosted: two workgroups
SEAM_NLAM = (31, 32, 33, 65)                                          # kSynthLam = 32 wavelengths per launch
SHAPE_NLAM = dict(zip(SYNTH_SHAPES, (65, 31, 32, 33)))


@functools.lru_cache(maxsize=None)
def synth_problem(shape, nlam, seed=3):
    """(raster, pops, case, src) of synth.line_raster on an atmosphere of (nz, nx, ny) points; nx = 1 or ny = 1 is
    the first row of a two-row atmosphere"""
    nz, nx, ny = shape
    atm = synth.atmosphere_raster(nz, max(nx, 2), max(ny, 2), seed=seed)
    for name in ("N_H", "T", "vx", "vy", "vz"):
        atm[name] = np.ascontiguousarray(atm[name][:ny, :nx])
    atm["x"], atm["y"] = atm["x"][:nx], atm["y"][:ny]
    return synth.line_raster(atm, nlam, seed=seed)


def _variant(base, **changes):
    raster, pops, case, src = base
    raster = dict(raster)
    pops = pops.copy()
    for name, v in changes.items():
        if name == "n1":
            pops[0] = v
        elif name == "n2":
            pops[1] = v
        else:
            raster[name] = v
    return raster, pops, case, src


@functools.lru_cache(maxsize=None)
def synth_cases():
    """{name: (raster, pops, case, src)} on a 4 x 3 x 2 raster with 7 wavelengths"""
    base = synth_problem((4, 3, 2), 7)
    raster, pops, case, src = base
    n1, n2 = pops
    rng = np.random.default_rng(9)
    zero = n1.copy()
    zero[0, :2, 1:3] = 0.0                                           # four of the 24 points
    return {
        "smooth": base,
        "alpha_c_zero": _variant(base, alpha_cont=np.zeros_like(raster["alpha_cont"])),
        "negative_strength": _variant(base, n2=8.0 * n1),             # n2 Bji = 2 n1 Bij;  g n1/n2 = 0.5
        "g_ratio_near_one": _variant(base, n2=4.0 * n1 * (1.0 - 2.0 ** -8)),
        "n2_zero": _variant(base, n2=np.zeros_like(n2)),
        "n1_n2_zero": _variant(base, n1=zero, n2=np.where(zero == 0.0, 0.0, n2)),
        "coronal": _variant(base, temperature=10.0 ** rng.uniform(6.0, 7.0, n1.shape)),
        "shifted": _variant(base, velocity=300.0 * raster["velocity"]),
    }


def synth_hp(problem, k):
    """(alpha_tot, S, kappa), each (nlam, ny, nx, nz) interior, of oracle/synth_ref.synth_point_hp"""
    raster, pops, case, src = problem
    shape = raster["temperature"].shape
    n = raster["temperature"].size
    vel = np.asarray(raster["velocity"]).reshape(3, n).T
    A, S, K = ref.synth_point_hp(k, case.lam, case.planck2, case, src, 4.0, vel, raster["doppler"], raster["gamma_static"],
                                 raster["gamma_unsold"], raster["temperature"], raster["alpha_cont"], pops[0], pops[1])
    back = lambda a: np.ascontiguousarray(a.T).reshape((case.lam.size,) + shape)
    return back(A), back(S), back(K)


SYNTH_K = _k(130.0, 35.0)


@functools.lru_cache(maxsize=None)
def synth_case_hp(name):
    out = synth_hp(synth_cases()[name], SYNTH_K)
    for a in out:
        a.setflags(write=False)
    return out


def rel_err(got, want):
    """element-wise |got / want - 1| over the finite, non-zero elements of want (0 where want is 0 and got is 0)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got - want) / np.abs(want)
    e = np.where((want == 0) & (got == 0), 0.0, e)
    return np.where(np.isfinite(want), e, 0.0)


def test_synth_cases_are_what_they_claim():
    cases = synth_cases()
    raster, pops, case, src = cases["smooth"]
    g = 4.0
    strength = lambda p: case.Bij * p[0] - case.Bji * p[1]
    assert (cases["alpha_c_zero"][0]["alpha_cont"] == 0).all()
    assert (strength(cases["negative_strength"][1]) < 0).all() and (strength(pops) > 0).all()
    ratio = g * cases["g_ratio_near_one"][1][0] / cases["g_ratio_near_one"][1][1]
    assert np.all((ratio > 1.0) & (ratio < 1.005))
    assert (cases["n2_zero"][1][1] == 0).all()
    p = cases["n1_n2_zero"][1]
    assert ((p[0] == 0) & (p[1] == 0)).sum() == 4 and ((p[0] == 0) == (p[1] == 0)).all()
    T = cases["coronal"][0]["temperature"]
    x = case.hc_over_kB / (case.lam[:, None, None, None] * T[None])
    assert T.min() >= 1e6 and x.max() < 0.06                         # exp(x) - 1 loses at least 1/x = 17 ulps
    vel = cases["shifted"][0]["velocity"]
    v_los = -(vel * SYNTH_K[:, None, None, None]).sum(axis=0)
    widths = np.abs(case.lambda0 * v_los / case.c0 / raster["doppler"])
    assert widths.max() > 30 and np.median(widths) > 5               # many Doppler widths
    for name in cases:
        A, S, K = synth_case_hp(name)
        print("synth case %-18s: kappa %.3g .. %.3g, non-finite S %d, alpha_tot < 0: %d" %
              (name, K.min(), K.max(), int((~np.isfinite(S)).sum()), int((A < 0).sum())))
    assert synth_case_hp("smooth")[2].max() <= 100
    assert synth_case_hp("coronal")[2].max() > 15
    assert (synth_case_hp("negative_strength")[0] < 0).any()
    assert np.isnan(synth_case_hp("n1_n2_zero")[1]).sum() == 4 * case.lam.size
    assert np.isfinite(synth_case_hp("n1_n2_zero")[0]).all()
    assert np.isfinite(synth_case_hp("n2_zero")[1]).all()


def test_synth_point_hp_agrees_with_the_oracle_restatement():
    """on the smooth atmosphere the fp64 restatement of plotter with the C oracle's alpha_line (`_plotter` of
    tests/test_synthesis.py) is within the 1e-12 contract of the 40-digit evaluation"""
    from test_synthesis import _plotter
    raster, pops, case, src = synth_cases()["smooth"]
    A, S, K = synth_case_hp("smooth")
    S64, A64 = _plotter(SYNTH_K, raster, pops, case, src)
    eA, eS = rel_err(A64, A).max(), rel_err(S64, S).max()
    print("smooth atmosphere, oracle restatement against 40 digits: alpha_tot %.3e, S %.3e, kappa <= %.3g" % (eA, eS, K.max()))
    assert eA < 1e-12 and eS < 1e-12


def test_synth_shapes_and_wavelength_counts():
    for shape in SYNTH_SHAPES:
        raster, pops, case, src = synth_problem(shape, SHAPE_NLAM[shape])
        nz, nx, ny = shape
        assert raster["temperature"].shape == (ny, nx, nz) and pops.shape == (2, ny, nx, nz)
        assert case.lam.size == SHAPE_NLAM[shape] and raster["velocity"].shape == (3, ny, nx, nz)
    assert sorted(SHAPE_NLAM.values()) == sorted(SEAM_NLAM)
    assert any(s[1] == 1 for s in SYNTH_SHAPES) and any(s[2] == 1 for s in SYNTH_SHAPES)
    nz, nx, ny = SYNTH_SHAPES[-1]
    assert nz * (nx + 2) * (ny + 2) == 378 > 256
    assert {n < 32 for n in SEAM_NLAM} == {True, False} and 32 in SEAM_NLAM and max(SEAM_NLAM) > 64
