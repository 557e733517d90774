"""The inputs of tests/test_regular_domain.py (GPU), shown on the CPU oracle to be what they claim to be.

The regular-grid solver decides three things from a direction k = (k_z, k_x, k_y): the marching signs and the
interpolation offsets (xy_intersect, functions.jl:430-457: four strict quadrant tests and an `else` that takes
sign_x = sign_y = +1 whenever a horizontal component is exactly zero), and per plane the kind of kernel,
cut = argmin(r_z, r_x, r_y) with the FIRST minimum winning (characteristics.jl:72).  The direction set below puts a
solve on every one of those decisions: exact zeros, the +-1e-16 residues that direction(theta, phi) leaves at
phi = 90, 180, 270, exact ties of two or three r values in all eight octants (a raster with bit-equal spacings), one
ulp either side of each tie, near-grazing rays, and a z axis whose steps change the kind from plane to plane.

Every horizontal pattern runs as an up solve (k_z < 0: k points upwind, the rays travel up) and as a down solve
(k_z > 0).  Fields are those of `_random_problem` of tests/test_regular.py (alpha log-uniform over six decades, random
S, non-periodic ghosts, nx != ny).

The second half is the shape table of the launch forms (derived from the inequalities of `regular_launch`,
csrc/vrt_regular.hip) and a known answer with a non-constant source function."""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as orc
from test_regular import _random_problem

H = 0.125                                   # spacing of the tie raster: x, y and z steps bit-equal
TINY = 1e-15                                # |component| below this is a rounding residue of direction()


def solve_oracle(k, up, S, I0, al, z, x, y, n_sweeps, return_planes=False):
    f = orc.short_characteristics_up if up else orc.short_characteristics_down
    return f(np.asarray(k, dtype=np.float64), S, I0, al, z, x, y, n_sweeps, return_planes=return_planes)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum())


class Case:
    """One solve: class label, direction, up flag, the plane kinds it was built for (1 xy, 2 yz, 3 xz; a set, or the
    whole sequence for the mixed raster), `pair`: label of the case whose I_0 it shares and is compared with."""

    def __init__(self, cls, label, k, kinds, pair=None, differs=None, tie=None):
        self.cls, self.label, self.k = cls, label, np.asarray(k, dtype=np.float64)
        self.up = bool(self.k[0] < 0)
        self.kinds, self.pair, self.differs, self.tie = kinds, pair, differs, tie

    def __repr__(self):
        return "%s[%s] k=(%r, %r, %r) %s" % ((self.cls, self.label) + tuple(float(v) for v in self.k) + ("up" if self.up else "down",))


# ---- raster G: the generic random raster -- exact zeros, rounding residues, near-grazing rays ------------------------
# 9 x 12 x 10 of _random_problem: dx = 1/11 = 0.0909, dy = 1.3/9 = 0.1444, dz in [0.055, 0.167].
#   theta = 100 / 80 (|k_z| = 0.174, horizontal 0.985): r_z >= 0.32; along x r_x = 0.092 -> yz; along y r_y = 0.147 -> xz
#   theta = 170 / 10 (|k_z| = 0.985, horizontal 0.174): r_z <= 0.17 < r_x = 0.52, r_y = 0.83 -> xy
def _inclined_kind(axis):
    return 2 if axis == 1 else 3


def generic_cases():
    cases = []
    thetas = (100.0, 80.0, 170.0, 10.0)
    # exact zeros: one horizontal component 0.0, the other of either sign; and both zero
    for theta in thetas:
        c, s = np.cos(np.radians(theta)), np.sin(np.radians(theta))
        for axis, sg in itertools.product((1, 2), (1.0, -1.0)):
            k = np.array([c, 0.0, 0.0])
            k[axis] = sg * s
            kind = 1 if theta in (170.0, 10.0) else _inclined_kind(axis)
            cases.append(Case("zero", "z%g_%d%+d" % (theta, axis, int(sg)), k, {kind}))
    cases.append(Case("zero", "pole_up", [-1.0, 0.0, 0.0], {1}))
    cases.append(Case("zero", "pole_down", [1.0, 0.0, 0.0], {1}))
    # rounding residues of direction(): phi = 0 gives an exact zero (sin 0), the others +-1e-16 of both signs.  Each
    # residue case has a partner with the residue set to 0.0 and the same I_0: where the non-zero horizontal component
    # is positive the quadrant tests give its axis sign -1 and the `else` branch +1, so the two must differ
    # (`differs`); where it is negative both give that axis +1, and the axis of the residue does not move the upwind
    # point (|r k| < 1e-15 << x), so the two agree to rounding.
    for theta, phi in itertools.product(thetas + (180.0,), (0.0, 90.0, 180.0, 270.0)):
        k = orc.direction(theta, phi)
        small = np.abs(k[1:]) < TINY
        if theta == 180.0:
            kind, big = 1, None
        else:
            big = 1 if not small[0] else 2
            kind = 1 if theta in (170.0, 10.0) else _inclined_kind(big)
        exact = not np.any((k[1:] != 0.0) & small)
        label = "d%g_%g" % (theta, phi)
        if exact:
            cases.append(Case("zero", label, k, {kind}))
            continue
        k0 = k.copy()
        k0[1:][small] = 0.0
        differs = big is not None and k[big] > 0
        cases.append(Case("zero", label + "_0", k0, {kind}))
        cases.append(Case("residue", label, k, {kind}, pair=label + "_0", differs=differs))
    # near-grazing rays: theta = 90 +- 0.5 and 90 +- 0.01 at two generic phi
    #   phi = 33: (k_x, k_y) = (0.839, 0.545): r_x = 0.108 < r_y = 0.265 -> yz;  phi = 250: (-0.342, -0.940): r_y = 0.154 < r_x = 0.266 -> xz
    for dth, (phi, kind) in itertools.product((0.5, -0.5, 0.01, -0.01), ((33.0, 2), (250.0, 3))):
        cases.append(Case("grazing", "g%+g_%g" % (dth, phi), orc.direction(90.0 + dth, phi), {kind}))
    return cases


# ---- raster T: bit-equal spacings -- exact ties of the r values, one ulp either side -----------------------------------
TIES = {                                    # name: (|k| before normalising (z, x, y), kind that wins the tie)
    "xy": ((0.2, 1.0, 1.0), 2),             # r_x == r_y < r_z: yz, the first of the two minima
    "zx": ((1.0, 1.0, 0.4), 1),             # r_z == r_x < r_y: xy, the first
    "zy": ((1.0, 0.4, 1.0), 1),             # r_z == r_y < r_x
    "zxy": ((1.0, 1.0, 1.0), 1),            # all three equal
}
# (tie, component nudged, kind on the far side of the tie when |component| GROWS by one ulp: its r shrinks and wins)
NUDGES = (("xy", 2, 3), ("zx", 1, 2), ("zy", 2, 3), ("zxy", 1, 2), ("zxy", 2, 3))
NUDGE_OCTANTS = ((-1.0, 1.0, -1.0), (1.0, -1.0, 1.0))


def tie_cases():
    cases = []
    for name, (v, kind) in TIES.items():
        a = unit(v)
        for sg in itertools.product((-1.0, 1.0), repeat=3):
            cases.append(Case("tie_" + name, "%s%+d%+d%+d" % ((name,) + tuple(int(s) for s in sg)), a * np.array(sg), {kind}, tie=name))
    for (name, comp, far), sg in itertools.product(NUDGES, NUDGE_OCTANTS):
        a = unit(TIES[name][0])
        for toward, kind in ((np.inf, far), (0.0, TIES[name][1])):
            b = a.copy()
            b[comp] = np.nextafter(a[comp], toward)
            cases.append(Case("ulp_" + name, "%s_c%d_%s%+d" % (name, comp, "grow" if toward else "shrink", int(sg[0])),
                              b * np.array(sg), {kind}, tie=name))
    return cases


# ---- raster M: the kind changes from plane to plane inside one solve ---------------------------------------------------
# x, y of _random_problem(9, 12, 10): dx = 0.0909, dy = 0.1444.  |k_z| = cos 45 = 0.7071:
#   phi = 40 / 220: |k_x| = 0.5417, |k_y| = 0.4545: r_x = 0.168 < r_y = 0.318; thin step 0.05: r_z = 0.071 -> xy, thick 0.3: r_z = 0.424 -> yz
#   phi = 60 / 240: |k_x| = 0.3536, |k_y| = 0.6124: r_y = 0.236 < r_x = 0.257;            thin -> xy,              thick -> xz
MIXED_STEPS = (0.05, 0.3, 0.05, 0.05, 0.3, 0.3, 0.05, 0.3)


def mixed_cases():
    cases = []
    for (theta, phi), other in (((135.0, 40.0), 2), ((45.0, 220.0), 2), ((135.0, 60.0), 3), ((45.0, 240.0), 3)):
        seq = [1 if st < 0.1 else other for st in MIXED_STEPS]
        kinds = [0] + seq if theta > 90 else seq + [0]          # plane idz is solved over the step below (up) / above (down)
        cases.append(Case("mixed", "m%g_%g" % (theta, phi), orc.direction(theta, phi), kinds))
    return cases


class Raster:
    def __init__(self, name, shape, seed, cases, z=None, cubic=False):
        nz, nx, ny = shape
        self.name, self.cases = name, cases
        self.z, self.x, self.y, self.S, self.al, _ = _random_problem(nz, nx, ny, seed)
        if cubic:
            self.x, self.y, self.z = np.arange(nx) * H, np.arange(ny) * H, np.arange(nz) * H
        if z is not None:
            self.z = np.asarray(z, dtype=np.float64)
        rng = np.random.default_rng(seed + 1000)
        by_label = {c.label: i for i, c in enumerate(cases)}
        assert len(by_label) == len(cases)
        self.I0s = rng.random((len(cases), ny, nx))
        for i, c in enumerate(cases):
            if c.pair is not None:
                self.I0s[i] = self.I0s[by_label[c.pair]]
        self.pairs = [(i, by_label[c.pair]) for i, c in enumerate(cases) if c.pair is not None]
        self.ks = np.stack([c.k for c in cases])
        self.ups = [c.up for c in cases]

    def all_xy(self, i):
        c = self.cases[i]
        return set(c.kinds) - {0} == {1}


@functools.lru_cache(maxsize=None)
def rasters():
    return {"generic": Raster("generic", (9, 12, 10), 31, generic_cases()),
            "ties": Raster("ties", (6, 9, 8), 32, tie_cases(), cubic=True),
            "mixed": Raster("mixed", (9, 12, 10), 33, mixed_cases(), z=np.concatenate([[0.0], np.cumsum(MIXED_STEPS)]))}


@functools.lru_cache(maxsize=None)
def oracle_solutions(name, n_sweeps):
    """(I, kinds) of every case of a raster: computed once, shared by the host and the GPU tests, never written to."""
    ra = rasters()[name]
    out = [solve_oracle(c.k, c.up, ra.S, ra.I0s[i], ra.al, ra.z, ra.x, ra.y, n_sweeps, return_planes=True)
           for i, c in enumerate(ra.cases)]
    for I, kinds in out:
        I.setflags(write=False)
    return out


def rel_diff(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("name", ["generic", "ties", "mixed"])
def test_direction_set_is_accepted_finite_and_of_the_kinds_it_was_built_for(name):
    ra = rasters()[name]
    assert len(ra.cases) < 100
    assert {c.up for c in ra.cases} == {True, False}
    for n_sweeps in (1, 3):
        for c, (I, kinds) in zip(ra.cases, oracle_solutions(name, n_sweeps)):
            assert abs(np.sqrt((c.k * c.k).sum()) - 1.0) < 1e-6 and c.k[0] != 0.0, c      # regular_check_k
            assert np.isfinite(I).all(), c
            if isinstance(c.kinds, list):
                assert kinds.tolist() == c.kinds, (c, kinds)
            else:
                assert set(kinds.tolist()) == {0} | c.kinds, (c, kinds)


def test_generic_set_has_every_zero_and_residue_pattern():
    cases = rasters()["generic"].cases
    zero = [c for c in cases if c.cls == "zero"]
    for pattern in ((True, False), (False, True), (True, True)):
        for up in (True, False):
            assert any(c.up == up and (c.k[1] == 0.0, c.k[2] == 0.0) == pattern for c in zero), (pattern, up)
    for up in (True, False):                                  # k_x = 0 with either sign of k_y, and the other way round
        assert {np.sign(c.k[2]) for c in zero if c.up == up and c.k[1] == 0.0 and c.k[2] != 0.0} == {1.0, -1.0}
        assert {np.sign(c.k[1]) for c in zero if c.up == up and c.k[2] == 0.0 and c.k[1] != 0.0} == {1.0, -1.0}
    res = [c for c in cases if c.cls == "residue"]
    small = np.array([[v for v in c.k[1:] if 0.0 < abs(v) < TINY][0] for c in res])
    assert (np.abs(small) < 1e-15).all() and (small > 0).any() and (small < 0).any()
    assert any(c.differs for c in res) and any(not c.differs for c in res)
    assert {c.label for c in cases if c.cls == "grazing"} >= {"g+0.5_33", "g-0.01_250"}
    k = next(c.k for c in cases if c.label == "g+0.01_33")
    assert 1.7e-4 < abs(k[0]) < 1.8e-4


def test_exact_zero_takes_the_else_branch_and_the_residue_does_not():
    """k_x = 0.0 falls into xy_intersect's `else` (sign_x = sign_y = +1); k_x = 6e-17 takes a quadrant.  Where the two
    choices differ on the axis that carries the ray, the solutions differ in the third digit; elsewhere they agree."""
    ra = rasters()["generic"]
    for n_sweeps in (1, 3):
        sol = oracle_solutions("generic", n_sweeps)
        for i, j in ra.pairs:
            d = rel_diff(sol[i][0], sol[j][0])
            if ra.cases[i].differs:
                assert d > 1e-6, (ra.cases[i], d)
            else:
                assert d < 1e-12, (ra.cases[i], d)


def test_ties_are_exact_and_the_ulp_cases_sit_on_the_boundary():
    ra = rasters()["ties"]
    assert ra.x[1] - ra.x[0] == ra.y[1] - ra.y[0] == H and (np.diff(ra.z) == H).all()
    sol = oracle_solutions("ties", 3)
    for name, (v, kind) in TIES.items():
        tied = [c for c in ra.cases if c.cls == "tie_" + name]
        assert len(tied) == 8 and len({tuple(np.sign(c.k)) for c in tied}) == 8
        for c in tied:
            r = np.abs(H / c.k)                               # (r_z, r_x, r_y) as every copy of the decision forms them
            eq = [j for j in range(3) if v[j] == max(v)]
            assert len({r[j] for j in eq}) == 1 and r.min() == r[eq[0]], (c, r)
    by_label = {c.label: i for i, c in enumerate(ra.cases)}
    for (name, comp, far), sg in itertools.product(NUDGES, NUDGE_OCTANTS):
        tie_kinds = {0, TIES[name][1]}
        grow = sol[by_label["%s_c%d_grow%+d" % (name, comp, int(sg[0]))]][1]
        shrink = sol[by_label["%s_c%d_shrink%+d" % (name, comp, int(sg[0]))]][1]
        assert set(grow.tolist()) == {0, far} != tie_kinds          # one ulp on: the other kernel
        assert set(shrink.tolist()) == tie_kinds                    # one ulp back: still the tie's


# ---- the shape table of the launch forms -------------------------------------------------------------------------------
# regular_launch (csrc/vrt_regular.hip), with m = max(nx, ny) - 2 and interior = (nx - 2)(ny - 2):
#   threads = min(1024, max(128, ceil64(m))); an all-xy batch doubles it while 2 threads <= 1024, <= interior (and the
#             batch stays under 256 Ki threads);  solve<256> if threads <= 256, else solve<1024>;
#             a yz plane takes row_march iff ny - 2 <= threads, an xz plane iff nx - 2 <= threads, else the strided loop
#   all-xy batch, VRT_REG_XY = 1 (default) or 2:  mt = min(1024, ceil64(interior)), npt = ceil(interior / mt),
#             lds = 8 (2 nx ny + 7 (nx + ny) + nz [+ 1 to even]) bytes;  mode 2 or lds > 150 KiB: xy_march_mem;  else
#             fits = nx ny <= (2, 3, 5 for npt <= 1, 2, 4) mt;  lds<1|2|4> for npt <= 1|2|4 and fits, else lds<0>
# Rows: (nz, nx, ny), direction class, VRT_REG_XY, (form, threads, rows of the solve forms)
BOTH = {"yz": "row_march", "xz": "row_march"}
SHAPES = [
    # interior 38 x 38 = 1444: mt = 1024, npt = 2, plane 1600 <= 3 x 1024 -> lds<2>; lds = 8 (3200 + 560 + 4) = 30 KB
    ((4, 40, 40), "steep", "1", ("xy_march_lds<2>", 1024, None)),
    ((4, 40, 40), "steep", "2", ("xy_march_mem", 1024, None)),
    # m = 38: threads 128, all-xy doubles to 1024 (<= 1444) -> solve<1024>
    ((4, 40, 40), "steep", "0", ("solve<1024>", 1024, BOTH)),
    # interior 1 x 198: mt = 256, npt = 1, but plane 600 > 2 x 256 -> !fits -> lds<0>
    ((3, 3, 200), "steep", "1", ("xy_march_lds<0>", 256, None)),
    ((3, 200, 3), "steep", "1", ("xy_march_lds<0>", 256, None)),
    # m = 198: threads 256; doubling needs 512 <= 198: no -> solve<256>
    ((3, 3, 200), "steep", "0", ("solve<256>", 256, BOTH)),
    # interior 3 x 1028 = 3084: mt = 1024, npt = 4, plane 5150 > 5 x 1024 = 5120 -> !fits -> lds<0>;
    # lds = 8 (10300 + 7245 + 4 + 1) = 140 400 B = 137 KiB <= 150 KiB: still in LDS
    ((4, 5, 1030), "steep", "1", ("xy_march_lds<0>", 1024, None)),
    ((4, 1030, 5), "steep", "2", ("xy_march_mem", 1024, None)),
    # interior 46 x 45 = 2070: mt = 1024, npt = 3, plane 2256 <= 5120 -> lds<4>
    ((3, 48, 47), "steep", "1", ("xy_march_lds<4>", 1024, None)),
    # plane 100 x 99: lds = 8 (19800 + 1393 + 2 + 1) = 169 568 B > 150 KiB -> xy_march_mem without being asked
    ((2, 100, 99), "steep", "1", ("xy_march_mem", 1024, None)),
    # rows of 298 points: m = 298 -> threads 320 -> solve<1024>; 298 <= 320 and 3 <= 320: both kinds row_march,
    # n_ser = 3 with 298 lanes and n_ser = 298 with 3 lanes
    ((3, 300, 5), "yz", "1", ("solve<1024>", 320, BOTH)),
    ((3, 300, 5), "xz", "1", ("solve<1024>", 320, BOTH)),
    ((3, 5, 300), "yz", "1", ("solve<1024>", 320, BOTH)),
    ((3, 5, 300), "xz", "1", ("solve<1024>", 320, BOTH)),
    # rows of 1028 points: threads 1024; the kind whose rows are 1028 long (1028 > 1024) takes the strided loop
    # unforced, the other row_march with n_ser = 1028 and 2 lanes
    ((3, 1030, 4), "yz", "1", ("solve<1024>", 1024, {"yz": "row_march", "xz": "strided"})),
    ((3, 1030, 4), "xz", "1", ("solve<1024>", 1024, {"yz": "row_march", "xz": "strided"})),
    ((3, 4, 1030), "yz", "1", ("solve<1024>", 1024, {"yz": "strided", "xz": "row_march"})),
    ((3, 4, 1030), "xz", "1", ("solve<1024>", 1024, {"yz": "strided", "xz": "row_march"})),
    # one plane, one interior point: interior 1 -> mt = 64, npt = 1, plane 9 <= 128 -> lds<1>; threads 128 (no doubling:
    # 256 > 1) -> solve<256>; n_ser = 1 and one active lane in both row kinds
    ((2, 3, 3), "steep", "1", ("xy_march_lds<1>", 64, None)),
    ((2, 3, 3), "steep", "0", ("solve<256>", 128, BOTH)),
    ((2, 3, 3), "yz", "1", ("solve<256>", 128, BOTH)),
    ((2, 3, 3), "xz", "1", ("solve<256>", 128, BOTH)),
    # one plane, one active lane or n_ser = 1: interior 7 -> mt = 64 -> lds<1>; threads 128
    ((2, 3, 9), "steep", "1", ("xy_march_lds<1>", 64, None)),
    ((2, 3, 9), "yz", "1", ("solve<256>", 128, BOTH)),          # n_ser = 1, 7 lanes
    ((2, 3, 9), "xz", "1", ("solve<256>", 128, BOTH)),          # n_ser = 7, 1 lane
    ((2, 9, 3), "steep", "1", ("xy_march_lds<1>", 64, None)),
    ((2, 9, 3), "yz", "1", ("solve<256>", 128, BOTH)),          # n_ser = 7, 1 lane
    ((2, 9, 3), "xz", "1", ("solve<256>", 128, BOTH)),          # n_ser = 1, 7 lanes
]
ALL_FORMS = {"solve<256>", "solve<1024>", "xy_march_lds<1>", "xy_march_lds<2>", "xy_march_lds<4>", "xy_march_lds<0>",
             "xy_march_mem"}
# (theta, phi) per class on the axes of shape_problem: dx = 0.1, dy = 0.13, dz in [0.1, 0.3]
#   steep: |k_z| >= 0.985, horizontal <= 0.174: r_z <= 0.31 < r_x >= 0.57
#   yz (theta = 100 / 80, phi = 10 / 190): |k| = (0.174, 0.970, 0.171): r_x = 0.103 < r_z >= 0.57, r_y = 0.76
#   xz (phi = 80 / 260): |k| = (0.174, 0.171, 0.970): r_y = 0.134 < r_z, r_x = 0.585
SHAPE_ANGLES = {"steep": ((175.0, 30.0), (6.0, 200.0), (172.0, 300.0), (180.0, 0.0), (9.0, 100.0)),
                "yz": ((100.0, 10.0), (80.0, 190.0), (100.0, 170.0), (80.0, 350.0)),
                "xz": ((100.0, 80.0), (80.0, 260.0), (100.0, 280.0), (80.0, 100.0))}
SHAPE_KIND = {"steep": 1, "yz": 2, "xz": 3}


@functools.lru_cache(maxsize=None)
def shape_problem(shape, cls):
    """axes, fields, directions, I_0 and the oracle's solutions of one (shape, direction class) of the table"""
    nz, nx, ny = shape
    seed = 40 + nz + 3 * nx + 7 * ny
    _, _, _, S, al, _ = _random_problem(nz, nx, ny, seed)
    rng = np.random.default_rng(seed + 1)
    z = np.cumsum(rng.uniform(0.1, 0.3, nz))
    x, y = np.arange(nx) * 0.1, np.arange(ny) * 0.13
    ks = np.stack([orc.direction(t, p) for t, p in SHAPE_ANGLES[cls]])
    ups = [t > 90 for t, _ in SHAPE_ANGLES[cls]]
    I0s = rng.random((len(ups), ny, nx))
    refs = []
    for j in range(len(ups)):
        I, kinds = solve_oracle(ks[j], ups[j], S, I0s[j], al, z, x, y, 3, return_planes=True)
        I.setflags(write=False)
        refs.append((I, kinds))
    return z, x, y, S, al, ks, ups, I0s, refs


def expected_launch(shape, cls, mode):
    """regular_launch's arithmetic, restated (the table above is checked against it here, and against the solver's own
    report on the GPU)"""
    nz, nx, ny = shape
    c64 = lambda v: (v + 63) // 64 * 64
    interior = (nx - 2) * (ny - 2)
    n_solve = len(SHAPE_ANGLES[cls])
    threads = min(1024, max(128, c64(max(nx, ny) - 2)))
    if cls == "steep":
        while threads * 2 <= 1024 and n_solve * threads * 2 <= 256 * 1024 and threads * 2 <= interior:
            threads *= 2
    if cls == "steep" and mode != "0":
        mt = min(1024, c64(interior))
        npt = -(-interior // mt)
        lead = 2 * nx * ny + nx + ny
        lds = 8 * (lead + (lead & 1) + 6 * (nx + ny) + nz)
        if mode == "2" or lds > 150 * 1024:
            return "xy_march_mem", mt, None
        fits = nx * ny <= (2 if npt <= 1 else 3 if npt <= 2 else 5) * mt
        for n in (1, 2, 4):
            if npt <= n and fits:
                return "xy_march_lds<%d>" % n, mt, None
        return "xy_march_lds<0>", mt, None
    rows = {"yz": "row_march" if ny - 2 <= threads else "strided", "xz": "row_march" if nx - 2 <= threads else "strided"}
    return ("solve<256>" if threads <= 256 else "solve<1024>"), threads, rows


def test_shape_table_follows_the_launch_inequalities_and_covers_every_form():
    forms, rows_seen = set(), set()
    for shape, cls, mode, expect in SHAPES:
        assert expected_launch(shape, cls, mode) == expect, (shape, cls, mode)
        forms.add(expect[0])
        if expect[2] and cls in ("yz", "xz"):
            rows_seen.add((expect[0], expect[2][cls]))
        assert shape[0] * shape[1] * shape[2] <= 20600
    assert forms == ALL_FORMS
    assert rows_seen == {("solve<256>", "row_march"), ("solve<1024>", "row_march"), ("solve<1024>", "strided")}


@pytest.mark.parametrize("shape,cls", sorted({(s, c) for s, c, _, _ in SHAPES}))
def test_shape_table_oracle_runs_are_finite_and_of_their_kind(shape, cls):
    refs = shape_problem(shape, cls)[8]
    for I, kinds in refs:
        assert np.isfinite(I).all()
        assert set(kinds.tolist()) == {0, SHAPE_KIND[cls]}


# ---- a known answer with a gradient ------------------------------------------------------------------------------------
# Horizontally uniform fields, S(z) = s0 + g z on a non-uniform z, alpha constant.  Along a ray travelling in -k,
# dS/ds = -k_z g, so I = S + k_z g / alpha solves dI/ds = alpha (S - I) exactly, and linear short characteristics with
# exact weights reproduce a linear S exactly: with I_0 = that value on the entry plane every plane holds it.  It sees
# what "uniform stays uniform" cannot: the split between the weights a and b, the upwind point of S_u, r and z_up.  The
# yz / xz kernels reach it once the row recurrence (started from zeros) has converged: alpha r >> 1 per row.
# xz_down_ray reads its centre values from the plane above (reference quirk, :794, :804) and misses by a few per cent:
# that figure is pinned, not repaired.
KAT_S0, KAT_G = 2.0, 0.7
KAT_ANGLES = ((170.0, 30.0), (100.0, 10.0), (100.0, 80.0), (10.0, 200.0), (80.0, 190.0), (80.0, 100.0))
KAT_SETTINGS = ((1e-3, 3), (0.3, 1), (80.0, 3), (3e3, 1))           # (alpha, n_sweeps)


def kat_directions():
    out = [("generic %g,%g" % a, orc.direction(*a)) for a in KAT_ANGLES]
    out += [(repr(c), c.k) for c in rasters()["generic"].cases if c.cls == "zero" and c.label.startswith(("z", "pole"))]
    return out


def kat_problem(k, alpha):
    z, x, y, S, al, I0 = _random_problem(9, 12, 10, 4)
    S = np.broadcast_to(KAT_S0 + KAT_G * z, S.shape).copy()
    exact = S + k[0] * KAT_G / alpha
    up = k[0] < 0
    I0 = exact[:, :, 0 if up else -1].copy()
    return z, x, y, S, np.full_like(S, alpha), I0, up, exact


def kat_class(kinds, up, alpha):
    """which bound a run is held to (None: not asserted -- the row recurrence has not converged at this alpha)"""
    kind = (set(kinds.tolist()) - {0}).pop()
    if kind == 1:
        return "xy_series" if alpha < 0.01 else "xy"
    if alpha < 80:
        return None
    return "xz_down" if kind == 3 and not up else "rows"


# measured on the oracle (max |I - exact| / max |exact| per class, all directions and settings); bound = 2 x measured
#   xy_series (alpha = 1e-3: the series branch of linear_weights, I ~ 1e3 g against S ~ 2: heavy cancellation)
KAT_MEASURED = {"xy_series": 2.780e-12, "xy": 1.228e-15, "rows": 1.607e-16}
KAT_XZ_DOWN_MEASURED = (3.796e-2, 4.142e-2)                          # smallest and largest miss of xz_down_ray


def oracle_batch(ks, ups, S, I0s, al, z, x, y, n_sweeps):
    return [solve_oracle(ks[j], ups[j], S, I0s[j], al, z, x, y, n_sweeps) for j in range(len(ups))]


def kat_run(batch):
    """{class: [(label, alpha, n_sweeps, error, I)]} of `batch(ks, ups, S, I0s, al, z, x, y, n_sweeps)`: one batch per
    (alpha, n_sweeps), the solves that are not asserted left out"""
    out = {}
    for alpha, n_sweeps in KAT_SETTINGS:
        todo = []
        for label, k in kat_directions():
            z, x, y, S, al, I0, up, exact = kat_problem(k, alpha)
            _, kinds = solve_oracle(k, up, S, I0, al, z, x, y, 1, return_planes=True)
            assert len(set(kinds.tolist())) == 2
            cls = kat_class(kinds, up, alpha)
            if cls is not None:
                todo.append((cls, label, k, up, I0, exact))
        Is = batch(np.stack([t[2] for t in todo]), [t[3] for t in todo], S, np.stack([t[4] for t in todo]), al, z, x, y, n_sweeps)
        for (cls, label, k, up, I0, exact), I in zip(todo, Is):
            out.setdefault(cls, []).append((label, alpha, n_sweeps, np.abs(I - exact).max() / np.abs(exact).max(), I))
    return out


@functools.lru_cache(maxsize=None)
def kat_oracle():
    return kat_run(oracle_batch)


def test_oracle_reproduces_a_linear_source_function():
    res = kat_oracle()
    assert set(res) == {"xy_series", "xy", "rows", "xz_down"}
    for cls, rows in sorted(res.items()):
        errs = [r[3] for r in rows]
        print("known answer, oracle, %-9s: %2d runs, error %.3e .. %.3e" % (cls, len(rows), min(errs), max(errs)))
    for cls, measured in KAT_MEASURED.items():
        for label, alpha, n_sweeps, err, _ in res[cls]:
            assert err <= 2 * measured, (cls, label, alpha, n_sweeps, err)
    lo, hi = KAT_XZ_DOWN_MEASURED
    for label, alpha, n_sweeps, err, _ in res["xz_down"]:
        assert lo / 2 <= err <= 2 * hi, (label, alpha, n_sweeps, err)


# ---- vrt_regular_last_launch_form: ABI and the checks that run before the device -----------------------------------------
def test_last_launch_form_symbol_and_argument_checks():
    import ctypes
    import os
    import re
    import voronoirt_amd as vrt
    from voronoirt_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "voronoirt.h")).read()
    assert re.search(r"\bvrt_regular_last_launch_form\s*\(", header)
    assert "vrt_regular_last_launch_form" in _lib.PROTOTYPES
    for i, name in enumerate(("SOLVE256", "SOLVE1024", "XY_MARCH_LDS1", "XY_MARCH_LDS2", "XY_MARCH_LDS4", "XY_MARCH_LDS0",
                              "XY_MARCH_MEM")):
        assert re.search(r"\bVRT_REG_FORM_%s = %d\b" % (name, i), header), name
    assert set(_lib.REG_FORMS) == ALL_FORMS and len(_lib.REG_FORMS) == 7
    assert callable(vrt.RegularSolver.last_launch_form)
    L = _lib.load()
    form, threads = ctypes.c_int(-7), ctypes.c_int(-7)
    dummy = ctypes.c_void_p(16)                                      # a handle the checks never dereference
    E = _lib.VRT_EINVAL
    assert L.vrt_regular_last_launch_form(None, ctypes.byref(form), ctypes.byref(threads)) == E
    assert L.vrt_regular_last_launch_form(dummy, None, ctypes.byref(threads)) == E
    assert L.vrt_regular_last_launch_form(dummy, ctypes.byref(form), None) == E
    assert form.value == -7 and threads.value == -7
    if L.vrt_device_count() == 0:                                    # no device: no handle to ask, and that is an error
        z = np.linspace(0.0, 1.0, 4)
        with pytest.raises(vrt.VrtError) as e:
            vrt.RegularSolver(z, z, z, device=0)
        assert e.value.code == _lib.VRT_ENODEVICE
