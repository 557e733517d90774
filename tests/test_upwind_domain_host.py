"""The inputs of tests/test_upwind_domain.py (GPU), shown on the CPU oracle to be what they claim to be.

The upwind search (smallest_angle, voronoi_utils.jl:360-396) is order dependent: a neighbour whose dot product is
greater than slot 2 takes slot 1 if it is also greater than slot 1 (the old holder is discarded) and slot 2 otherwise,
both with strict '>', and `dots[2] <= 0` collapses slot 2 onto slot 1.  The device (k_upwind_table, csrc/vrt_kernels.hip)
evaluates that rule in closed form per chunk of 16 row slots.  The two can only differ where a comparison sees equal
operands, and on grids in general position none ever does.  The grids below are lattices with binary-exact coordinates
(spacings 1/8, 1/4 or 1.5e6), so that collinear neighbours have bit-equal Delaunay lines and axis, face-diagonal and
body-diagonal directions give bit-equal dot products, exact zeros and exact -1; the directions are handed over as k
arrays (direction(theta, phi) leaves 1e-16 residues), each tie direction also with one component moved by one ulp.

Plan creation accepts k_z = 0 when the sweep direction is given (`dirs`), so the horizontal directions are exact.
One plan holds at most 64 active angles; the direction set has exactly 64.

The Delaunay lines (calc_Delaunay_lines, :186-245) take their periodic image with a strict '<': across 4 (or 2) sites
the offset of half a box is an exact equality ("no shift"), and the left-edge branch mirrors instead of shifting, which
on cell-centred exact coordinates puts the neighbour on the site itself (a NaN line, skipped by every comparison)."""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import pyref
from voronoirt_amd import synth

H = 0.125                                   # lattice spacing of the shells grids: every coordinate binary-exact
CHUNK = 16                                  # row slots k_upwind_table visits at a time


# ---- grids -------------------------------------------------------------------------------------------------------------
def _site_id(i, j, k, nx, ny, nz):
    return (np.mod(i, nx) * ny + np.mod(j, ny)) * nz + k + 1


def shell_links(nx, ny, nz, r2):
    """{site: set of neighbour ids} (1-based) of the periodic cubic lattice whose rows list every lattice offset with
    |d|^2 <= r2, wrapped in x and y, cut in z; an offset and its opposite that wrap onto one site are listed once"""
    R = int(np.sqrt(r2))
    offs = [d for d in itertools.product(range(-R, R + 1), repeat=3) if 0 < d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= r2]
    links = {}
    for i, j, k in itertools.product(range(nx), range(ny), range(nz)):
        s = int(_site_id(i, j, k, nx, ny, nz))
        row = set()
        for dz, dx, dy in offs:
            if 0 <= k + dz < nz:
                q = int(_site_id(i + dx, j + dy, k + dz, nx, ny, nz))
                if q != s:
                    row.add(q)
        links[s] = row
    return links


def _drop(a, b):
    """link (a, b) of shells-ragged is removed: a function of the unordered pair.  Every eighth site is sparse (keeps a
    quarter of its links); the others lose only those."""
    a, b = min(a, b), max(a, b)
    sparse = ((a - 1) % 8 == 0) + ((b - 1) % 8 == 0)
    return sparse > 0 and (a * 7 + b * 13) % 4 != 0


def _trim(links, site, target, walls, protect):
    """remove single symmetric links of `site` (largest partner first) until its row has `target` entries"""
    while len(links[site]) + walls(site) > target:
        q = max(v for v in links[site] if v not in protect)
        links[site].discard(q)
        links[q].discard(site)


def shells_grid(nx, ny, nz, r2, seed, h=H, ragged=False):
    """positions (z, x, y) = ((k, i, j) + 0.5) h, neighbours (D+1, n) with rows shuffled by synth._pack_rows, bounds"""
    links = shell_links(nx, ny, nz, r2)
    n = nx * ny * nz
    walls = lambda s: int((s - 1) % nz in (0, nz - 1))
    if ragged:
        for a in range(1, n + 1):
            for b in [b for b in links[a] if b > a and _drop(a, b)]:
                links[a].discard(b)
                links[b].discard(a)
        # one row of exactly 3 x 16 entries and one of 3 x 16 + 1: two interior sites that are not neighbours
        full = sorted(s for s in links if len(links[s]) + walls(s) >= 3 * CHUNK + 2)
        a = full[0]
        b = next(s for s in full if s not in links[a] and s != a)
        _trim(links, a, 3 * CHUNK, walls, {b})
        _trim(links, b, 3 * CHUNK + 1, walls, {a})
    K = max(len(v) for v in links.values()) + 1
    cols = np.zeros((n, K), dtype=np.int64)
    for s, row in links.items():
        row = sorted(row)
        cols[s - 1, :len(row)] = row
        k = (s - 1) % nz
        if k == 0:
            cols[s - 1, len(row)] = synth.BOTTOM_WALL
        elif k == nz - 1:
            cols[s - 1, len(row)] = synth.TOP_WALL
    nbr = synth._pack_rows(cols, np.random.default_rng(seed))
    ii, jj, kk = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    pos = np.stack([(kk.ravel() + 0.5) * h, (ii.ravel() + 0.5) * h, (jj.ravel() + 0.5) * h], axis=1)
    return np.ascontiguousarray(pos), nbr, (0.0, nz * h, 0.0, nx * h, 0.0, ny * h)


def reshuffled(nbr, seed):
    """every row of a neighbour matrix in a new order"""
    rng = np.random.default_rng(seed)
    nb = nbr.copy()
    for i in range(nb.shape[1]):
        c = nb[0, i]
        nb[1:c + 1, i] = rng.permutation(nb[1:c + 1, i])
    return nb


COINCIDENT_SITE = 75                        # 0-based: (i, j, k) = (2, 2, 3) of shells, moved onto its +x neighbour (3, 2, 3)


@functools.lru_cache(maxsize=None)
def grids():
    """name -> (positions, neighbours, bounds); never written to"""
    out = {"cubic": synth.regular_lattice_grid(5, 4, 6),
           "bcc0": synth.bcc_grid(4, 3, 7, jitter=0.0),
           "shells": shells_grid(5, 5, 6, 5, 1),
           "shells-ragged": shells_grid(5, 5, 6, 5, 2, ragged=True),
           "periodic-tie": shells_grid(4, 4, 5, 5, 3, h=0.25),        # coordinates (i + 0.5) / 4
           "periodic-tie2": shells_grid(2, 2, 5, 2, 4, h=0.25)}       # 2 across: the offset +-1 is half a box
    pos, nbr, bounds = out["shells"]
    pos = pos.copy()
    pos[COINCIDENT_SITE] = pos[COINCIDENT_SITE + 5 * 6]
    out["coincident"] = (pos, nbr, bounds)
    for p, nb, _ in out.values():
        p.setflags(write=False)
        nb.setflags(write=False)
    return out


GRIDS = ("cubic", "bcc0", "shells", "shells-ragged", "periodic-tie", "periodic-tie2", "coincident")
SOLVE_GRIDS = ("cubic", "bcc0", "shells-ragged")
ORDER_GRIDS = ("shells", "bcc0")
ORDER_SEEDS = (11, 12, 13)


@functools.lru_cache(maxsize=None)
def oracle_sites(name, order_seed=None):
    pos, nbr, bounds = grids()[name]
    if order_seed is not None:
        nbr = reshuffled(nbr, order_seed)
    return orc.make_sites(pos, nbr, bounds)


# ---- directions ----------------------------------------------------------------------------------------------------------
class Direction:
    """label, class, k, sweep direction (+1 up, -1 down), `tie`: label of the tie direction it sits one ulp from"""

    def __init__(self, cls, label, k, d=None, tie=None):
        self.cls, self.label, self.k = cls, label, np.asarray(k, dtype=np.float64)
        self.d = d if d is not None else (1 if self.k[0] < 0 else -1)
        self.tie = tie

    def __repr__(self):
        return "%s[%s] k=(%r, %r, %r) %s" % ((self.cls, self.label) + tuple(float(v) for v in self.k) + ("up" if self.d > 0 else "down",))


def _nudged(cls, base, comp, dirs_out):
    """`base` with component comp moved one ulp towards and away from zero (from 0.0: to the smallest denormals)"""
    for name, toward in (("-", 0.0 if base.k[comp] != 0.0 else -np.inf), ("+", np.inf if base.k[comp] >= 0.0 else -np.inf)):
        k = base.k.copy()
        k[comp] = np.nextafter(k[comp], toward)
        assert k[comp] != base.k[comp]
        dirs_out.append(Direction(cls, "%s_c%d%s" % (base.label, comp, name), k, d=base.d, tie=base.label))


@functools.lru_cache(maxsize=None)
def directions():
    s2, s3 = np.sqrt(0.5), 1.0 / np.sqrt(3.0)
    sg = lambda v: "+" if v > 0 else "-"
    out = [Direction("axis", "-z", [-1.0, 0.0, 0.0]), Direction("axis", "+z", [1.0, 0.0, 0.0]),
           # horizontal k: the sweep direction is given; each axis once with the up and once with the down sweep
           Direction("axis", "+x", [0.0, 1.0, 0.0], d=1), Direction("axis", "-x", [0.0, -1.0, 0.0], d=-1),
           Direction("axis", "+y", [0.0, 0.0, 1.0], d=-1), Direction("axis", "-y", [0.0, 0.0, -1.0], d=1)]
    face = []
    for a, b in itertools.product((-1.0, 1.0), repeat=2):
        face.append(Direction("face", "zx" + sg(a) + sg(b), [a * s2, b * s2, 0.0]))
        face.append(Direction("face", "zy" + sg(a) + sg(b), [a * s2, 0.0, b * s2]))
    flat = [Direction("face", "xy" + sg(a) + sg(b), [0.0, a * s2, b * s2], d=1 if a * b > 0 else -1)
            for a, b in itertools.product((-1.0, 1.0), repeat=2)]
    body = [Direction("body", "b" + sg(a) + sg(b) + sg(c), [a * s3, b * s3, c * s3])
            for a, b, c in itertools.product((-1.0, 1.0), repeat=3)]
    out += face + flat + body
    # one ulp either side.  An exact 0.0 moves to +-4.9e-324: the products with a line are denormal or round to zero.
    for base in out[:2]:
        _nudged("ulp_axis", base, 1, out)
    _nudged("ulp_axis", out[2], 2, out)
    for base in face:
        _nudged("ulp_face", base, 1 if base.k[1] != 0.0 else 2, out)
    for base in flat[:2]:
        _nudged("ulp_face", base, 1, out)
    for base in body[::2]:
        _nudged("ulp_body", base, 1, out)
    # generic control
    out.append(Direction("generic", "d180_0", orc.direction(180.0, 0.0)))
    out.append(Direction("generic", "d90.0001_33", orc.direction(90.0001, 33.0)))
    import voronoirt_amd as vrt
    _, th, ph, _ = vrt.read_quadrature("ul7n12.dat")
    for a in (1, 6):
        out.append(Direction("generic", "ul7n12_%d" % a, orc.direction(th[a], ph[a])))
    assert len({d.label for d in out}) == len(out)
    return tuple(out)


def direction_arrays():
    ds = directions()
    return np.stack([d.k for d in ds]), [d.d for d in ds]


@functools.lru_cache(maxsize=None)
def oracle_tables(name, order_seed=None):
    """orc.upwind_table of every direction on a grid: (up, dots, w, r, status) per direction; never written to"""
    so = oracle_sites(name, order_seed)
    out = []
    for d in directions():
        t = orc.upwind_table(so, d.k)
        for a in t:
            a.setflags(write=False)
        out.append(t)
    return out


# ---- what a (grid, direction) contains, from the oracle's lines ------------------------------------------------------------
CLASSES = ("max_tie_in_chunk", "max_tie_across_chunks", "slot2_tie", "zero_dot", "minus_one_dot", "collapse_eq_0",
           "collapse_lt_0", "wall_inside_chunk", "nan_line")


def visited(so, d):
    """sites the sweep of direction d solves: all but the boundary layer and the last site of the order"""
    perm, lay = (so.perm_up, so.layers_up) if d > 0 else (so.perm_down, so.layers_down)
    m = np.zeros(so.n, dtype=bool)
    m[perm[lay[1] - 1:-1] - 1] = True
    return m


def classify(so, k):
    """{class: boolean mask over the sites} for one direction, by replaying the sequential rule on the oracle's lines"""
    n = so.n
    out = {c: np.zeros(n, dtype=bool) for c in CLASSES}
    nbr, lines = so.neighbours, so.delaunay_lines
    for i in range(n):
        cnt = int(nbr[0, i])
        ids = nbr[1:cnt + 1, i]
        L = lines[i, :cnt]
        with np.errstate(invalid="ignore"):
            dots = (k[0] * L[:, 0] + k[1] * L[:, 1]) + k[2] * L[:, 2]
        real = ids > 0
        nan = real & np.isnan(dots)
        valid = real & ~nan
        D1 = D2 = -1.0
        second = []                                          # slots that competed for slot 2 with their value
        for j in np.nonzero(valid)[0]:
            dj = dots[j]
            if dj > D2:
                if dj > D1:
                    D1 = dj
                else:
                    D2 = dj
            if dj <= D1 and dj > -1.0:
                second.append(dj)
        arg = np.nonzero(valid & (dots == D1))[0]
        if D1 > -1.0 and arg.size > 1:
            chunks = arg // CHUNK
            out["max_tie_in_chunk"][i] = np.unique(chunks).size < chunks.size
            out["max_tie_across_chunks"][i] = chunks[0] != chunks[-1]
        out["slot2_tie"][i] = D2 > -1.0 and sum(1 for v in second if v == D2) - (1 if D2 == D1 else 0) > 1
        out["zero_dot"][i] = bool((valid & (dots == 0.0)).any())
        out["minus_one_dot"][i] = bool((valid & (dots == -1.0)).any())
        out["collapse_eq_0"][i] = D2 == 0.0
        out["collapse_lt_0"][i] = D2 < 0.0
        wall = np.nonzero(ids < 0)[0]
        out["wall_inside_chunk"][i] = any(j % CHUNK not in (0, CHUNK - 1) and j + 1 < cnt and real[j - 1] and real[j + 1]
                                          for j in wall)
        out["nan_line"][i] = bool(nan.any())
    return out


@functools.lru_cache(maxsize=None)
def class_masks(name, order_seed=None):
    """[{class: mask over the sites}] per direction of a grid"""
    so = oracle_sites(name, order_seed)
    return [classify(so, d.k) for d in directions()]


@functools.lru_cache(maxsize=None)
def class_counts(name):
    """{class: [number of sites per direction]} of a grid"""
    per = class_masks(name)
    return {c: [int(p[c].sum()) for p in per] for c in CLASSES}


def lines_equal(a, b):
    """bit for bit, NaN positions as "both NaN\""""
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def valid_line_mask(so):
    m = np.zeros(so.delaunay_lines.shape[:2], dtype=bool)
    for j in range(so.D):
        m[:, j] = (j < so.neighbours[0]) & (so.neighbours[j + 1] > 0)
    return m


# ---- fields of the solves ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solve_problem(name, nlam):
    """S, alpha over the three linear_weights branches (dtau from 1e-6 to 1e3), I_0 of both sweeps; never written to"""
    so = oracle_sites(name)
    rng = np.random.default_rng(50 + nlam + len(name))
    S = 1.0 + rng.random((so.n, nlam))
    step = np.diff(np.unique(so.positions[:, 0])).min()
    alpha = 10.0 ** rng.uniform(-6, 3, (so.n, 1)) * (1.0 + rng.random((so.n, nlam))) / step
    I0u = rng.random((so.layers_up[1] - 1, nlam))
    I0d = rng.random((so.layers_down[1] - 1, nlam))
    for a in (S, alpha, I0u, I0d):
        a.setflags(write=False)
    return S, alpha, I0u, I0d


@functools.lru_cache(maxsize=None)
def solve_directions(name):
    """indices of the directions whose solve is defined on a grid: every visited site has finite weights.  (A horizontal
    axis direction on a site whose only neighbour along it has a NaN line leaves dots = (0, 0), and a best dot of 4.9e-324
    has a seventh power of 0: status 0, weights 0 / 0.  The tables of such directions are compared; their intensities are
    NaN in the reference itself and are not.)"""
    so = oracle_sites(name)
    return tuple(a for a, (d, t) in enumerate(zip(directions(), oracle_tables(name)))
                 if (t[4][visited(so, d.d)] == 0).all() and np.isfinite(t[2][visited(so, d.d)]).all())


@functools.lru_cache(maxsize=None)
def oracle_solves(name, nlam, n_sweeps):
    """per-angle I (n_solve_directions, n, nlam) of solve_directions(name), by Delaunay_upII / Delaunay_downII"""
    so = oracle_sites(name)
    S, alpha, I0u, I0d = solve_problem(name, nlam)
    ds = [directions()[a] for a in solve_directions(name)]
    out = np.zeros((len(ds), so.n, nlam))
    for a, d in enumerate(ds):
        for l in range(nlam):
            f, I0 = (orc.Delaunay_upII, I0u) if d.d > 0 else (orc.Delaunay_downII, I0d)
            out[a, :, l] = f(d.k, S[:, l].copy(), I0[:, l].copy(), alpha[:, l].copy(), so, n_sweeps)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_J(name, nlam, n_sweeps):
    import voronoirt_amd as vrt
    so = oracle_sites(name)
    S, alpha, I0u, I0d = solve_problem(name, nlam)
    w, th, ph, _ = vrt.read_quadrature("ul7n12.dat")
    J = orc.J_voronoi(w, th, ph, S, alpha, so, I0_up=I0u, I0_down=I0d, n_sweeps=n_sweeps)
    J.setflags(write=False)
    return J


# ---- the tests -----------------------------------------------------------------------------------------------------------
def test_direction_set_fits_one_plan_and_holds_both_kinds():
    ds = directions()
    assert len(ds) == 64                                     # kMaxAngles of one plan
    for d in ds:
        assert abs(np.sqrt((d.k * d.k).sum()) - 1.0) < 1e-6, d            # plan_select_angles
    assert {d.cls for d in ds} == {"axis", "face", "body", "ulp_axis", "ulp_face", "ulp_body", "generic"}
    assert sum(1 for d in ds if d.k[0] == 0.0) >= 8 and {d.d for d in ds if d.k[0] == 0.0} == {1, -1}
    for d in ds:
        if d.tie is not None:
            base = next(b for b in ds if b.label == d.tie)
            diff = np.nonzero(d.k != base.k)[0]
            assert diff.size == 1 and d.k[diff[0]] in (np.nextafter(base.k[diff[0]], np.inf), np.nextafter(base.k[diff[0]], -np.inf))
    resid = [d for d in ds if d.cls == "generic"]
    assert any(0 < abs(v) < 1e-15 for d in resid for v in d.k)             # direction() leaves residues: the control


def test_grids_are_what_they_claim():
    g = grids()
    sizes = {name: g[name][0].shape[0] for name in GRIDS}
    print("sites:", sizes)
    assert max(sizes.values()) <= 300
    assert sum(1 for n in sizes.values() if n % 16 != 0 and n % 4 != 0) >= 2
    for name in ("shells", "shells-ragged", "periodic-tie", "periodic-tie2", "coincident", "bcc0"):
        pos = g[name][0]
        assert np.array_equal(pos * 16.0, np.round(pos * 16.0)), name      # binary-exact coordinates
    # bcc0: 14 entries plus a wall in the boundary cells, rows shuffled
    nbr = g["bcc0"][1]
    assert nbr[0].max() == 14 and ((nbr[1:] == synth.BOTTOM_WALL).sum(axis=0) <= 1).all() and (nbr[1:] == synth.TOP_WALL).any()
    assert not np.array_equal(nbr[1:], np.sort(nbr[1:], axis=0))
    # shells: rows of 56 entries in the interior (4 chunks)
    assert g["shells"][1][0].max() == 56
    for name in GRIDS:                                       # symmetric adjacency everywhere
        nbr = g[name][1]
        rows = [set(int(v) for v in nbr[1:nbr[0, i] + 1, i] if v > 0) for i in range(nbr.shape[1])]
        for i, row in enumerate(rows):
            assert i + 1 not in row and len(row) == int((nbr[1:nbr[0, i] + 1, i] > 0).sum()), (name, i)
            for q in row:
                assert i + 1 in rows[q - 1], (name, i, q)


@pytest.mark.parametrize("name", GRIDS)
def test_grid_preparation_accepts_every_grid_as_the_oracle_does(name):
    """the library's host-side preparation (a handle without a device) refuses none of them, the coincident pair
    included, and layers them as the oracle does"""
    import voronoirt_amd as vrt
    hs = vrt.VoronoiSites(*grids()[name], device=-1)
    so = oracle_sites(name)
    for key in ("layers_up", "layers_down", "perm_up", "perm_down"):
        assert np.array_equal(getattr(hs, key), getattr(so, key)), key
    assert hs.max_neighbours == so.D
    hs.close()


def test_ragged_rows_span_one_to_four_chunks_inside_one_wave():
    nbr = grids()["shells-ragged"][1]
    cnt = nbr[0]
    chunks = (cnt + CHUNK - 1) // CHUNK
    print("shells-ragged: row lengths %d .. %d, rows per chunk count %s" % (cnt.min(), cnt.max(), np.bincount(chunks).tolist()))
    assert set(chunks.tolist()) == {1, 2, 3, 4}
    waves = [chunks[s:s + 4] for s in range(0, cnt.size, 4)]
    mixed = sum(1 for w in waves if w.min() == 1 and w.max() >= 3)
    print("shells-ragged: aligned groups of four site ids with a 1-chunk and a >= 3-chunk row:", mixed)
    assert mixed >= 5
    assert (cnt % CHUNK == 0).any() and (cnt % CHUNK == 1).any()
    assert cnt.size % 4 != 0                                 # the last wave's tail groups are clamped to site n - 1
    assert chunks[-1] != chunks[-2] or chunks[-2] != chunks[-3] or cnt.size % 4 == 2


@pytest.mark.parametrize("name", GRIDS)
def test_oracle_and_pyref_agree_bit_for_bit(name):
    """calc_Delaunay_lines and smallest_angle of the C oracle against the pure-Python restatement on every (grid,
    direction, site): the reference of the GPU half, no product code involved.  status == 0 for every site."""
    pos, nbr, bounds = grids()[name]
    so = oracle_sites(name)
    n, D = so.n, so.D
    P = [None] + [[0.0] + [float(v) for v in pos[i]] for i in range(n)]
    N = [None] + [[0] + [int(v) for v in nbr[:, i]] for i in range(n)]
    lines = pyref.calc_delaunay_lines(P, N, n, bounds[2], bounds[3], bounds[4], bounds[5])
    m = valid_line_mask(so)
    ref = np.full((n, D, 3), np.nan)
    for (j, i), v in lines.items():
        ref[i - 1, j - 1] = v[1:]
    assert lines_equal(ref[m], so.delaunay_lines[m])
    assert len(lines) == int(m.sum())
    tabs = oracle_tables(name)
    for d, (up, dots, w, r, st) in zip(directions(), tabs):
        assert (st == 0).all(), d
        kk = [0.0] + [float(v) for v in d.k]
        for i in range(n):
            pd, pi = pyref.smallest_angle(i + 1, N[i + 1][1:N[i + 1][1] + 2], kk, lines)
            assert pi[1] == up[i, 0] and pi[2] == up[i, 1], (d, i)
            assert pd[1] == dots[i, 0] and pd[2] == dots[i, 1], (d, i)
            rc, od, oi = orc.smallest_angle(i, so, d.k) if i % 7 == 0 else (0, dots[i], up[i])
            assert rc == 0 and np.array_equal(od, dots[i]) and np.array_equal(oi, up[i])


# floors: a handful of sites in the worst direction class that is built to hold the case (the counts are printed)
FLOORS = {
    # (grid, class of decision point): (direction classes summed over, floor of the number of (direction, site) pairs)
    ("cubic", "max_tie_in_chunk"): (("face", "body"), 100),
    ("cubic", "zero_dot"): (("axis",), 6 * 100),
    ("cubic", "minus_one_dot"): (("axis",), 6 * 90),
    ("cubic", "collapse_eq_0"): (("axis",), 6 * 90),
    ("cubic", "collapse_lt_0"): (("generic",), 10),
    ("cubic", "slot2_tie"): (("body",), 50),
    ("cubic", "nan_line"): (("axis",), 6 * 10),
    ("bcc0", "max_tie_in_chunk"): (("face", "axis"), 100),
    ("bcc0", "slot2_tie"): (("axis", "face", "body"), 100),
    ("bcc0", "zero_dot"): (("axis", "face"), 500),
    ("bcc0", "minus_one_dot"): (("axis", "body"), 500),
    ("bcc0", "wall_inside_chunk"): (("axis",), 6 * 20),
    ("shells", "max_tie_in_chunk"): (("axis", "face", "body"), 500),
    ("shells", "max_tie_across_chunks"): (("axis", "face", "body"), 500),
    ("shells", "slot2_tie"): (("axis", "face", "body"), 500),
    ("shells", "zero_dot"): (("axis",), 6 * 140),
    ("shells", "minus_one_dot"): (("axis",), 6 * 100),
    ("shells", "wall_inside_chunk"): (("axis",), 6 * 30),
    ("shells-ragged", "max_tie_across_chunks"): (("axis", "face", "body"), 200),
    ("shells-ragged", "slot2_tie"): (("axis", "face", "body"), 200),
    ("shells-ragged", "collapse_eq_0"): (("axis",), 5),
    ("periodic-tie", "max_tie_across_chunks"): (("axis", "face", "body"), 100),
    ("periodic-tie", "nan_line"): (("axis",), 6 * 10),
    ("coincident", "nan_line"): (("axis",), 6 * 2),
}


@pytest.mark.parametrize("name", GRIDS)
def test_each_class_contains_what_it_is_named_for(name):
    counts = class_counts(name)
    ds = directions()
    by_cls = sorted({d.cls for d in ds})
    print()
    for c in CLASSES:
        print("%-14s %-22s" % (name, c) + "  ".join("%s %4d" % (cls, sum(v for d, v in zip(ds, counts[c]) if d.cls == cls))
                                                    for cls in by_cls))
    for (g, c), (classes, floor) in FLOORS.items():
        if g == name:
            got = sum(v for d, v in zip(ds, counts[c]) if d.cls in classes)
            assert got >= floor, (g, c, got, floor)
    if name != "periodic-tie2":                              # (its rows have 9 entries: one chunk, little to decide)
        for c in ("zero_dot", "minus_one_dot", "collapse_eq_0", "collapse_lt_0"):
            assert sum(counts[c]) >= 5, (name, c)


def test_every_decision_point_is_held_by_some_grid():
    total = {c: sum(sum(class_counts(name)[c]) for name in GRIDS) for c in CLASSES}
    print("(direction, site) pairs over all grids:", total)
    for c in CLASSES:
        assert total[c] >= 50, c


@pytest.mark.parametrize("name", GRIDS)
def test_one_ulp_either_side_of_a_tie_picks_the_other_id(name):
    """a direction one ulp off a tie direction breaks the tie by value, whatever the row order: for a counted number of
    sites one of the two neighbours of a tie direction picks another slot-1 or slot-2 id than the tie direction"""
    ds = directions()
    tabs = oracle_tables(name)
    idx = {d.label: a for a, d in enumerate(ds)}
    flips = {}
    for a, d in enumerate(ds):
        if d.tie is not None:
            other = (tabs[a][0] != tabs[idx[d.tie]][0]).any(axis=1)
            flips.setdefault(d.cls, []).append(int(other.sum()))
    print("%-14s sites whose ids differ from the tie direction's, per one-ulp direction: %s" % (name, flips))
    if name != "periodic-tie2":
        for cls in ("ulp_axis", "ulp_face", "ulp_body"):
            assert sum(flips[cls]) >= 20, (name, cls)


@pytest.mark.parametrize("name", ORDER_GRIDS)
def test_row_order_changes_the_choice_under_ties(name):
    ds = directions()
    base = oracle_tables(name)
    for seed in ORDER_SEEDS:
        tabs = oracle_tables(name, seed)
        changed = {}
        for a, d in enumerate(ds):
            c = int((tabs[a][0] != base[a][0]).any(axis=1).sum())
            changed[d.cls] = changed.get(d.cls, 0) + c
            assert np.array_equal(tabs[a][1][:, 0], base[a][1][:, 0]), d   # the maximum belongs to the set, not to its order
        print("%-8s order seed %d: (direction, site) pairs whose ids changed, per class: %s" % (name, seed, changed))
        assert changed["axis"] + changed["face"] + changed["body"] >= 100


def test_periodic_test_sits_on_the_equality_and_the_mirror_branch_is_taken():
    """x_r_r + x_i_l == px - qx bit for bit (strict '<': no shift) for a counted number of (site, slot) pairs, the
    left-edge MIRROR branch for others; the same for y"""
    for name, floor_eq, floor_mirror in (("periodic-tie", 200, 200), ("periodic-tie2", 20, 0), ("cubic", 0, 20)):
        pos, nbr, bounds = grids()[name]
        eq = mirror = shift = 0
        for axis, lo, hi in ((1, bounds[2], bounds[3]), (2, bounds[4], bounds[5])):
            for i in range(pos.shape[0]):
                p = pos[i, axis]
                for q in nbr[1:nbr[0, i] + 1, i]:
                    if q > 0:
                        qv = pos[q - 1, axis]
                        right = (hi - p) + abs(qv - lo)
                        left = (p - lo) + abs(hi - qv)
                        eq += right == p - qv
                        shift += right < p - qv
                        mirror += (not right < p - qv) and left < qv - p
        print("%-13s periodic test: %d (site, slot) pairs on the equality, %d shifted, %d mirrored" % (name, eq, shift, mirror))
        assert eq >= floor_eq and mirror >= floor_mirror
    # the equality means "no shift": the line of such a pair points the long way, inside the box
    pos, nbr, bounds = grids()["periodic-tie"]
    so = oracle_sites("periodic-tie")
    seen = 0
    for i in range(so.n):
        for j in range(int(nbr[0, i])):
            q = nbr[j + 1, i]
            if q > 0 and (bounds[3] - pos[i, 1]) + abs(pos[q - 1, 1] - bounds[2]) == pos[i, 1] - pos[q - 1, 1]:
                d = pos[q - 1] - pos[i]
                if pos[q - 1, 2] == pos[i, 2]:
                    assert np.array_equal(so.delaunay_lines[i, j], d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
                    seen += 1
    assert seen >= 20


def test_coincident_sites_are_accepted_with_a_nan_line_both_ways():
    """the oracle does not refuse the grid: the two lines are NaN, every comparison skips them, status stays 0"""
    pos, nbr, _ = grids()["coincident"]
    a, b = COINCIDENT_SITE, COINCIDENT_SITE + 30
    assert np.array_equal(pos[a], pos[b])
    so = oracle_sites("coincident")
    ja = int(np.nonzero(nbr[1:, a] == b + 1)[0][0])
    jb = int(np.nonzero(nbr[1:, b] == a + 1)[0][0])
    assert np.isnan(so.delaunay_lines[a, ja]).all() and np.isnan(so.delaunay_lines[b, jb]).all()
    for d, (up, dots, w, r, st) in zip(directions(), oracle_tables("coincident")):
        assert (st == 0).all()
        assert b + 1 not in up[a] and a + 1 not in up[b], d


@pytest.mark.parametrize("name", SOLVE_GRIDS)
def test_solves_visit_only_sites_with_an_upwind_and_stay_finite(name):
    so = oracle_sites(name)
    ds = [directions()[a] for a in solve_directions(name)]
    left_out = [d.label for a, d in enumerate(directions()) if a not in solve_directions(name)]
    print("%-14s %d directions solved; weights 0 / 0 at a visited site, tables only: %s" % (name, len(ds), left_out))
    assert len(ds) >= 40 and {d.cls for d in ds} == {d.cls for d in directions()}
    assert sum(1 for d in ds if d.k[0] == 0.0) >= 2 and {d.d for d in ds} == {1, -1}
    for nlam, n_sweeps in ((1, 1), (3, 3)):
        I = oracle_solves(name, nlam, n_sweeps)
        assert np.isfinite(I).all() and np.isfinite(oracle_J(name, nlam, n_sweeps)).all()
    _, alpha, _, _ = solve_problem(name, 3)
    step = np.diff(np.unique(so.positions[:, 0])).min()
    dtau = alpha * step
    assert (dtau < 5e-4).any() and (dtau > 50).any() and ((dtau > 5e-4) & (dtau < 50)).any()
