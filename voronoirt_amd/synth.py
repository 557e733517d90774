"""Seeded synthetic grids and fields.

The reference builds its Voronoi grids by rejection-sampling sites from a Bifrost snapshot
(src/sample_grids.jl:223-230, src/compare_line.jl:64-106) and running voro++
(rt_preprocessing/output_sites.cc:35-49).  Neither the snapshot nor voro++ exists in the build
image, so the grids used by the tests and the benchmark are generated here, in the same
formats the reference's `read_cell` consumes (src/voronoi_utils.jl:36-63):

  G1  `bcc_grid`      jittered body-centred-cubic lattice, any size, numpy only.  The BCC
                      Voronoi cell (truncated octahedron) is a simple polytope, so its 14-face
                      topology is exact under small jitter.  Site ids are randomly permuted
                      (the reference's sites come out of a sampler in random order) and every
                      neighbour row is shuffled (voro++ face order is arbitrary).
  G2  `voronoi_grid`  a true periodic-xy / walled-z Voronoi tessellation from
                      scipy.spatial.Delaunay with periodic and mirror image points, for the
                      small committed parity fixtures; `voronoi_neighbours` does the same for
                      GIVEN sites (in-process stand-in for the voro++ preprocessing step).

Array conventions follow the reference (Julia, 1-based ids):
  positions  (n, 3) float64 C-order, columns (z, x, y)   == Julia positions[3, n]
  neighbours (D+1, n) int64 C-order, row 0 = count       == Julia neighbours[n, D+1]
             ids 1-based; -5 = bottom wall (z_min), -6 = top wall (z_max)
  bounds     (z_min, z_max, x_min, x_max, y_min, y_max)   (src/io.jl:122-124)
"""
from __future__ import annotations

import numpy as np

BOTTOM_WALL = -5   # src/voronoi_utils.jl:97
TOP_WALL = -6      # src/voronoi_utils.jl:141

# Bifrost-shaped box: x,y in [0, 6 Mm] periodic, z from -0.5 Mm upwards
BOX_XY = 6.0e6
Z_MIN = -0.5e6

# a, c of the BCC lattice for the BASELINE configs (2*a*a*c sites)
BCC_CONFIGS = {
    "C2": (37, 90),     # 246 420 sites
    "C3": (59, 143),    # 995 566 sites
    "C4": (59, 143),
    "C5": (94, 227),    # 4 011 544 sites
}


def _pack_rows(cols: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """cols: (n, K) int64 candidate neighbour ids, 0 = empty slot.  Shuffles each row, moves
    the non-empty entries to the front and returns the (D+1, n) reference matrix."""
    n, K = cols.shape
    keys = rng.random((n, K))
    keys[cols == 0] = 2.0                       # empties sort last
    order = np.argsort(keys, axis=1, kind="stable")
    packed = np.take_along_axis(cols, order, axis=1)
    counts = (packed != 0).sum(axis=1)
    D = int(counts.max())
    out = np.zeros((D + 1, n), dtype=np.int64)
    out[0] = counts
    out[1:] = packed[:, :D].T
    return out


def bcc_grid(a: int, c: int, seed: int, jitter: float = 0.05, box_xy: float = BOX_XY,
             z_min: float = Z_MIN, permute_ids: bool = True):
    """G1: jittered BCC lattice of a x a x c cubic cells (2*a*a*c sites).

    Returns (positions (n,3) [z,x,y], neighbours (D+1,n), bounds)."""
    if a < 3 or c < 2:
        raise ValueError("bcc_grid needs a >= 3 and c >= 2")
    rng = np.random.default_rng(seed)
    h = box_xy / a
    ncell = a * a * c
    n = 2 * ncell
    ii, jj, kk = np.meshgrid(np.arange(a), np.arange(a), np.arange(c), indexing="ij")
    ii = ii.ravel()
    jj = jj.ravel()
    kk = kk.ravel()

    def cid(i, j, k, centre):
        """lattice id (0-based) of corner/centre site (i, j, k) with x,y wrap; -1 outside z."""
        ok = (k >= 0) & (k < c)
        v = ((np.mod(i, a) * a + np.mod(j, a)) * c + np.clip(k, 0, c - 1)) + (ncell if centre else 0)
        return np.where(ok, v, -1)

    cand_corner = []   # for corner sites: 8 centres + 6 corners
    for di in (-1, 0):
        for dj in (-1, 0):
            for dk in (-1, 0):
                cand_corner.append(cid(ii + di, jj + dj, kk + dk, True))
    for (di, dj, dk) in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        cand_corner.append(cid(ii + di, jj + dj, kk + dk, False))
    cand_centre = []   # for centre sites: 8 corners + 6 centres
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                cand_centre.append(cid(ii + di, jj + dj, kk + dk, False))
    for (di, dj, dk) in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        cand_centre.append(cid(ii + di, jj + dj, kk + dk, True))
    cand = np.concatenate([np.stack(cand_corner, 1), np.stack(cand_centre, 1)], axis=0)  # (n,14)

    # which wall replaces the missing neighbours: below -> bottom, above -> top
    kz = np.concatenate([kk, kk])
    missing = cand < 0
    wall = np.zeros(n, dtype=np.int64)
    has_missing = missing.any(axis=1)
    wall[has_missing & (kz == 0)] = BOTTOM_WALL
    wall[has_missing & (kz == c - 1)] = TOP_WALL
    if c == 1:
        raise ValueError("c must be >= 2")

    # lattice positions: corners at (k + 1/4) h, centres at (k + 3/4) h above z_min
    x = np.concatenate([ii * h, (ii + 0.5) * h])
    y = np.concatenate([jj * h, (jj + 0.5) * h])
    z = np.concatenate([z_min + (kk + 0.25) * h, z_min + (kk + 0.75) * h])
    jit = (rng.random((n, 3)) - 0.5) * (2.0 * jitter * h)
    pos_lat = np.stack([z, x, y], axis=1) + jit
    z_max = z_min + c * h
    # keep jittered sites strictly inside the periodic box
    pos_lat[:, 1] = np.mod(pos_lat[:, 1], box_xy)
    pos_lat[:, 2] = np.mod(pos_lat[:, 2], box_xy)

    # random relabelling of the sites: new id of lattice site s is newid[s] (1-based)
    if permute_ids:
        newid = rng.permutation(n).astype(np.int64) + 1
    else:
        newid = np.arange(1, n + 1, dtype=np.int64)
    cols = np.zeros((n, 15), dtype=np.int64)
    cols[:, :14] = np.where(cand >= 0, newid[np.clip(cand, 0, n - 1)], 0)
    cols[:, 14] = wall
    nbr_lat = _pack_rows(cols, rng)                   # rows still in lattice order
    inv = np.empty(n, dtype=np.int64)
    inv[newid - 1] = np.arange(n)
    positions = np.ascontiguousarray(pos_lat[inv])
    neighbours = np.ascontiguousarray(nbr_lat[:, inv])
    bounds = (z_min, z_max, 0.0, box_xy, 0.0, box_xy)
    return positions, neighbours, bounds


def voronoi_neighbours(positions: np.ndarray, bounds, margin: float = 0.3, shuffle_seed: int | None = 0):
    """Neighbour matrix of the Voronoi tessellation of GIVEN sites, periodic in x and y, walls at
    z_min / z_max: an in-process replacement (scipy/Qhull) for the reference's preprocessing
    step, which forks the voro++ program `output_sites` and parses its text output
    (src/functions.jl:13-23, rt_preprocessing/output_sites.cc:35-49, src/voronoi_utils.jl:42-63).
    positions (n, 3) columns (z, x, y) inside `bounds` = (z_min, z_max, x_min, x_max, y_min, y_max).
    Returns the (D+1, n) matrix `read_cell` would build (row 0 = count, 1-based ids, -5 / -6 walls).

    Periodicity is imposed with image copies of the sites within `margin` (fraction of the box)
    of an x/y edge; the walls with mirror images across z_min / z_max: for a point set that is
    mirror-symmetric about a plane the Voronoi cells never cross the plane, so the cell of a
    site in the augmented set is exactly the wall-cut cell voro++ reports, and a Delaunay edge
    to any bottom (top) mirror image is a face on the bottom (top) wall.  voro++ lists the faces
    of a cell in construction order, which is not reproducible here: rows are shuffled with
    `shuffle_seed` (None keeps ascending ids).  `margin` (fraction of the box whose sites get
    periodic / mirror images) must exceed a few cell diameters: with few sites or a strongly
    stratified density the sparse cells are larger than the default 0.3 and some of their neighbours
    across the seam are missed (a valid neighbour graph for the solver tests, but not the exact
    tessellation: `vrt.voro` is, see tests/test_host.py, which compares at margin > 1)."""
    from scipy.spatial import Delaunay

    base = np.ascontiguousarray(positions, dtype=np.float64)
    n = base.shape[0]
    rng = np.random.default_rng(shuffle_seed) if shuffle_seed is not None else None
    z_min, z_max, x_min, x_max, y_min, y_max = bounds
    Lz, Lx, Ly = z_max - z_min, x_max - x_min, y_max - y_min
    x, y = base[:, 1], base[:, 2]
    pts = [base]
    owner = [np.arange(n)]
    kind = [np.zeros(n, dtype=np.int64)]        # 0 site/periodic image, -5/-6 mirror image
    # periodic images (x,y), only for sites near an edge
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            if sx == 0 and sy == 0:
                continue
            sel = np.ones(n, dtype=bool)
            if sx == 1:
                sel &= (x - x_min) < margin * Lx
            if sx == -1:
                sel &= (x_max - x) < margin * Lx
            if sy == 1:
                sel &= (y - y_min) < margin * Ly
            if sy == -1:
                sel &= (y_max - y) < margin * Ly
            idx = np.nonzero(sel)[0]
            p = base[idx].copy()
            p[:, 1] += sx * Lx
            p[:, 2] += sy * Ly
            pts.append(p)
            owner.append(idx)
            kind.append(np.zeros(idx.size, dtype=np.int64))
    allp = np.concatenate(pts)
    allo = np.concatenate(owner)
    allk = np.concatenate(kind)
    # mirror images across the walls of everything (sites and periodic images) near a wall
    for wallz, tag in ((z_min, BOTTOM_WALL), (z_max, TOP_WALL)):
        near = np.abs(allp[:, 0] - wallz) < margin * Lz
        idx = np.nonzero(near & (allk == 0))[0]
        p = allp[idx].copy()
        p[:, 0] = 2.0 * wallz - p[:, 0]
        allp = np.concatenate([allp, p])
        allo = np.concatenate([allo, allo[idx]])
        allk = np.concatenate([allk, np.full(idx.size, tag, dtype=np.int64)])

    tri = Delaunay(allp)
    indptr, indices = tri.vertex_neighbor_vertices
    rows = []
    D = 0
    for i in range(n):
        nb = indices[indptr[i]:indptr[i + 1]]
        k = allk[nb]
        ids = allo[nb[k == 0]] + 1
        ids = ids[ids != i + 1]
        # a site can touch two images of the same neighbour only in tiny boxes; keep unique ids
        ids = np.unique(ids)
        ent = list(ids)
        if (k == BOTTOM_WALL).any():
            ent.append(BOTTOM_WALL)
        if (k == TOP_WALL).any():
            ent.append(TOP_WALL)
        ent = np.array(ent, dtype=np.int64)
        if rng is not None:
            rng.shuffle(ent)
        rows.append(ent)
        D = max(D, ent.size)
    neighbours = np.zeros((D + 1, n), dtype=np.int64)
    for i, ent in enumerate(rows):
        neighbours[0, i] = ent.size
        neighbours[1:ent.size + 1, i] = ent
    return neighbours


def voronoi_grid(n: int, seed: int, bounds=(0.0, 1.0, 0.0, 1.0, 0.0, 1.0), scale_height=None,
                 margin: float = 0.3):
    """G2: random sites + their true Voronoi neighbour lists (`voronoi_neighbours`).

    Sites are uniform in x,y and either uniform in z or (scale_height = H) distributed with
    density proportional to exp(-(z - z_min)/H), mimicking the reference's density-weighted
    samplers (src/sample_grids.jl:223-230)."""
    rng = np.random.default_rng(seed)
    z_min, z_max, x_min, x_max, y_min, y_max = bounds
    Lz, Lx, Ly = z_max - z_min, x_max - x_min, y_max - y_min
    x = x_min + rng.random(n) * Lx
    y = y_min + rng.random(n) * Ly
    u = rng.random(n)
    if scale_height is None:
        z = z_min + u * Lz
    else:
        H = scale_height
        z = z_min - H * np.log(1.0 - u * (1.0 - np.exp(-Lz / H)))
    base = np.stack([z, x, y], axis=1)
    neighbours = voronoi_neighbours(base, bounds, margin=margin, shuffle_seed=int(rng.integers(1 << 31)))
    return np.ascontiguousarray(base), neighbours, tuple(bounds)


def regular_lattice_grid(nx: int, ny: int, nz: int, seed: int = 0, jitter: float = 0.0):
    """Unit-cube simple-cubic lattice with 6-neighbour lists (tiny analytic test cases)."""
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    ii, jj, kk = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    ii, jj, kk = ii.ravel(), jj.ravel(), kk.ravel()

    def sid(i, j, k):
        return (np.mod(i, nx) * ny + np.mod(j, ny)) * nz + k + 1

    cols = np.zeros((n, 6), dtype=np.int64)
    cols[:, 0] = sid(ii + 1, jj, kk)
    cols[:, 1] = sid(ii - 1, jj, kk)
    cols[:, 2] = sid(ii, jj + 1, kk)
    cols[:, 3] = sid(ii, jj - 1, kk)
    cols[:, 4] = np.where(kk + 1 < nz, sid(ii, jj, np.minimum(kk + 1, nz - 1)), TOP_WALL)
    cols[:, 5] = np.where(kk - 1 >= 0, sid(ii, jj, np.maximum(kk - 1, 0)), BOTTOM_WALL)
    neighbours = _pack_rows(cols, rng)
    pos = np.stack([(kk + 0.5) / nz, (ii + 0.5) / nx, (jj + 0.5) / ny], axis=1)
    if jitter:
        pos = pos + (rng.random((n, 3)) - 0.5) * 2.0 * jitter / max(nx, ny, nz)
    return np.ascontiguousarray(pos), neighbours, (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)


# ---------------------------------------------------------------------------------------------
# text formats shared with the reference
# ---------------------------------------------------------------------------------------------
def write_sites_file(path: str, positions: np.ndarray) -> None:
    """voro++ input: "id\\tx\\ty\\tz", 1-based id (src/io.jl:16-20; the reference passes
    positions[2,:], positions[3,:], positions[1,:] because rows are (z, x, y))."""
    with open(path, "w") as f:
        for i, (z, x, y) in enumerate(positions, start=1):
            f.write(f"{i}\t{float(x)!r}\t{float(y)!r}\t{float(z)!r}\n")


def write_neighbours_file(path: str, neighbours: np.ndarray, seed: int | None = 0) -> None:
    """voro++ "%i %n" output (rt_preprocessing/output_sites.cc:49): "id n1 n2 ... nk" per cell,
    lines in arbitrary (block) order -- shuffled here when seed is not None."""
    n = neighbours.shape[1]
    order = np.arange(n)
    if seed is not None:
        np.random.default_rng(seed).shuffle(order)
    with open(path, "w") as f:
        for i in order:
            c = int(neighbours[0, i])
            f.write(" ".join([str(i + 1)] + [str(int(v)) for v in neighbours[1:c + 1, i]]) + "\n")


# ---------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return x ^ (x >> np.uint64(31))


def counter_uniform(seed: int, stream: int, index: np.ndarray) -> np.ndarray:
    """U[0,1) from a counter-based generator keyed by (seed, stream, index)."""
    with np.errstate(over="ignore"):
        key = _splitmix64(np.uint64(seed) * np.uint64(0x100000001B3) + np.uint64(stream))
        v = _splitmix64(index.astype(np.uint64) ^ key)
    return (v >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def synthetic_fields(positions: np.ndarray, bounds, nlam: int, seed: int, n_angles: int = 0,
                     alpha0: float = 1.0e-2, scale_height: float = 0.7e6,
                     site_slice: slice | None = None):
    """S(site, λ) > 0 and α(site, λ) per SURVEY 8d.

    α = α0 · exp(-(z - z_min)/H) · (1 + 0.1 u) · ψ(λ) with a Gaussian "line core" ψ, so the
    neighbour-to-neighbour Δτ spans ~1e-6 .. 1e3 over the box and all three branches of
    `linear_weights` (src/functions.jl:484-500) are exercised.  S = 1 + 0.5 sin(2π z/Lz) + 0.1 u.
    With n_angles > 0 an angle-dependent α (n_angles, n, nlam) is returned (line case, where the
    Doppler-shifted profile makes α depend on the direction, src/lambda_iteration.jl:89-96).
    Returns (S (n, nlam), alpha)."""
    z = positions[:, 0]
    n = z.size
    z_min, z_max = bounds[0], bounds[1]
    Lz = z_max - z_min
    site = np.arange(n, dtype=np.uint64)
    lam = np.arange(nlam, dtype=np.uint64)
    idx = site[:, None] * np.uint64(nlam) + lam[None, :]
    uS = counter_uniform(seed, 1, idx)
    S = 1.0 + 0.5 * np.sin(2.0 * np.pi * (z - z_min) / Lz)[:, None] + 0.1 * uS
    centre = 0.5 * (nlam - 1)
    sigma = max(nlam / 6.0, 1.0)
    lamf = np.arange(nlam, dtype=np.float64)
    strat = alpha0 * np.exp(-(z - z_min) / scale_height)
    if n_angles <= 0:
        uA = counter_uniform(seed, 2, idx)
        psi = 1.0 + 9.0 * np.exp(-((lamf - centre) / sigma) ** 2)
        alpha = strat[:, None] * (1.0 + 0.1 * uA) * psi[None, :]
        return S, alpha
    alpha = np.empty((n_angles, n, nlam))
    for a in range(n_angles):
        uA = counter_uniform(seed, 100 + a, idx)
        shift = 0.15 * sigma * np.cos(2.0 * np.pi * a / n_angles)   # direction-dependent core
        psi = 1.0 + 9.0 * np.exp(-((lamf - centre - shift) / sigma) ** 2)
        alpha[a] = strat[:, None] * (1.0 + 0.1 * uA) * psi[None, :]
    return S, alpha


# ---------------------------------------------------------------------------------------------
# rasters
# ---------------------------------------------------------------------------------------------
def atmosphere_raster(nz: int, nx: int, ny: int, seed: int, box_xy: float = BOX_XY, z_min: float = Z_MIN,
                      z_max: float = 2.5e6):
    """A seeded, Bifrost-shaped atmosphere raster (the input of the reference's samplers, src/sample_grids.jl) for
    tests and probes.

    z (nz) is non-uniform, finest at the bottom; x (nx) and y (ny) are uniform on [0, box_xy].  N_H falls by about
    10^5 over the height (from 1e23 m^-3); T has a photosphere of about 6 500 K, a minimum near 4 000 K and a
    chromospheric rise to about 2e4 K at the top; both carry small horizontal structure (a few per cent) and
    counter_uniform noise.  vx, vy, vz are a few km/s.  Arrays are (ny, nx, nz) -- Julia's (nz, nx, ny), the layout
    `initialise` and `rejection_sampling` read.  Returns a dict with z, x, y, N_H, T, vx, vy, vz."""
    if nz < 2 or nx < 2 or ny < 2:
        raise ValueError("atmosphere_raster needs at least two points per axis")
    s = np.linspace(0.0, 1.0, nz)
    z = z_min + (z_max - z_min) * (0.4 * s + 0.6 * s * s)
    x = np.linspace(0.0, box_xy, nx)
    y = np.linspace(0.0, box_xy, ny)
    h = (z - z_min) / (z_max - z_min)
    T_z = 4000.0 + 2500.0 * np.exp(-h / 0.12) + 16000.0 / (1.0 + np.exp(-(h - 0.8) / 0.05))
    logN_z = 23.0 - 5.0 * h
    X, Y = x[None, :] / box_xy, y[:, None] / box_xy
    plane = (np.sin(2 * np.pi * (3 * X + 0.25)) * np.cos(2 * np.pi * (2 * Y)) +
             0.5 * np.sin(2 * np.pi * (5 * X + 4 * Y)))                             # (ny, nx)
    idx = np.arange(ny * nx, dtype=np.uint64).reshape(ny, nx)
    noise = counter_uniform(seed, 10, idx) - 0.5
    bend = np.sin(2 * np.pi * h)[None, None, :]
    T = T_z[None, None, :] * (1.0 + 0.04 * plane[:, :, None] * bend + 0.02 * noise[:, :, None])
    N_H = 10.0 ** (logN_z[None, None, :] + 0.03 * plane[:, :, None] * (1.0 - h)[None, None, :]
                   + 0.01 * noise[:, :, None])
    v = []
    for c in range(3):
        u = counter_uniform(seed, 11 + c, idx) - 0.5
        v.append(3.0e3 * (np.cos(2 * np.pi * (X * (c + 1) + Y * (2 - c)))[:, :, None] * (0.5 + h)[None, None, :]
                          + 0.3 * u[:, :, None]))
    return {"z": z, "x": x, "y": y, "N_H": N_H, "T": T, "vx": v[0], "vy": v[1], "vz": v[2]}


def line_raster(atm: dict, nlam: int, seed: int, line_to_cont: float = 100.0):
    """Inputs of an emergent spectrum on an `atmosphere_raster`: the raster dict of api.synth_opacity (axes + velocity
    (3, ny, nx, nz) [vz, vx, vy], doppler, gamma_static, gamma_unsold, temperature, alpha_cont), raster populations
    (2, ny, nx, nz), the line's constants (a namespace with lam, planck2, lambda0, c0, hc_over_kB, strength_const, Bij,
    Bji) and src_const.  Magnitudes in SI: a 500 nm line, nlam wavelengths over +-8 Doppler widths; α_c follows N_H so
    that the continuum's τ = 1 lies inside the box, and the line centre is about `line_to_cont` times more opaque."""
    import types

    z, x, y, T, N_H = atm["z"], atm["x"], atm["y"], atm["T"], atm["N_H"]
    L = z[-1] - z[0]
    shape = T.shape
    idx = np.arange(T.size, dtype=np.uint64).reshape(shape)
    c0, kB, h, m_H = 2.99792458e8, 1.380649e-23, 6.62607015e-34, 1.6735575e-27
    lambda0 = 500e-9
    doppler = lambda0 / c0 * np.sqrt(2 * kB * T / m_H)
    n1 = 1e-6 * N_H * (1.0 + 0.1 * counter_uniform(seed, 20, idx))
    n2 = n1 * 1e-3 * (1.0 + counter_uniform(seed, 21, idx))
    alpha_cont = 30.0 / L * N_H / N_H.max()
    strength_const = line_to_cont * 30.0 / L * np.sqrt(np.pi) * doppler.mean() / (1e-6 * N_H.max())
    lam = lambda0 + doppler.mean() * np.linspace(-8.0, 8.0, nlam)
    raster = {"z": z, "x": x, "y": y, "velocity": np.stack([atm["vz"], atm["vx"], atm["vy"]]), "doppler": doppler,
              "gamma_static": 4.7e8 + 1e8 * counter_uniform(seed, 22, idx),
              "gamma_unsold": 1e-9 * (1.0 + counter_uniform(seed, 23, idx)), "temperature": T,
              "alpha_cont": alpha_cont}
    case = types.SimpleNamespace(lam=lam, planck2=2.0 * (lambda0 / lam) ** 5, lambda0=lambda0, c0=c0,
                                 hc_over_kB=h * c0 / kB, strength_const=strength_const, Bij=1.0, Bji=0.25)
    return raster, np.stack([n1, n2]), case, 2.0


def regular_line_case(nz: int, nx: int, ny: int, seed: int, nbb: int = 21, nbf: int = 6):
    """Inputs of Λ_regular's loop (src/lambda_iteration.jl:116-205) on `atmosphere_raster(nz, nx, ny, seed)` with the
    one-cell periodic ghost border of get_atmos(...; periodic=true): returns z, x, y (the ghosted axes) and the keyword
    arguments of api.LineCase on all nz (nx + 2) (ny + 2) points in Julia order (numpy (ny + 2, nx + 2, nz) flattened).

    A 2-level + continuum atom: nbb line wavelengths (log-spaced wings), two blocks of nbf bound-free wavelengths;
    magnitudes chosen so that the raster is optically thick at line centre and thin in the wings, radiative and
    collisional rates are comparable and the populations stay positive.  The fields are drawn on the interior and
    wrapped, so that the ghost points hold their interior values."""
    c0, kB, h_pl, m_H = 2.99792458e8, 1.380649e-23, 6.62607015e-34, 1.6735575e-27
    atm = atmosphere_raster(nz, nx, ny, seed)
    z = atm["z"]
    rng = np.random.default_rng(seed)
    lambda0 = 121.567e-9
    q = np.concatenate([-np.geomspace(600, 0.05, nbb // 2), [0.0], np.geomspace(0.05, 600, nbb // 2)])
    lam = np.concatenate([lambda0 * (1 + q * 2.5e3 / c0), np.linspace(22.8e-9, 91.17e-9, nbf),
                          np.linspace(91.2e-9, 364.7e-9, nbf)])
    nlam = lam.size
    blocks = np.array([0, nbb, nbb, nbb + nbf, nbb + nbf, nbb + 2 * nbf], dtype=np.int64)

    def wrap(a):                                  # (ny, nx, nz, ...) interior -> ghosted, flattened to (n, ...)
        a = np.asarray(a)
        pad = [(1, 1), (1, 1)] + [(0, 0)] * (a.ndim - 2)
        g = np.pad(a, pad, mode="wrap")
        return g.reshape((-1,) + g.shape[3:])

    shape = (ny, nx, nz)
    zeta = np.broadcast_to(((z - z[0]) / (z[-1] - z[0]))[None, None, :], shape)
    T = 6e3 + 6e3 * zeta + 200 * rng.random(shape)
    doppler = lambda0 / c0 * np.sqrt(2 * kB * T / m_H)
    n1 = 1e16 * np.exp(-3 * zeta) * (1 + 0.1 * rng.random(shape))
    lte = np.stack([n1, n1 * 1e-3 * (1 + rng.random(shape)), n1 * 1e-2 * (1 + rng.random(shape))], axis=-1)
    B0 = (1.0 + zeta)[..., None] * (1 + 0.05 * rng.random(shape + (nlam,)))
    Cm = 10 ** rng.uniform(-1, 1, shape + (3, 3))
    for d in range(3):
        Cm[..., d, d] = 0.0
    L = z[-1] - z[0]
    strength_const = 60.0 / L * doppler.mean() / n1.mean()          # line-centre τ of order 100 across the height
    lte_g = wrap(lte).T.copy()
    case = dict(
        lam=lam, blocks=blocks, lambda0=lambda0, c0=c0, velocity=wrap(rng.normal(0, 3e3, shape + (3,))),
        doppler=wrap(doppler), gamma_static=wrap(4.702e8 + 10 ** rng.uniform(7, 8.7, shape)),
        gamma_unsold=wrap(10 ** rng.uniform(-8.5, -7.5, shape)), alpha_cont=wrap(0.05 / L * np.exp(-2 * zeta)),
        eps=wrap(10 ** rng.uniform(-2.5, -0.5, shape)), temperature=wrap(T), atom_density=lte_g.sum(axis=0), B0=wrap(B0),
        lte=lte_g, C=wrap(Cm), planck2=2.0 * (lambda0 / lam) ** 5,
        sigma_bf1=1e-21 * (lam[nbb:nbb + nbf] / lam[nbb + nbf - 1]) ** 3,
        sigma_bf2=2e-21 * (lam[nbb + nbf:] / lam[-1]) ** 3, strength_const=strength_const, Bij=1.0, Bji=0.25,
        sigma_bb_const=2e-32, hc_over_kB=h_pl * c0 / kB, pref_ij=2e36, pref_ji=2e37)
    from .api import periodic_axis
    return z, periodic_axis(atm["x"]), periodic_axis(atm["y"]), case


def three_wavelength_line_case(nz: int, nx: int, ny: int, seed: int):
    """`regular_line_case` at the smallest odd wavelength count a line case can have: 22.8 nm, 91.2 nm and the line centre.
    Every block needs two wavelengths, so the three overlap: both bound-free blocks are [0, 2), the line block is [1, 3).
    Not an atom anyone would model, but a valid input, with positive S and populations over the iterates, whose n nλ is
    odd whenever n is."""
    z, x, y, case = regular_line_case(nz, nx, ny, seed, nbb=1, nbf=1)
    order = np.argsort(case["lam"])
    lam = case["lam"][order]
    case.update(lam=lam, planck2=case["planck2"][order], B0=np.ascontiguousarray(case["B0"][:, order]),
                blocks=np.array([1, 3, 0, 2, 0, 2], dtype=np.int64), sigma_bf1=1e-21 * (lam[:2] / lam[1]) ** 3,
                sigma_bf2=2e-21 * (lam[:2] / lam[1]) ** 3)
    return z, x, y, case


# ---------------------------------------------------------------------------------------------
# the continuum scattering case (src/lambda_continuum.jl)
# ---------------------------------------------------------------------------------------------
def _planck_kW_nm(lam, T):
    """B_λ(T) in kW nm^-1 m^-2 sr^-1 (the reference's unit), lam in m"""
    h_pl, c0, kB = 6.62607015e-34, 2.99792458e8, 1.380649e-23
    return 1e-12 * 2.0 * h_pl * c0 ** 2 / lam ** 5 / np.expm1(h_pl * c0 / (lam * kB * T))


def _continuum_fields(h, T, strat, nlam: int, seed: int, idx):
    """α, ε, B_0 (..., nlam) from the relative height h in [0, 1], the temperature and the α stratification (1 / m)"""
    lam = 500e-9 * (1.0 + 0.1 * np.arange(nlam))
    idl = idx[..., None] * np.uint64(nlam) + np.arange(nlam, dtype=np.uint64)
    colour = 1.0 + 0.3 * np.arange(nlam) / max(nlam, 1)                    # a little redder, a little more opaque
    alpha = strat[..., None] * colour * (1.0 + 0.1 * counter_uniform(seed, 31, idl))
    # ε from about 1 at the bottom to about 1e-6 at the top: thick (> 1e-4) below h of about 0.65, thin above
    eps = 10.0 ** (-6.0 * h[..., None]) * (1.0 - 0.3 * counter_uniform(seed, 32, idl))
    B0 = _planck_kW_nm(lam, T[..., None] * (1.0 + 0.01 * counter_uniform(seed, 33, idl)))
    return alpha, eps, B0


def continuum_case(positions: np.ndarray, bounds, nlam: int = 1, seed: int = 0, eps_thick: float = 1e-4):
    """Inputs of Λ_voronoi's continuum loop (src/lambda_continuum.jl:109-160) on the sites of a grid: the keyword
    arguments of api.ContinuumCase, arrays (n, nlam), wavelengths 500 nm (1 + 0.1 l).

    α falls exponentially with height so that τ = 1 lies inside the box (τ of the whole height about 6); ε = α_a / α_cont
    runs from about 1 at the bottom to about 1e-6 at the top, so that thin AND thick entries exist at every wavelength
    and the masked and the unmasked criterion differ; B_0 is the Planck function of a temperature with a photosphere,
    a minimum and a chromospheric rise, in kW nm^-1 m^-2 sr^-1."""
    z = positions[:, 0]
    z_min, z_max = bounds[0], bounds[1]
    h = (z - z_min) / (z_max - z_min)
    T = 4000.0 + 2500.0 * np.exp(-h / 0.12) + 6000.0 / (1.0 + np.exp(-(h - 0.8) / 0.05))
    strat = 40.0 / (z_max - z_min) * np.exp(-h / 0.15)
    alpha, eps, B0 = _continuum_fields(h, T, strat, nlam, seed, np.arange(z.size, dtype=np.uint64))
    return dict(alpha=alpha, eps=eps, B0=B0, eps_thick=eps_thick)


def regular_continuum_case(nz: int, nx: int, ny: int, seed: int, nlam: int = 1, eps_thick: float = 1e-4):
    """Inputs of Λ_regular's continuum loop (src/lambda_continuum.jl:58-107) on `atmosphere_raster(nz, nx, ny, seed)` with
    the one-cell periodic ghost border of get_atmos(...; periodic=true): returns z, x, y (the ghosted axes) and the
    keyword arguments of api.ContinuumCase on all nz (nx + 2) (ny + 2) points in Julia order (numpy (ny + 2, nx + 2, nz)
    flattened).  The fields are drawn on the interior and wrapped, so that the ghost points hold their interior values
    exactly, as `regular_line_case` does.  α follows N_H (τ = 1 inside the box), ε and B_0 as `continuum_case`, B_0 from
    the raster's temperature capped at 10 000 K."""
    atm = atmosphere_raster(nz, nx, ny, seed)
    z = atm["z"]
    shape = (ny, nx, nz)
    h = np.broadcast_to(((z - z[0]) / (z[-1] - z[0]))[None, None, :], shape)
    T = np.minimum(atm["T"], 1.0e4)
    strat = 30.0 / (z[-1] - z[0]) * atm["N_H"] / atm["N_H"].max()
    idx = np.arange(ny * nx * nz, dtype=np.uint64).reshape(shape)
    alpha, eps, B0 = _continuum_fields(h, T, strat, nlam, seed, idx)

    def wrap(a):                                  # (ny, nx, nz, nlam) interior -> ghosted, flattened to (n, nlam)
        g = np.pad(a, [(1, 1), (1, 1), (0, 0), (0, 0)], mode="wrap")
        return np.ascontiguousarray(g.reshape(-1, nlam))

    from .api import periodic_axis
    return z, periodic_axis(atm["x"]), periodic_axis(atm["y"]), dict(alpha=wrap(alpha), eps=wrap(eps), B0=wrap(B0),
                                                                     eps_thick=eps_thick)
