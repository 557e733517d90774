"""The device tessellation (vrt_tessellate_gpu / vrt_tessellate_dev, csrc/vrt_tessellate.hip) against the host code
vrt_tessellate in the same process, which tests/test_host.py pins to Qhull's neighbour sets.

General-position inputs: the two matrices are equal element for element (ids, order, counts, zero fill) and no site
needs the host (host_sites == 0).  Exactly degenerate lattices: every row holds the true face neighbours and nothing
outside the cells that touch the site.  A second library with the face capacity lowered to 16 (build.build_tess_variant)
shows the fallback path."""
import ctypes

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib, synth
from voronoirt_amd import build as vbuild

from test_tessellate_device_host import D1, host_matrix, stratified_positions, uniform_case, stratified_case

pytestmark = pytest.mark.gpu
UNIT = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)


def _ptr(a, t):
    return a.ctypes.data_as(t)


def device_matrix(pos, bounds, d1=D1, lib=None, fill=-77):
    """vrt_tessellate_gpu on device 0: (rc, matrix that started as `fill`, max_count, host_sites)"""
    L = lib or _lib.load()
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = pos.shape[0]
    M = np.full((d1, n), fill, dtype=np.int64)
    mx, hs = ctypes.c_int64(-1), ctypes.c_int64(-1)
    b = np.array(bounds, dtype=np.float64)
    rc = L.vrt_tessellate_gpu(0, n, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl), d1, _ptr(M, _lib.p_i64), ctypes.byref(mx),
                              ctypes.byref(hs))
    return rc, M, mx.value, hs.value


def assert_equal_to_host(pos, bounds):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    want, want_max = host_matrix(pos, bounds)
    rc, got, mx, hs = device_matrix(pos, bounds)
    assert rc == _lib.VRT_OK, _lib.load().vrt_last_error()
    differ = np.nonzero((got != want).any(axis=0))[0]
    assert differ.size == 0, (differ.size, [(int(i) + 1, got[:12, i].tolist(), want[:12, i].tolist()) for i in differ[:3]])
    assert mx == want_max and hs == 0
    return got


def rows_as_sets(M):
    return [frozenset(M[1:M[0, i] + 1, i].tolist()) for i in range(M.shape[1])]


@pytest.fixture(scope="module")
def case1():
    pos, bounds = uniform_case()
    return pos, bounds, host_matrix(pos, bounds)[0]


# ---- 1-5: general position ---------------------------------------------------------------------------------------------
def test_uniform_random_equals_host(case1):
    pos, bounds, want = case1
    got = assert_equal_to_host(pos, bounds)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("n, rel_h", [(3000, 0.15), (20000, 0.07)])
def test_exponentially_stratified_equals_host(n, rel_h):
    """deep shells and huge single shells for the sparse sites at the top"""
    if n == 3000:
        pos, bounds = stratified_case()
    else:
        bounds = UNIT
        pos = stratified_positions(n, 7, bounds, rel_h)
    assert_equal_to_host(pos, bounds)


def test_anisotropic_box_equals_host():
    """g_y = 1: one bucket is visited through several images in a shell"""
    rng = np.random.default_rng(1003)
    pos = np.stack([rng.random(300), rng.random(300) * 3.0, rng.random(300) * 0.5], axis=1)
    assert_equal_to_host(pos, (0.0, 1.0, 0.0, 3.0, 0.0, 0.5))


@pytest.mark.parametrize("n", [1, 2, 3, 40])
def test_few_sites(n):
    pos = np.ascontiguousarray(np.random.default_rng(2).random((40, 3))[:n])
    if n == 1:          # vrt_tessellate takes two sites and more: the host code's site-list entry is the yardstick
        rc, got, mx, hs = device_matrix(pos, UNIT)
        assert rc == _lib.VRT_OK and mx == 2 and hs == 0
        assert got[:3, 0].tolist() == [2, -5, -6] and not got[3:].any()
        want = np.zeros((D1, 1), dtype=np.int64)
        ids = np.array([1], dtype=np.int64)
        b = np.array(UNIT)
        assert _lib.load().vrt_tessellate_sites(1, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl), D1, 1, _ptr(ids, _lib.p_i64),
                                                _ptr(want, _lib.p_i64), None) == _lib.VRT_OK
        assert np.array_equal(got, want)
    else:
        got = assert_equal_to_host(pos, UNIT)
    assert all((i + 1) not in row for i, row in enumerate(rows_as_sets(got)))


def test_sites_on_the_box_faces_equal_host():
    pos = np.random.default_rng(21).random((500, 3))
    col, side = (1, 1, 2, 2, 0, 0), (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)      # x_min, x_max, y_min, y_max, z_min, z_max
    for k in range(16):
        pos[k, col[k % 6]] = side[k % 6]
    assert_equal_to_host(pos, UNIT)


# ---- 6: lattices -------------------------------------------------------------------------------------------------------
def cubic_lattice(m, scale):
    """m^3 sites at (i + 1/2) scale in a box of edge m scale; per site the true 6 face neighbours (periodic in x and
    y, a wall below the lowest and above the highest layer) and the 26 cells that touch it, as sets of ids / walls"""
    k, i, j = [a.ravel() for a in np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")]
    pos = np.ascontiguousarray(np.stack([k + 0.5, i + 0.5, j + 0.5], axis=1) * scale)
    ident = lambda kk, ii, jj: (kk * m + ii % m) * m + jj % m + 1
    faces, touch = [], []
    for s in range(m ** 3):
        f, t = set(), set()
        for dk in (-1, 0, 1):
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (dk, di, dj) == (0, 0, 0):
                        continue
                    kk = k[s] + dk
                    e = -5 if kk < 0 else (-6 if kk >= m else ident(kk, i[s] + di, j[s] + dj))
                    if e == s + 1:
                        continue                  # (never for m >= 3)
                    t.add(e)
                    if abs(dk) + abs(di) + abs(dj) == 1:
                        f.add(e)
        faces.append(f)
        touch.append(t)
    L = m * scale
    return pos, (0.0, L, 0.0, L, 0.0, L), faces, touch


@pytest.mark.parametrize("m, scale", [(6, 1.0), (12, 1.0), (6, 3.7e6), (12, 3.7e6)])
def test_cubic_lattice_rows_between_face_and_touching_neighbours(m, scale):
    pos, bounds, faces, touch = cubic_lattice(m, scale)
    rc, got, mx, hs = device_matrix(pos, bounds)
    assert rc == _lib.VRT_OK, _lib.load().vrt_last_error()
    print(f"cubic {m}^3 x {scale:g}: host_sites {hs}, max_count {mx}")
    rows = rows_as_sets(got)
    for s, row in enumerate(rows):
        assert faces[s] <= row <= touch[s], (s + 1, sorted(row), sorted(faces[s]))
        assert got[0, s] == len(row) and not got[got[0, s] + 1:, s].any()


def test_exact_bcc_lattice_rows():
    pos, lattice, bounds = synth.bcc_grid(6, 8, seed=1, jitter=0.0)
    rc, got, mx, hs = device_matrix(pos, bounds)
    assert rc == _lib.VRT_OK, _lib.load().vrt_last_error()
    print(f"exact BCC 6x6x8: host_sites {hs}, max_count {mx}")
    h = 6.0e6 / 6
    inner = (pos[:, 0] > bounds[0] + 1.5 * h) & (pos[:, 0] < bounds[1] - 1.5 * h)
    rows, lat = rows_as_sets(got), rows_as_sets(lattice)
    assert inner.sum() > 200
    for s in range(pos.shape[0]):
        true = frozenset(e for e in lat[s] if e > 0)
        if inner[s]:
            # in this honeycomb only the 14 face neighbours touch a cell
            assert rows[s] == true and len(true) == 14, (s + 1, sorted(rows[s]), sorted(true))
        else:
            assert true <= rows[s]
            if pos[s, 0] < bounds[0] + 0.5 * h:
                assert -5 in rows[s]
            if pos[s, 0] > bounds[1] - 0.5 * h:
                assert -6 in rows[s]


def test_jittered_bcc_equals_host_and_the_analytic_14():
    pos, lattice, bounds = synth.bcc_grid(7, 9, seed=4)
    got = assert_equal_to_host(pos, bounds)
    h = 6.0e6 / 7
    inner = (pos[:, 0] > bounds[0] + 1.5 * h) & (pos[:, 0] < bounds[1] - 1.5 * h)
    rows, lat = rows_as_sets(got), rows_as_sets(lattice)
    assert inner.sum() > 300 and all(rows[i] == lat[i] and len(rows[i]) == 14 for i in np.nonzero(inner)[0])


# ---- 7: determinism ----------------------------------------------------------------------------------------------------
def test_same_bytes_twice_and_on_another_stream(case1):
    import torch
    pos, bounds, want = case1
    a = device_matrix(pos, bounds)[1]
    b = device_matrix(pos, bounds)[1]
    assert a.tobytes() == b.tobytes() == want.tobytes()
    s = torch.cuda.Stream()
    t = torch.as_tensor(pos, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        M, hs = vrt.voro_dev(t, bounds)
    torch.cuda.synchronize()
    assert M.dtype == torch.int64 and tuple(M.shape) == (D1, pos.shape[0]) and M.device == t.device and hs == 0
    assert M.cpu().numpy().tobytes() == want.tobytes()
    # the wrapper with an ordinal: the rows up to the longest
    V = vrt.voro(pos, bounds, device=0)
    assert np.array_equal(V, want[: want[0].max() + 1])


def test_relabelled_sites_give_relabelled_sets(case1):
    pos, bounds, want = case1
    n = pos.shape[0]
    p = np.random.default_rng(9).permutation(n)           # new site k is old site p[k]
    new_id = np.empty(n, dtype=np.int64)
    new_id[p] = np.arange(1, n + 1)
    rc, got, _, hs = device_matrix(np.ascontiguousarray(pos[p]), bounds)
    assert rc == _lib.VRT_OK and hs == 0
    old, new = rows_as_sets(want), rows_as_sets(got)
    for k in range(n):
        assert new[k] == frozenset(e if e < 0 else int(new_id[e - 1]) for e in old[p[k]])


# ---- 8: refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_matrix_and_the_next_call_is_good(case1):
    L = _lib.load()
    pos, bounds, want = case1
    b = np.array(bounds, dtype=np.float64)

    def good():
        rc, got, _, hs = device_matrix(pos, bounds)
        assert rc == _lib.VRT_OK and hs == 0 and got.tobytes() == want.tobytes()

    # sites outside the box: the lowest is named, in the host's words
    out = pos.copy()
    out[[1700, 312, 2044], 1] = [1.5, -0.25, np.nan]
    rc, M, mx, hs = device_matrix(out, bounds)
    assert rc == _lib.VRT_EINVAL and (M == -77).all() and mx == -1 and hs == -1
    text = L.vrt_last_error()
    hostM = np.zeros((D1, out.shape[0]), dtype=np.int64)
    assert L.vrt_tessellate(out.shape[0], _ptr(out, _lib.p_dbl), _ptr(b, _lib.p_dbl), D1, _ptr(hostM, _lib.p_i64), None) == _lib.VRT_EINVAL
    assert text == L.vrt_last_error() == b"site 313 lies outside the box"
    good()
    # a matrix too narrow for the rows
    p40 = np.ascontiguousarray(np.random.default_rng(0).random((40, 3)))
    rc, M, mx, hs = device_matrix(p40, UNIT, d1=5)
    assert rc == _lib.VRT_EGRID and (M == -77).all()
    assert b"has more neighbours than the matrix holds" in L.vrt_last_error()
    good()
    # NULL pointers and n <= 0: as the host entry
    M = np.full((D1, 40), -77, dtype=np.int64)
    args = (_ptr(p40, _lib.p_dbl), _ptr(np.array(UNIT), _lib.p_dbl), D1, _ptr(M, _lib.p_i64))
    for n in (0, -3):
        assert L.vrt_tessellate(n, *args, None) == _lib.VRT_EINVAL
        assert L.vrt_tessellate_gpu(0, n, *args, None, None) == _lib.VRT_EINVAL
        assert L.vrt_tessellate_dev(0, n, *args[:3], M.ctypes.data, None, None, None) == _lib.VRT_EINVAL
    for k in (0, 1, 3):
        a = list(args)
        a[k] = None
        assert L.vrt_tessellate(40, *a, None) == _lib.VRT_EINVAL
        assert L.vrt_tessellate_gpu(0, 40, *a, None, None) == _lib.VRT_EINVAL
    assert (M == -77).all()
    good()


# ---- 9: fallback -------------------------------------------------------------------------------------------------------
def test_sites_beyond_a_lowered_capacity_are_recomputed_by_the_host(case1):
    pos, bounds, want = case1
    V = ctypes.CDLL(vbuild.build_tess_variant())
    V.vrt_tessellate_gpu.restype, V.vrt_tessellate_gpu.argtypes = _lib.PROTOTYPES["vrt_tessellate_gpu"]
    V.vrt_tessellate_capacity.restype = ctypes.c_int64
    assert V.vrt_tessellate_capacity() == 16 and _lib.load().vrt_tessellate_capacity() >= 48
    rc, got, mx, hs = device_matrix(pos, bounds, lib=V)
    assert rc == _lib.VRT_OK, _lib.load().vrt_last_error()
    print(f"face capacity 16: host_sites {hs} of {pos.shape[0]}")
    assert 0 < hs < pos.shape[0]
    assert got.tobytes() == want.tobytes() and mx == want[0].max()


# ---- 10: chain ---------------------------------------------------------------------------------------------------------
def test_sampler_to_J_through_the_device_forms_equals_the_host_chain():
    import torch
    a = synth.atmosphere_raster(48, 24, 24, seed=6)
    z, x, y = a["z"], a["x"], a["y"]
    n, nlam = 2000, 3
    inv = 1.0 / np.log10(a["N_H"])
    q = np.ascontiguousarray((inv * inv) * a["T"] ** (-2 / 5))
    bounds = (z[0], z[-1], x[0], x[-1], y[0], y[-1])
    dq = torch.as_tensor(q.ravel(), device="cuda")
    dpos = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    vrt.rejection_sampling_dev(n, z, x, y, dq.data_ptr(), 2, dpos.data_ptr(),
                               stream=torch.cuda.current_stream().cuda_stream)
    M, hs = vrt.voro_dev(dpos, bounds)
    pos = dpos.cpu().numpy()
    M = M.cpu().numpy()
    nbr_dev = np.ascontiguousarray(M[: M[0].max() + 1])
    nbr_host = vrt.voro(pos, bounds)
    assert hs == 0 and np.array_equal(nbr_dev, nbr_host)
    rng = np.random.default_rng(3)
    S = 1.0 + rng.random((n, nlam))
    alpha = (0.5 + rng.random((n, nlam))) * 4.0 / (bounds[1] - bounds[0])
    J = []
    for nbr in (nbr_dev, nbr_host):
        sites = vrt.VoronoiSites(pos, nbr, bounds)
        try:
            I0 = S[sites.perm_up[: sites.layers_up[1] - 1] - 1]
            J.append(vrt.J_lambda_voronoi(S, alpha, sites, "n1.dat", I0_up=I0))
        finally:
            sites.close()
    assert J[0].shape == (n, nlam) and np.isfinite(J[0]).all() and J[0].tobytes() == J[1].tobytes()
