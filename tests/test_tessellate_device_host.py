"""CPU tests of the device tessellation's host side (no GPU): the two C entries are declared and bound, the host code's
per-site body run over a list of sites (what the device entries recompute a flagged site with) gives exactly
vrt_tessellate's rows, the Python wrappers refuse bad arguments before the library is loaded, and the host form's
device check leaves the matrix untouched."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D1 = 71


def stratified_positions(n, seed, bounds, rel_h):
    """The sites of synth.voronoi_grid(n, seed, bounds, scale_height=rel_h * Lz) without its Qhull neighbour lists
    (the same draws in the same order)."""
    rng = np.random.default_rng(seed)
    z_min, z_max, x_min, x_max, y_min, y_max = bounds
    Lz, Lx, Ly = z_max - z_min, x_max - x_min, y_max - y_min
    x = x_min + rng.random(n) * Lx
    y = y_min + rng.random(n) * Ly
    u = rng.random(n)
    H = rel_h * Lz
    z = z_min - H * np.log(1.0 - u * (1.0 - np.exp(-Lz / H)))
    return np.ascontiguousarray(np.stack([z, x, y], axis=1))


def uniform_case():
    rng = np.random.default_rng(11)
    n = 2500
    pos = np.stack([rng.uniform(0, 2, n), rng.uniform(0, 1, n), rng.uniform(0, 1, n)], axis=1)
    return np.ascontiguousarray(pos), (0.0, 2.0, 0.0, 1.0, 0.0, 1.0)


def stratified_case():
    bounds = (-0.5e6, 14.0e6, 0.0, 6.0e6, 0.0, 6.0e6)
    return stratified_positions(3000, 1002, bounds, 0.15), bounds


def _ptr(a, t):
    return a.ctypes.data_as(t)


def host_matrix(pos, bounds):
    n = pos.shape[0]
    M = np.zeros((D1, n), dtype=np.int64)
    mx = ctypes.c_int64()
    b = np.array(bounds, dtype=np.float64)
    rc = _lib.load().vrt_tessellate(n, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl), D1, _ptr(M, _lib.p_i64), ctypes.byref(mx))
    assert rc == _lib.VRT_OK
    return M, mx.value


def subset_rows(pos, bounds, lists, fill=-77):
    """vrt_tessellate_sites over each list of 1-based ids in turn, into one matrix that starts as `fill`."""
    n = pos.shape[0]
    M = np.full((D1, n), fill, dtype=np.int64)
    b = np.array(bounds, dtype=np.float64)
    worst = 0
    for ids in lists:
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        mx = ctypes.c_int64()
        rc = _lib.load().vrt_tessellate_sites(n, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl), D1, ids.size,
                                              _ptr(ids, _lib.p_i64), _ptr(M, _lib.p_i64), ctypes.byref(mx))
        assert rc == _lib.VRT_OK, _lib.load().vrt_last_error()
        worst = max(worst, mx.value)
    return M, worst


def test_header_declares_and_lib_binds_the_device_entries():
    header = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("vrt_tessellate_gpu", "vrt_tessellate_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*int device, int64_t n, const double \*" % name, code), name
        assert name in _lib.PROTOTYPES
        assert getattr(_lib.load(), name).restype is ctypes.c_int
    assert len(_lib.PROTOTYPES["vrt_tessellate_gpu"][1]) == 8 and len(_lib.PROTOTYPES["vrt_tessellate_dev"][1]) == 9
    # the header states the row order the two sides share
    assert "ascending (s, d2, j)" in header and "-5 before -6" in header


@pytest.mark.parametrize("case", [uniform_case, stratified_case])
def test_site_list_form_of_the_host_code_equals_vrt_tessellate(case):
    pos, bounds = case()
    n = pos.shape[0]
    want, want_max = host_matrix(pos, bounds)
    every = np.arange(1, n + 1)
    shuffled = np.random.default_rng(5).permutation(every)
    for lists in ([every], [every[: n // 2], every[n // 2:]], [shuffled]):
        got, got_max = subset_rows(pos, bounds, lists)
        assert np.array_equal(got, want)
        assert got_max == want_max
    # a list touches the rows of its sites only
    part, _ = subset_rows(pos, bounds, [shuffled[:100]])
    listed = np.zeros(n, dtype=bool)
    listed[shuffled[:100] - 1] = True
    assert np.array_equal(part[:, listed], want[:, listed]) and (part[:, ~listed] == -77).all()


def test_site_list_form_refuses_what_it_cannot_do():
    pos, bounds = uniform_case()
    L = _lib.load()
    b = np.array(bounds, dtype=np.float64)
    M = np.full((D1, 40), -77, dtype=np.int64)
    mx = ctypes.c_int64()
    args = (40, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl))
    for ids in ([0], [41]):
        ids = np.array(ids, dtype=np.int64)
        assert L.vrt_tessellate_sites(*args, D1, 1, _ptr(ids, _lib.p_i64), _ptr(M, _lib.p_i64), ctypes.byref(mx)) == _lib.VRT_EINVAL
    ids = np.arange(1, 41, dtype=np.int64)
    small = np.full((5, 40), -77, dtype=np.int64)
    assert L.vrt_tessellate_sites(*args, 5, 40, _ptr(ids, _lib.p_i64), _ptr(small, _lib.p_i64), ctypes.byref(mx)) == _lib.VRT_EGRID
    assert b"more neighbours than the matrix holds" in L.vrt_last_error()
    assert (M == -77).all() and (small == -77).all()
    # a single site: the walls only
    one = np.zeros((D1, 1), dtype=np.int64)
    ids = np.array([1], dtype=np.int64)
    assert L.vrt_tessellate_sites(1, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl), D1, 1, _ptr(ids, _lib.p_i64),
                                  _ptr(one, _lib.p_i64), ctypes.byref(mx)) == _lib.VRT_OK
    assert one[:3, 0].tolist() == [2, -5, -6] and not one[3:].any()


def test_wrappers_refuse_bad_arguments_before_the_library_is_loaded():
    code = r"""
import numpy as np, torch
import voronoirt_amd as vrt
from voronoirt_amd import _lib
pos = np.random.default_rng(0).random((10, 3))
b = (0, 1, 0, 1, 0, 1)
def refused(f):
    try:
        f()
    except ValueError:
        return True
    return False
assert refused(lambda: vrt.voro(pos, b, device="x"))
assert refused(lambda: vrt.voro(pos, b, device=1.5))
assert refused(lambda: vrt.voro(pos, b, device=True))
t = torch.zeros((10, 3), dtype=torch.float64)
assert refused(lambda: vrt.voro_dev(t.to(torch.float32), b))
assert refused(lambda: vrt.voro_dev(torch.zeros((10, 6), dtype=torch.float64)[:, ::2], b))
assert refused(lambda: vrt.voro_dev(torch.zeros((3, 10), dtype=torch.float64).t(), b))
assert refused(lambda: vrt.voro_dev(pos, b))
assert _lib._lib is None, "the library was loaded"
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_voro_with_device_none_is_the_host_path():
    pos, bounds = uniform_case()
    a = vrt.voro(pos[:400], bounds)
    b = vrt.voro(pos[:400], bounds, device=None)
    want, mx = host_matrix(np.ascontiguousarray(pos[:400]), bounds)
    assert a.tobytes() == b.tobytes() and np.array_equal(a, want[: mx + 1])


def test_host_form_checks_the_device_and_leaves_the_matrix():
    L = _lib.load()
    pos, bounds = uniform_case()
    pos = np.ascontiguousarray(pos[:40])
    b = np.array(bounds, dtype=np.float64)
    M = np.full((D1, 40), -77, dtype=np.int64)
    mx, hs = ctypes.c_int64(-1), ctypes.c_int64(-1)
    for device in (-1, L.vrt_device_count()):
        rc = L.vrt_tessellate_gpu(device, 40, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl), D1, _ptr(M, _lib.p_i64),
                                  ctypes.byref(mx), ctypes.byref(hs))
        assert rc in (_lib.VRT_ENODEVICE, _lib.VRT_EINVAL)
        assert (M == -77).all() and mx.value == -1 and hs.value == -1
    # the argument checks come before the device: the same refusals with and without one
    assert L.vrt_tessellate_gpu(0, 40, None, _ptr(b, _lib.p_dbl), D1, _ptr(M, _lib.p_i64), None, None) == _lib.VRT_EINVAL
    assert L.vrt_tessellate_gpu(0, 0, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl), D1, _ptr(M, _lib.p_i64), None, None) == _lib.VRT_EINVAL
    assert L.vrt_tessellate_gpu(0, 40, _ptr(pos, _lib.p_dbl), _ptr(b, _lib.p_dbl), 4, _ptr(M, _lib.p_i64), None, None) == _lib.VRT_EINVAL
    assert L.vrt_tessellate_dev(0, 40, None, _ptr(b, _lib.p_dbl), D1, None, None, None, None) == _lib.VRT_EINVAL
    assert (M == -77).all()
