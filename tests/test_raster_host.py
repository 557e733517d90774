"""Raster resampling (vrt_grid_nearest, vrt_grid_to_raster[_dev], vrt_raster_to_grid[_dev]) without a GPU: the ABI,
the argument checks that run before the device is touched, and the kernels' resource usage."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vrt_grid_nearest", "vrt_grid_to_raster_dev", "vrt_raster_to_grid_dev", "vrt_grid_to_raster",
       "vrt_raster_to_grid", "vrt_grid_raster_stats"]


def test_raster_symbols_exported_and_prototyped():
    header = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert getattr(L, name) is not None
    for name in ("nearest_sites", "Voronoi_to_Raster", "Voronoi_to_Raster_inv_dist", "initialise",
                 "Voronoi_to_Raster_dev", "initialise_dev"):
        assert callable(getattr(vrt, name))


@pytest.fixture(scope="module")
def host_grid():
    pos, nbr, bounds = synth.regular_lattice_grid(4, 4, 4)
    g = vrt.VoronoiSites(pos, nbr, bounds, device=-1)
    yield g
    g.close()


def _d(a):
    return a.ctypes.data_as(_lib.p_dbl)


def _nearest(g, q, metric=0, k=1):
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    idx = np.zeros((q.shape[0], 2), dtype=np.int64)
    dist = np.zeros((q.shape[0], 2))
    return _lib.load().vrt_grid_nearest(g.handle, q.shape[0], _d(q), metric, k,
                                        idx.ctypes.data_as(_lib.p_i64), _d(dist))


AX = np.linspace(0.0, 1.0, 5)
DUMMY = ctypes.c_void_p(16)           # a device pointer the host-only grid never dereferences


def _to_raster(g, z=AX, x=AX, y=AX, metric=0, mode=1, nf=3, ld=3, dev=False, nz=None):
    z, x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, x, y))
    nz = z.size if nz is None else nz
    if dev:
        return _lib.load().vrt_grid_to_raster_dev(g.handle, nz, x.size, y.size, _d(z), _d(x), _d(y), metric, mode,
                                                  nf, ld, DUMMY, DUMMY, None)
    out = np.zeros(max(nz, 1) * x.size * y.size * max(nf, 1))
    f = np.zeros(64 * max(ld, 1))
    return _lib.load().vrt_grid_to_raster(g.handle, nz, x.size, y.size, _d(z), _d(x), _d(y), metric, mode, nf, ld,
                                          _d(f), _d(out))


def _to_grid(g, z=AX, x=AX, y=AX, nf=3, ld=3, dev=False):
    z, x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, x, y))
    if dev:
        return _lib.load().vrt_raster_to_grid_dev(g.handle, z.size, x.size, y.size, _d(z), _d(x), _d(y), nf, DUMMY,
                                                  ld, DUMMY, None)
    r = np.zeros(z.size * x.size * y.size * max(nf, 1))
    f = np.zeros(64 * max(ld, 1))
    return _lib.load().vrt_raster_to_grid(g.handle, z.size, x.size, y.size, _d(z), _d(x), _d(y), nf, _d(r), ld,
                                          _d(f))


def test_nearest_argument_checks_before_the_device(host_grid):
    g = host_grid
    ok = np.array([[0.5, 0.5, 0.5], [0.0, 0.0, 1.0]])
    assert _nearest(g, ok) == _lib.VRT_ENODEVICE
    assert _nearest(g, ok, metric=1, k=2) == _lib.VRT_ENODEVICE
    assert _nearest(g, [[0.5, 1.5, 0.5]], metric=1) == _lib.VRT_ENODEVICE      # wrapped under PERIODIC_XY
    assert _nearest(g, ok, k=0) == _lib.VRT_EINVAL
    assert _nearest(g, ok, k=3) == _lib.VRT_EINVAL
    assert _nearest(g, ok, metric=2) == _lib.VRT_EINVAL
    assert _nearest(g, [[1.0 + 1e-9, 0.5, 0.5]]) == _lib.VRT_EINVAL              # z above z_max
    assert _nearest(g, [[-1e-9, 0.5, 0.5]], metric=1) == _lib.VRT_EINVAL
    assert _nearest(g, [[0.5, 1.5, 0.5]]) == _lib.VRT_EINVAL                     # x outside, Euclidean
    assert _nearest(g, [[0.5, 0.5, -0.1]]) == _lib.VRT_EINVAL
    assert _nearest(g, [[np.nan, 0.5, 0.5]]) == _lib.VRT_EINVAL
    assert _nearest(g, [[0.5, np.inf, 0.5]], metric=1) == _lib.VRT_EINVAL


@pytest.mark.parametrize("dev", [False, True])
def test_to_raster_argument_checks_before_the_device(host_grid, dev):
    g = host_grid
    assert _to_raster(g, dev=dev) == _lib.VRT_ENODEVICE
    assert _to_raster(g, mode=2, metric=1, dev=dev) == _lib.VRT_ENODEVICE
    assert _to_raster(g, z=[0.5], x=[0.25], y=[1.0], dev=dev) == _lib.VRT_ENODEVICE     # one point per axis
    ghost = np.linspace(-0.25, 1.25, 7)                                                # periodic_borders' ghost cells
    assert _to_raster(g, x=ghost, y=ghost, metric=1, dev=dev) == _lib.VRT_ENODEVICE
    bad = [dict(x=ghost, y=ghost, metric=0),                   # outside x/y under the Euclidean metric
           dict(z=np.linspace(0.0, 1.1, 5)), dict(z=np.linspace(-0.1, 1.0, 5), metric=1),   # outside z
           dict(z=[0.0, 0.5, 0.5, 1.0]), dict(x=[0.0, 0.6, 0.4, 1.0]),                    # not strictly ascending
           dict(y=[0.0, np.nan, 1.0]),
           dict(z=[], nz=0),                                   # no point
           dict(mode=0), dict(mode=3), dict(metric=-1), dict(metric=2),
           dict(nf=0, ld=0), dict(nf=3, ld=2),
           dict(nf=1 << 62, ld=1 << 62) if dev else dict(nf=3, ld=-1)]
    for kw in bad:
        assert _to_raster(g, dev=dev, **kw) == _lib.VRT_EINVAL, kw
    # an overflowing raster size
    if dev:
        big = np.linspace(0.0, 1.0, 1 << 16)
        assert _to_raster(g, x=big, y=big, dev=True) == _lib.VRT_EINVAL


@pytest.mark.parametrize("dev", [False, True])
def test_to_grid_argument_checks_before_the_device(host_grid, dev):
    g = host_grid
    # the lattice's sites lie at (k + 0.5)/4: inside [0.125, 0.875]
    inner = np.array([0.125, 0.3, 0.875])
    assert _to_grid(g, dev=dev) == _lib.VRT_ENODEVICE
    assert _to_grid(g, z=inner, x=inner, y=inner, dev=dev) == _lib.VRT_ENODEVICE       # sites on the faces
    bad = [dict(z=[0.5]), dict(x=[0.0]),                       # fewer than two points
           dict(z=[0.0, 0.5, 0.4, 1.0]), dict(y=[0.0, 0.5, 0.5, 1.0]),
           dict(x=[0.2, 1.0]), dict(y=[0.0, 0.8]),             # sites outside the axis ranges
           dict(z=[0.13, 0.875]),
           dict(nf=0, ld=0), dict(nf=3, ld=1)]
    for kw in bad:
        assert _to_grid(g, dev=dev, **kw) == _lib.VRT_EINVAL, kw


def test_nearest_cells_option(host_grid):
    g = host_grid
    for v in ("auto", 1, 7, 256):
        g.set_option("VRT_NEAREST_CELLS", v)
    for v in ("0", "257", "x", "", "-2", "3.5"):
        with pytest.raises(vrt.VrtError):
            g.set_option("VRT_NEAREST_CELLS", v)
    g.set_option("VRT_NEAREST_CELLS", "auto")


def test_python_mirror_reaches_the_library(host_grid):
    """The mirrors hand the checks to the library: a valid call on a host-only grid is VRT_ENODEVICE."""
    g = host_grid
    with pytest.raises(vrt.VrtError) as e:
        vrt.Voronoi_to_Raster(g, np.zeros((64, 2)), AX, AX, AX)
    assert e.value.code == _lib.VRT_ENODEVICE
    with pytest.raises(vrt.VrtError) as e:
        vrt.Voronoi_to_Raster_inv_dist(g, np.zeros(64), AX, np.linspace(-0.5, 1.5, 3), AX, periodic=True)
    assert e.value.code == _lib.VRT_ENODEVICE
    with pytest.raises(vrt.VrtError) as e:
        vrt.initialise(g, AX, AX, AX, np.zeros((2, 5, 5, 5)))
    assert e.value.code == _lib.VRT_ENODEVICE
    with pytest.raises(vrt.VrtError) as e:
        vrt.nearest_sites(g, [[0.5, 2.0, 0.5]], k=2)
    assert e.value.code == _lib.VRT_EINVAL


def test_raster_kernels_use_no_scratch(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    src = os.path.join(ROOT, "voronoirt_amd", "csrc", "vrt_raster.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-fno-fast-math", "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(src), "-c", src,
                        "-o", str(tmp_path / "vrt_raster.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert all(any(k in n for n in names) for k in ("k_nearest", "k_gather", "k_trilinear")), names
    assert len(scratch) == len(names) >= 3
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
