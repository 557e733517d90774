"""Site sampling from a raster density (vrt_sample_sites[_dev]) without a GPU: the ABI, the argument checks that run
before the device is touched, the kernels' resource usage and the quantities the Python samplers form."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vrt_sample_sites", "vrt_sample_sites_dev"]
PY = ["rejection_sampling", "rejection_sampling_dev", "sample_from_invNH_invT", "sample_from_logNH_invT",
      "sample_from_logNH_invT_rootv", "sample_from_temp_gradient"]


def test_sample_symbols_exported_and_prototyped():
    header = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert getattr(L, name) is not None
    for name in PY:
        assert callable(getattr(vrt, name)) and name in vrt.__all__
    assert callable(synth.atmosphere_raster)


def _d(a):
    return a.ctypes.data_as(_lib.p_dbl)


Z = np.array([0.0, 0.1, 0.35, 0.6, 1.0])
X = np.linspace(-1.0, 1.0, 4)
Y = np.linspace(2.0, 3.0, 3)
Q = np.arange(Z.size * X.size * Y.size, dtype=np.float64).reshape(Y.size, X.size, Z.size)
DUMMY = ctypes.c_void_p(16)           # a device pointer that a refused call never dereferences


def _sample(z=Z, x=X, y=Y, q=Q, n=10, seed=1, batch=0, cap=0, device=0, dev=False, nz=None, null=None):
    z, x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, x, y))
    q = np.ascontiguousarray(q, dtype=np.float64)
    nz = z.size if nz is None else nz
    pos = np.zeros((min(max(n, 1), 16), 3))         # (a refused call writes nothing)
    used = ctypes.c_int64(-7)
    L = _lib.load()
    args = [None if null == c else _d(a) for c, a in enumerate((z, x, y))]
    if dev:
        rc = L.vrt_sample_sites_dev(device, nz, x.size, y.size, *args, None if null == 3 else DUMMY, n, seed, batch,
                                    cap, None if null == 4 else DUMMY, ctypes.byref(used), None)
    else:
        rc = L.vrt_sample_sites(device, nz, x.size, y.size, *args, None if null == 3 else _d(q), n, seed, batch, cap,
                                None if null == 4 else _d(pos), ctypes.byref(used))
    return rc


@pytest.mark.parametrize("dev", [False, True])
def test_sample_argument_checks_before_the_device(dev):
    # valid calls reach the device and find none
    assert _sample(dev=dev) == _lib.VRT_ENODEVICE
    assert _sample(n=1, seed=(1 << 64) - 1, batch=64, cap=1000, dev=dev) == _lib.VRT_ENODEVICE
    assert _sample(z=[0.0, 1.0], x=[0.0, 1.0], y=[0.0, 1.0], q=[1.0, 0, 0, 0, 0, 0, 0, 2.0], dev=dev) \
        == _lib.VRT_ENODEVICE
    bad = [dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=4),
           dict(device=-1),
           dict(z=[0.5], q=Q[:, :, :1]), dict(x=[0.0], q=Q[:, :1, :]), dict(y=[2.0], q=Q[:1]),   # one point
           dict(z=[], nz=0, q=Q[:, :, :0]),
           dict(z=[0.0, 0.1, 0.1, 0.6, 1.0]), dict(x=[-1.0, 0.0, -0.5, 1.0]),                  # not ascending
           dict(y=[3.0, 2.5, 2.0]), dict(z=[0.0, 0.1, np.nan, 0.6, 1.0]), dict(x=[-1.0, 0.0, 0.5, np.inf]),
           dict(z=[-1.7e308, 0.1, 0.35, 0.6, 1.7e308]),                                        # extent overflows
           dict(n=0), dict(n=-5), dict(n=1 << 31),
           dict(batch=-1), dict(cap=-1)]
    for kw in bad:
        assert _sample(dev=dev, **kw) == _lib.VRT_EINVAL, kw
    if not dev:
        # the host form also checks the quantity: finite, not constant
        for q in (np.where(Q == 7, np.nan, Q), np.where(Q == 0, -np.inf, Q), np.full_like(Q, 3.25),
                  np.where(Q == 59, 1e308, np.where(Q == 0, -1e308, Q))):
            assert _sample(q=q) == _lib.VRT_EINVAL
    # an overflowing raster size
    big = np.linspace(0.0, 1.0, 1 << 16)
    assert _sample(x=big, y=big, dev=True) == _lib.VRT_EINVAL


def test_python_mirror_reaches_the_library():
    """A valid Python call is VRT_ENODEVICE here: the checks pass and the library finds no device."""
    with pytest.raises(vrt.VrtError) as e:
        vrt.rejection_sampling(5, Z, X, Y, Q, seed=3)
    assert e.value.code == _lib.VRT_ENODEVICE
    with pytest.raises(vrt.VrtError) as e:
        vrt.rejection_sampling(5, Z, X, Y, np.ones_like(Q), seed=3)
    assert e.value.code == _lib.VRT_EINVAL and "constant" in e.value.message
    with pytest.raises(vrt.VrtError) as e:
        vrt.rejection_sampling_dev(5, Z, X, Y, 16, 3, 16, max_proposals=-1)
    assert e.value.code == _lib.VRT_EINVAL
    with pytest.raises(ValueError):
        vrt.rejection_sampling(5, Z, X, Y, Q[:, :, :4], seed=3)
    with pytest.raises(ValueError):
        vrt.rejection_sampling(5, Z, X, Y, Q, seed=-1)


@pytest.fixture
def captured(monkeypatch):
    """the quantity each sample_from_* hands to rejection_sampling"""
    seen = {}

    def fake(n_sites, z, x, y, quantity, seed, **kw):
        seen.update(n=n_sites, z=z, quantity=np.array(quantity), seed=seed, kw=kw)
        return "sampled"
    monkeypatch.setattr(api, "rejection_sampling", fake)
    return seen


def test_python_pdfs_are_the_reference_formulas(captured):
    a = synth.atmosphere_raster(9, 5, 4, seed=2)
    z, x, y, N_H, T = a["z"], a["x"], a["y"], a["N_H"], a["T"]
    vx, vy, vz = a["vx"], a["vy"], a["vz"]
    ny, nx, nz = T.shape
    assert (nz, nx, ny) == (z.size, x.size, y.size) == (9, 5, 4)

    # sample_grids.jl:223-230  log10(N_H)^(-2) * T^(-2/5)   (Julia's literal ^(-2) is i = inv(v); i*i)
    assert vrt.sample_from_invNH_invT(z, x, y, N_H, T, 77, 5, batch=64) == "sampled"
    i = 1.0 / np.log10(N_H)
    assert np.array_equal(captured["quantity"], (i * i) * T ** (-0.4))
    assert captured["n"] == 77 and captured["seed"] == 5 and captured["kw"] == {"batch": 64}
    # :198-206  log10(N_H) * T^(-2/5)
    vrt.sample_from_logNH_invT(z, x, y, N_H, T, 3, 1)
    assert np.array_equal(captured["quantity"], np.log10(N_H) * T ** (-0.4))
    # :208-221  log10(N_H) * T^(-2/5) * (vx^2 + vy^2 + vz^2)^(1/3)
    vrt.sample_from_logNH_invT_rootv(z, x, y, N_H, T, vx, vy, vz, 3, 1)
    v_sqrd = (vx * vx + vy * vy) + vz * vz
    assert np.array_equal(captured["quantity"], (np.log10(N_H) * T ** (-0.4)) * v_sqrd ** (1.0 / 3.0))
    # :97-115  |dT/dz|: plane 1 and planes 2..end-1 forward, plane end backward (Julia's 1-based planes)
    vrt.sample_from_temp_gradient(z, x, y, T, 3, 1)
    g = np.empty_like(T)
    g[:, :, 0] = (T[:, :, 1] - T[:, :, 0]) / (z[1] - z[0])
    for k in range(1, nz - 1):
        g[:, :, k] = (T[:, :, k + 1] - T[:, :, k]) / (z[k + 1] - z[k])
    g[:, :, nz - 1] = (T[:, :, nz - 1] - T[:, :, nz - 2]) / (z[nz - 1] - z[nz - 2])
    assert np.array_equal(captured["quantity"], np.abs(g))
    assert np.array_equal(captured["quantity"][:, :, -1], captured["quantity"][:, :, -2])   # the one-sided end
    assert not np.array_equal(captured["quantity"][:, :, 0], captured["quantity"][:, :, 1])


def test_atmosphere_raster_shape_and_profile():
    a = synth.atmosphere_raster(40, 6, 5, seed=4)
    b = synth.atmosphere_raster(40, 6, 5, seed=4)
    for k in ("N_H", "T", "vx", "vy", "vz"):
        assert a[k].shape == (5, 6, 40) and np.array_equal(a[k], b[k]) and np.isfinite(a[k]).all()
    dz = np.diff(a["z"])
    assert (dz > 0).all() and dz[-1] > 2 * dz[0]                           # non-uniform, finest at the bottom
    nh = a["N_H"].mean(axis=(0, 1))
    assert 3e4 < nh[0] / nh[-1] < 3e5                                      # falls by about 10^5
    t = a["T"].mean(axis=(0, 1))
    k = int(np.argmin(t))
    assert 0 < k < 39 and t[-1] > 3 * t[k] and t[0] > t[k]                 # minimum, then the chromospheric rise
    assert a["T"][:, :, 20].std() > 0 and a["vx"].std() > 1e3
    assert not np.array_equal(synth.atmosphere_raster(40, 6, 5, seed=5)["T"], a["T"])


def test_sample_kernels_use_no_scratch(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    src = os.path.join(ROOT, "voronoirt_amd", "csrc", "vrt_raster.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-fno-fast-math", "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(src), "-c", src,
                        "-o", str(tmp_path / "vrt_raster.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = dict(zip(names, (int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr))))
    for k in ("k_sample_flags", "k_sample_scan", "k_sample_write", "k_minmax"):
        hit = [n for n in names if k in n]
        assert len(hit) == 1, (k, names)
        assert scratch[hit[0]] == 0, (k, scratch)
