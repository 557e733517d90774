"""Emergent spectra (vrt_synth_opacity*, vrt_regular_emergent_dev, vrt_top_intensity, vrt_tau_unity*) without a GPU:
the ABI, the argument checks that run before the device is touched, and the shapes the Python forms give."""
import ctypes
import os
import re

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vrt_synth_opacity_dev", "vrt_synth_opacity", "vrt_regular_emergent_dev", "vrt_top_intensity",
       "vrt_tau_unity_dev", "vrt_tau_unity"]
DUMMY = ctypes.c_void_p(16)           # a device pointer the checks never dereference


def _d(a):
    return a.ctypes.data_as(_lib.p_dbl) if a is not None else None


def test_synthesis_symbols_exported_and_prototyped():
    header = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert getattr(L, name) is not None
    for name in ("synth_opacity", "synth_opacity_dev", "top_intensity", "top_intensity_dev", "tau_unity",
                 "tau_unity_dev", "emergent_spectrum", "periodic_axis"):
        assert callable(getattr(vrt, name))


Z = np.linspace(0.0, 1.0, 6)
X = np.linspace(0.0, 2.0, 5)
Y = np.linspace(0.0, 1.0, 4)
K = np.array([-1.0, 0.0, 0.0])


def _tau_dev(z=Z, x=X, y=Y, k=K, nlam=2, alpha=DUMMY, height=DUMMY):
    z, x, y, k = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, x, y, k))
    return _lib.load().vrt_tau_unity_dev(z.size, x.size, y.size, _d(z), _d(x), _d(y), _d(k), nlam, alpha, height, None)


def test_tau_unity_argument_checks_before_the_device():
    E = _lib.VRT_EINVAL
    assert _tau_dev(k=[0.0, 1.0, 0.0]) == E                           # k_z = 0
    assert _tau_dev(k=[-0.9, 0.0, 0.0]) == E                          # not a unit vector
    assert _tau_dev(nlam=0) == E
    assert _tau_dev(x=[0.0, 0.5, 1.5, 2.0, 2.5]) == E                # not uniform
    assert _tau_dev(y=Y[::-1]) == E                                   # not ascending
    assert _tau_dev(z=[0.0, 0.2, 0.1, 0.5, 0.7, 1.0]) == E           # z not ascending
    assert _tau_dev(alpha=None) == E and _tau_dev(height=None) == E
    z, x, y, k = Z, X, Y, np.array([0.0, 1.0, 0.0])
    a, h = np.zeros((1, 6, 7, 6)), np.zeros((1, 4, 5))
    assert _lib.load().vrt_tau_unity(6, 5, 4, _d(z), _d(x), _d(y), _d(k), 1, _d(a), 0, _d(h)) == E


def _opacity_dev(nlam=2, k=K, ptr=DUMMY, S=DUMMY, A=ctypes.c_void_p(32), lam=np.array([1.0, 2.0])):
    k, lam = np.ascontiguousarray(k, dtype=np.float64), np.ascontiguousarray(lam, dtype=np.float64)
    p2 = np.ones(lam.size)
    return _lib.load().vrt_synth_opacity_dev(6, 3, 2, _d(k), nlam, _d(lam), _d(p2), 1.0, 1.0, 1.0, 1.0, 1.0, 0.25, 2.0,
                                             4.0, ptr, ptr, ptr, ptr, ptr, ptr, ptr, S, A, None)


def test_opacity_argument_checks_before_the_device():
    E = _lib.VRT_EINVAL
    assert _opacity_dev(nlam=0) == E
    assert _opacity_dev(k=[0.5, 0.5, 0.5]) == E
    assert _opacity_dev(ptr=None) == E
    assert _opacity_dev(S=None) == E
    assert _opacity_dev(S=DUMMY, A=DUMMY) == E                        # S and alpha the same array


def test_emergent_argument_checks_before_the_device():
    E = _lib.VRT_EINVAL
    L = _lib.load()
    k = np.ascontiguousarray(K)
    assert L.vrt_regular_emergent_dev(None, _d(k), 2, DUMMY, DUMMY, 3, DUMMY, None) == E     # no handle
    form, threads = ctypes.c_int(), ctypes.c_int()
    assert L.vrt_regular_last_launch_form(None, ctypes.byref(form), ctypes.byref(threads)) == E
    z, xg, yg = Z, api.periodic_axis(X), api.periodic_axis(Y)
    S = np.zeros(6 * 7 * 6)
    out = np.zeros(5 * 4)
    for kk, nlam in (([0.0, 0.0, 1.0], 1), ([-0.5, 0.0, 0.0], 1), (K, 0)):
        kk = np.ascontiguousarray(kk, dtype=np.float64)
        assert L.vrt_top_intensity(6, 7, 6, _d(z), _d(xg), _d(yg), _d(kk), nlam, _d(S), _d(S), 3, 0, _d(out)) == E
    assert L.vrt_top_intensity(6, 7, 6, _d(z), _d(xg), _d(yg), _d(k), 1, None, _d(S), 3, 0, _d(out)) == E


class _FakeLib:
    """records the sizes an entry point is called with and fills the output it was given"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_forms_shape_their_outputs(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    atm = synth.atmosphere_raster(6, 5, 4, seed=1)
    raster, pops, case, src = synth.line_raster(atm, 3, seed=1)
    S, A = vrt.synth_opacity(K, raster, pops, case, src)
    assert S.shape == A.shape == (3, 6, 7, 6)
    assert fake.calls[-1][0] == "vrt_synth_opacity" and fake.calls[-1][1][1:4] == (6, 5, 4)
    H = vrt.tau_unity(K, A, Z, X, Y)
    assert H.shape == (3, 4, 5)
    name, args = fake.calls[-1]
    assert name == "vrt_tau_unity" and args[:3] == (6, 5, 4) and args[7] == 3
    I = vrt.top_intensity(K, S, A, Z, X, Y)
    assert I.shape == (3, 4, 5)
    name, args = fake.calls[-1]
    assert name == "vrt_top_intensity" and args[:3] == (6, 7, 6) and args[7] == 3
    with pytest.raises(ValueError):
        vrt.tau_unity(K, A[:, 1:-1], Z, X, Y)                         # not ghosted
    with pytest.raises(ValueError):
        vrt.top_intensity(K, S, A[:2], Z, X, Y)
    bad = dict(raster, velocity=raster["velocity"][:2])
    with pytest.raises(ValueError):
        vrt.synth_opacity(K, bad, pops, case, src)


def test_emergent_spectrum_checks_its_inputs_before_the_device():
    pos, nbr, bounds = synth.regular_lattice_grid(4, 4, 4)
    g = vrt.VoronoiSites(pos, nbr, bounds, device=-1)
    atm = synth.atmosphere_raster(6, 5, 4, seed=1, box_xy=1.0, z_min=0.0, z_max=1.0)
    raster, _, case, src = synth.line_raster(atm, 3, seed=1)
    pops = np.ones((g.n, 3))
    with pytest.raises(ValueError):
        vrt.emergent_spectrum(g, pops[:, :1], raster, case, 180.0, 0.0, src_const=src)      # one population
    with pytest.raises(ValueError):
        vrt.emergent_spectrum(g, pops[1:], raster, case, 180.0, 0.0, src_const=src)         # not one row per site
    with pytest.raises(ValueError):
        vrt.emergent_spectrum(g, pops, dict(raster, doppler=raster["doppler"][:, :, :-1]), case, 180.0, 0.0,
                              src_const=src)
    g.close()


def test_periodic_axis_is_periodic_borders():
    a = np.array([1.0, 1.5, 2.0, 2.5])
    assert np.array_equal(api.periodic_axis(a), [0.5, 1.0, 1.5, 2.0, 2.5, 3.0])


def test_synthesis_kernels_resource_usage():
    """The new kernels compile for gfx950 without scratch (the resource report of the build)."""
    import subprocess
    src = os.path.join(ROOT, "voronoirt_amd", "csrc")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                          "-fno-fast-math", "--cuda-device-only", "-c", "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-I", src,
                          os.path.join(src, "vrt_synth.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stderr
    m = re.search(r"Function Name: (\S*k_tau_unity\S*).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    assert m and int(m.group(2)) == 0, text[-2000:]
