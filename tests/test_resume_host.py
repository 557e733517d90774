"""Resuming the line Λ-iteration sessions from saved S and populations (vrt_lambda_set_state,
vrt_regular_lambda_set_state, vrt_multi_lambda_set_state), host side (no GPU): the three entries are declared, exported
and bound with prototypes that agree with the header, refuse a NULL session and an empty request before a device is
touched, the Python drivers carry the keywords, and the checkpoint file is written atomically and read back whole.
`small_lambda_case` is the line case of tests/test_resume.py."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib, api
from test_physics import C0, H_PLANCK, K_B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrt_lambda_set_state", "vrt_regular_lambda_set_state", "vrt_multi_lambda_set_state")
SESSION_DRIVERS = (vrt.Lambda_voronoi_host, vrt.Lambda_regular, vrt.MultiDevicePlan.lambda_iteration)


def small_lambda_case(pos, bounds, seed, nbb, nbf):
    """The line case of tests/test_physics.py::_lambda_case with nbb line wavelengths (an even count has no line-centre
    wavelength) and 2 x nbf continuum wavelengths: nλ = nbb + 2 nbf."""
    n = pos.shape[0]
    rng = np.random.default_rng(seed)
    lambda0 = 121.567e-9
    half = np.geomspace(0.05, 600, nbb // 2)
    q = np.concatenate([-half[::-1], [0.0] if nbb % 2 else [], half])
    lam = np.concatenate([lambda0 * (1 + q * 2.5e3 / C0), np.linspace(22.8e-9, 91.17e-9, nbf), np.linspace(91.2e-9, 364.7e-9, nbf)])
    nlam = lam.size
    assert nlam == nbb + 2 * nbf and (np.diff(lam[:nbb]) > 0).all()
    blocks = np.array([0, nbb, nbb, nbb + nbf, nbb + nbf, nlam], dtype=np.int64)
    z = (pos[:, 0] - bounds[0]) / (bounds[1] - bounds[0])
    T = 6e3 + 6e3 * z + 200 * rng.random(n)
    doppler = lambda0 / C0 * np.sqrt(2 * K_B * T / 1.6735575e-27)
    n1 = 1e16 * np.exp(-3 * z) * (1 + 0.1 * rng.random(n))
    lte = np.stack([n1, n1 * 1e-3 * (1 + rng.random(n)), n1 * 1e-2 * (1 + rng.random(n))])
    B0 = (1.0 + z)[:, None] * (1 + 0.05 * rng.random((n, nlam)))
    Cm = 10 ** rng.uniform(-1, 1, (n, 3, 3))
    for d in range(3):
        Cm[:, d, d] = 0.0
    box = bounds[1] - bounds[0]
    return vrt.LineCase(
        lam=lam, blocks=blocks, lambda0=lambda0, c0=C0, velocity=rng.normal(0, 3e3, (n, 3)), doppler=doppler,
        gamma_static=4.702e8 + 10 ** rng.uniform(7, 8.7, n), gamma_unsold=10 ** rng.uniform(-8.5, -7.5, n),
        alpha_cont=0.05 / box * np.exp(-2 * z), eps=10 ** rng.uniform(-2.5, -0.5, n), temperature=T,
        atom_density=lte.sum(axis=0), B0=B0, lte=lte, C=Cm, planck2=2.0 * (lambda0 / lam) ** 5,
        sigma_bf1=1e-21 * (lam[nbb:nbb + nbf] / lam[nbb + nbf - 1]) ** 3,
        sigma_bf2=2e-21 * (lam[nbb + nbf:] / lam[-1]) ** 3,
        strength_const=60.0 / box * doppler.mean() / n1.mean(), Bij=1.0, Bji=0.25, sigma_bb_const=2e-32,
        hc_over_kB=H_PLANCK * C0 / K_B, pref_ij=2e36, pref_ji=2e37)


# ---- 1: symbols ------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_resume_symbols_declared_exported_and_bound():
    text, code = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    # the header says what the call leaves alone
    assert re.search(r"J, R and γ as \*_get returns them are NOT\s+\* changed by this call", text)
    # no device-pointer variant, nothing for the continuum sessions (they have _set_source)
    assert not re.search(r"vrt_\w*set_state_dev|vrt_(regular_)?continuum_set_state", code)


def test_resume_prototypes_agree_with_the_header():
    _, code = _header()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        res, bound = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(bound) == len(args) == 3, (name, args)
        assert re.fullmatch(r"(vrt_lambda|vrt_regular_lambda|vrt_multi_lambda) \*s", args[0]) and bound[0] is ctypes.c_void_p
        assert args[0].split()[0] + "_set_state" == name
        for a, b, arg in zip(args[1:], bound[1:], ("S", "populations")):
            assert a == f"const double *{arg}" and b is _lib.p_dbl, (name, a, b)


# ---- 2: argument checks ------------------------------------------------------------------------------------------------------
def test_resume_refuses_bad_arguments_without_a_device():
    """A NULL session, and a session pointer with both arrays NULL, are VRT_EINVAL with a message, in a child process that
    sees no device (the handle is never dereferenced)."""
    script = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from voronoirt_amd import _lib
L = _lib.load()
d = lambda a: a.ctypes.data_as(_lib.p_dbl)
v = np.ones(8)
fake = ctypes.c_void_p(8)
out = []
for name in sys.argv[2].split(","):
    fn = getattr(L, name)
    for args in ((None, d(v), d(v)), (None, None, None), (None, d(v), None), (fake, None, None)):
        rc = fn(*args)
        out.append(f"{rc}:{len(L.vrt_last_error() or b'')}")
print(" ".join(out))
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT, ",".join(NEW)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    codes = [c.split(":") for c in r.stdout.split()]
    assert len(codes) == 12, r.stdout
    assert all(int(rc) == _lib.VRT_EINVAL and int(msg) > 0 for rc, msg in codes), r.stdout


# ---- 3: the Python keywords -----------------------------------------------------------------------------------------------------
def test_resume_keywords_exist_and_default_to_none():
    for fn in SESSION_DRIVERS:
        p = inspect.signature(fn).parameters
        for key in ("S0", "populations0", "checkpoint", "resume"):
            assert p[key].default is None, (fn.__name__, key)
        assert p["checkpoint_every"].default == 1, fn.__name__
    p = inspect.signature(vrt.Lambda_voronoi).parameters
    assert p["S0"].default is None and p["populations0"].default is None
    assert "checkpoint" not in p and "resume" not in p              # the torch-driven loop simply starts from the arrays


# ---- 4: the checkpoint file -----------------------------------------------------------------------------------------------------
def _state(n, nlam, seed):
    rng = np.random.default_rng(seed)
    return 1.0 + rng.random((n, nlam)), rng.random((3, n)), [1.0 / (k + 1) for k in range(seed)]


def test_checkpoint_round_trips_the_four_keys(tmp_path):
    S, pops, hist = _state(7, 5, 4)
    path = tmp_path / "run.npz"
    api.write_checkpoint(path, S, pops, 4, hist)
    assert sorted(os.listdir(tmp_path)) == ["run.npz"]              # no temporary file is left, no second suffix
    with np.load(path) as f:
        assert sorted(f.files) == sorted(api.CHECKPOINT_KEYS) == ["S", "history", "iterate", "populations"]
    ck = api.read_checkpoint(path, 7, 5)
    assert np.array_equal(ck["S"], S) and np.array_equal(ck["populations"], pops)
    assert ck["iterate"] == 4 and ck["history"] == hist and isinstance(ck["iterate"], int)
    # a target name that does not end in .npz is written under exactly that name
    other = tmp_path / "state.ckpt"
    api.write_checkpoint(other, S, pops, 4, hist)
    assert sorted(os.listdir(tmp_path)) == ["run.npz", "state.ckpt"]
    assert np.array_equal(api.read_checkpoint(other)["S"], S)


def test_checkpoint_write_is_atomic(tmp_path, monkeypatch):
    """A write that dies between the temporary file and os.replace leaves the previous checkpoint whole."""
    S, pops, hist = _state(7, 5, 3)
    path = tmp_path / "run.npz"
    api.write_checkpoint(path, S, pops, 3, hist)
    seen = {}

    def dies(src, dst):
        seen["src"], seen["dst"] = src, dst
        seen["tmp_complete"] = np.array_equal(np.load(src)["S"], 2 * S)      # the new state was all in the temporary file
        raise OSError("killed between the temporary file and the replace")

    monkeypatch.setattr(os, "replace", dies)
    with pytest.raises(OSError):
        api.write_checkpoint(path, 2 * S, pops, 4, hist + [0.1])
    monkeypatch.undo()
    assert seen["dst"] == str(path) and os.path.dirname(seen["src"]) == str(tmp_path) and seen["src"].endswith(".npz")
    assert seen["tmp_complete"]
    ck = api.read_checkpoint(path, 7, 5)
    assert np.array_equal(ck["S"], S) and ck["iterate"] == 3 and ck["history"] == hist
    assert sorted(os.listdir(tmp_path)) == ["run.npz"]


def test_checkpoint_shape_mismatch_is_a_value_error(tmp_path):
    S, pops, hist = _state(7, 5, 2)
    path = tmp_path / "run.npz"
    api.write_checkpoint(path, S, pops, 2, hist)
    for n, nlam in ((8, 5), (7, 6), (5, 7)):
        with pytest.raises(ValueError):
            api.read_checkpoint(path, n, nlam)
    # a file that is no checkpoint, and arrays that do not belong together
    np.savez(tmp_path / "other.npz", S=S)
    with pytest.raises(ValueError):
        api.read_checkpoint(tmp_path / "other.npz")
    api.write_checkpoint(tmp_path / "torn.npz", S, pops[:, :6], 2, hist)
    with pytest.raises(ValueError):
        api.read_checkpoint(tmp_path / "torn.npz")
    # the drivers check before any device work: no device is needed to be refused
    with pytest.raises(ValueError):
        api._start_state(None, None, path, 1, 8, 5, "test")
    with pytest.raises(ValueError):
        api._start_state(S, None, path, 1, 7, 5, "test")           # resume and S0 together
    with pytest.raises(ValueError):
        api._start_state(S[:, :4], None, None, 1, 7, 5, "test")
    with pytest.raises(ValueError):
        api._start_state(None, pops.T, None, 1, 7, 5, "test")
    with pytest.raises(ValueError):
        api._start_state(None, None, None, 0, 7, 5, "test")
    got = api._start_state(None, None, path, 1, 7, 5, "test")
    assert np.array_equal(got[0], S) and np.array_equal(got[1], pops) and got[2] == 2 and got[3] == hist
