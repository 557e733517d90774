"""Ng acceleration of the Λ-iteration sessions, host side (no GPU): the entry points are declared, exported and bound,
their argument checks answer VRT_EINVAL before a device is touched, the ctypes signatures agree with the header, and the
host-only sanitizer build still links with the new device symbols stubbed."""
import ctypes
import os
import re
import subprocess
import sys

from voronoirt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrt_ng_accelerate_dev", "vrt_lambda_set_acceleration", "vrt_regular_lambda_set_acceleration",
       "vrt_lambda_last_acceleration", "vrt_regular_lambda_last_acceleration")


def _header():
    text = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_accel_symbols_declared_and_exported():
    text, code = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    # the multi-device session gets no acceleration entry, and the header says so
    assert not re.search(r"vrt_multi_lambda_\w*acceleration\s*\(", code)
    assert "vrt_multi_lambda_* has NO acceleration entry" in text


def test_accel_prototypes_agree_with_the_header():
    """argument by argument: int -> c_int, int64_t -> c_int64, double arrays and int * -> typed pointers on the host
    side, device pointers / handles / streams -> void pointers"""
    _, code = _header()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        res, bound = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(bound) == len(args), (name, args)
        for a, b in zip(args, bound):
            if re.fullmatch(r"int \w+", a):
                want = (ctypes.c_int,)
            elif re.fullmatch(r"int64_t \w+", a):
                want = (ctypes.c_int64,)
            elif re.fullmatch(r"int \*\w+", a):
                want = (_lib.p_int,)
            elif re.fullmatch(r"double \w+\[\d\]", a):
                want = (_lib.p_dbl,)
            else:                                   # device arrays, session handles, the stream
                assert re.fullmatch(r"(const )?(double|void|vrt_lambda|vrt_regular_lambda) \*\w+", a), (name, a)
                want = (ctypes.c_void_p,)
            assert b in want, (name, a, b)


def test_accel_refuses_bad_arguments_without_a_device():
    """NULL pointers, count < 1, order outside {0, 2}, start < 4, period < 4: VRT_EINVAL, in a child process that sees no
    device (the fake handle is never dereferenced: the settings are checked first)"""
    script = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from voronoirt_amd import _lib
L = _lib.load()
d = lambda a: a.ctypes.data_as(_lib.p_dbl)
sums, co, ap = np.zeros(5), np.zeros(2), ctypes.c_int(7)
fake = ctypes.c_void_p(64)
rc = []
acc = L.vrt_ng_accelerate_dev
rc.append(acc(0, fake, fake, fake, fake, fake, d(sums), d(co), ctypes.byref(ap), None))
rc.append(acc(-5, fake, fake, fake, fake, fake, d(sums), d(co), ctypes.byref(ap), None))
for hole in range(5):
    ptrs = [fake] * 5
    ptrs[hole] = None
    rc.append(acc(8, *ptrs, d(sums), d(co), ctypes.byref(ap), None))
rc.append(acc(8, fake, fake, fake, fake, fake, None, d(co), ctypes.byref(ap), None))
rc.append(acc(8, fake, fake, fake, fake, fake, d(sums), None, ctypes.byref(ap), None))
rc.append(acc(8, fake, fake, fake, fake, fake, d(sums), d(co), None, None))
for name in ("vrt_lambda_set_acceleration", "vrt_regular_lambda_set_acceleration"):
    f = getattr(L, name)
    rc.append(f(None, 2, 4, 4))
    rc.append(f(None, 0, 0, 0))
    for order, start, period in ((1, 4, 4), (3, 4, 4), (-2, 4, 4), (2, 3, 4), (2, 4, 3), (2, 0, 0), (2, -1, 8)):
        rc.append(f(fake, order, start, period))
for name in ("vrt_lambda_last_acceleration", "vrt_regular_lambda_last_acceleration"):
    f = getattr(L, name)
    rc.append(f(None, ctypes.byref(ap), d(sums), d(co)))
    rc.append(f(fake, None, d(sums), d(co)))
print(" ".join(str(r) for r in rc))
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    codes = r.stdout.split()
    assert len(codes) == 32 and all(int(c) == _lib.VRT_EINVAL for c in codes), r.stdout


def test_accel_source_is_built_and_keeps_to_plain_cpp():
    """vrt_accel.hip is a source of the product library; it holds no inline assembly and no atomic on a floating-point
    value (the sums are reduced through fixed slots)"""
    from voronoirt_amd import build
    assert "vrt_accel.hip" in build.SOURCES
    text = open(os.path.join(ROOT, "voronoirt_amd", "csrc", "vrt_accel.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "asm" not in code and "atomic" not in code.lower() and "__builtin" not in code


def test_host_sanitizer_screen_takes_the_new_device_symbols():
    """tools/asan_host.sh check: the stub generator finds the new device-side symbols from the objects and the header"""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_host.sh"), "check"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "loads with every symbol resolved" in r.stdout
    built = re.search(r"built (\S+)/libvrt_hip\.so: (\d+) device-side symbols stubbed", r.stdout)
    assert built, r.stdout[-2000:]
    stubbed = open(os.path.join(ROOT, built.group(1), "to_stub.txt")).read().split()      # the script's own output folder
    assert len(stubbed) == int(built.group(2))
    assert "vrt_ng_accelerate_dev" in stubbed
    assert any("ng_after_iterate" in s for s in stubbed)
