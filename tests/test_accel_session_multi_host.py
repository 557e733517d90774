"""Ng acceleration of the multi-device Λ-iteration session, host side (no GPU): vrt_multi_lambda_set_acceleration and
vrt_multi_lambda_last_acceleration are declared (include/voronoirt_multi_accel.h), exported and bound with the header's signatures; argument errors answer
before a device is touched; the header compiles as C; and the phases that the single-device sessions and the multi-device
session share (csrc/vrt_internal.h: schedule, record, history, order of addition, all-or-nothing commit) are driven by a
stand-alone program, tests/probes/ng_phases_main.cpp, through a REJECTED step -- one member of three reports a bad verdict
and no member's S handle may move -- which no physical case provokes reliably on the device."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

from voronoirt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrt_multi_lambda_set_acceleration", "vrt_multi_lambda_last_acceleration")


def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_multi_session_acceleration_declared_exported_and_bound():
    """the two entries stand in include/voronoirt_multi_accel.h, which voronoirt.h includes, and are exported by the
    companion library libvrt_hip_multi_accel.so (tests/test_accel_host.py keeps voronoirt.h itself free of them, and
    tests/test_host.py ties the exports of libvrt_hip.so and _lib.PROTOTYPES to voronoirt.h: the bindings have a table of
    their own and are attached to the object _lib.load() returns)"""
    _, main = _header("voronoirt.h")
    _, code = _header("voronoirt_multi_accel.h")
    assert re.search(r'^#include "voronoirt_multi_accel.h"$', main, flags=re.M)
    lib = ctypes.CDLL(_lib.ACCEL_LIB_PATH)          # the companion library, which links libvrt_hip.so
    loaded = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.MULTI_ACCEL_PROTOTYPES, name
        res, args = _lib.MULTI_ACCEL_PROTOTYPES[name]
        assert getattr(loaded, name).restype is res and list(getattr(loaded, name).argtypes) == args, name
    assert set(_lib.MULTI_ACCEL_PROTOTYPES) == set(re.findall(r"\b(vrt_[a-z_0-9]+)\s*\(", code))
    # the bindings and the declarations are the single-device session's, argument for argument
    assert _lib.MULTI_ACCEL_PROTOTYPES[NEW[0]] == _lib.PROTOTYPES["vrt_lambda_set_acceleration"]
    assert _lib.MULTI_ACCEL_PROTOTYPES[NEW[1]] == _lib.PROTOTYPES["vrt_lambda_last_acceleration"]
    args = lambda text, n: re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)", text).group(1)
    norm = lambda s: " ".join(s.replace("vrt_multi_lambda", "vrt_lambda").split())
    for name, single in zip(NEW, ("vrt_lambda_set_acceleration", "vrt_lambda_last_acceleration")):
        assert norm(args(code, name)) == norm(args(main, single)), name


def test_multi_session_acceleration_refuses_bad_arguments_without_a_device():
    """a NULL session with good and with bad settings (order 1, start 3, period 3): VRT_EINVAL in a child process that sees
    no device.  Every call passes a NULL handle, so each returns at the NULL check: what this shows is that nothing is
    touched before the arguments are judged; the settings themselves are judged by ng_check_settings, which
    tests/test_accel_host.py exercises through the single-device entries."""
    script = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from voronoirt_amd import _lib
L = _lib.load()
applied, sums, co = ctypes.c_int(7), np.zeros(5), np.zeros(2)
d = lambda a: a.ctypes.data_as(_lib.p_dbl)
rc = [L.vrt_multi_lambda_set_acceleration(None, 2, 4, 4),        # NULL session
      L.vrt_multi_lambda_set_acceleration(None, 0, 0, 0),
      L.vrt_multi_lambda_set_acceleration(None, 1, 4, 4),        # order 1
      L.vrt_multi_lambda_set_acceleration(None, 2, 3, 4),        # start 3
      L.vrt_multi_lambda_set_acceleration(None, 2, 4, 3),        # period 3
      L.vrt_multi_lambda_last_acceleration(None, ctypes.byref(applied), d(sums), d(co)),
      L.vrt_multi_lambda_last_acceleration(None, None, None, None)]
assert len(L.vrt_last_error() or b"") > 0
assert applied.value == 7 and not sums.any() and not co.any()
print(" ".join(str(r) for r in rc))
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    codes = r.stdout.split()
    assert len(codes) == 7 and all(int(c) == _lib.VRT_EINVAL for c in codes), r.stdout


def test_header_with_the_multi_session_entries_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "voronoirt.h"\n'
                   "int use(vrt_multi_lambda *s) {\n"
                   "    double sums[5], co[2], d; int applied = 0;\n"
                   "    if (vrt_multi_lambda_set_acceleration(s, 2, 4, 4)) return -2;\n"
                   "    vrt_multi_lambda_iterate(s, &d);\n"
                   "    vrt_multi_lambda_last_acceleration(s, &applied, sums, co);\n"
                   "    return applied;\n"
                   "}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_shared_ng_phases_reject_all_or_nothing(tmp_path):
    """tests/probes/ng_phases_main.cpp over the phase functions of csrc/vrt_internal.h against a fake of the HIP calls behind
    them, built with ASan + UBSan (runtimes linked in: nothing is preloaded) and run as a child process"""
    exe = tmp_path / "ng_phases_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voronoirt_amd", "csrc"), "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "probes", "ng_phases_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    assert "ok all or nothing" in out and "no S handle moved on a rejected step" in out[-1]
