"""The standalone pieces of the Ng step, host side (no GPU): the three entry points are declared, exported and bound with
the header's signatures, vrt_ng_coefficients is the host formula of tests/test_accel.py bit for bit, bad arguments answer
before a device is touched, and the header still compiles as C."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from voronoirt_amd import _lib
from test_accel import _coefficients, _geometric, _iterates, _reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrt_ng_sums_dev", "vrt_ng_coefficients", "vrt_ng_apply_dev")


def _header():
    text = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_ng_pieces_declared_and_exported():
    text, code = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name


def test_ng_pieces_prototypes_agree_with_the_header():
    _, code = _header()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        res, bound = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(bound) == len(args), (name, args)
        for a, b in zip(args, bound):
            if re.fullmatch(r"int \w+", a):
                want = ctypes.c_int
            elif re.fullmatch(r"int64_t \w+", a):
                want = ctypes.c_int64
            elif re.fullmatch(r"double \w+", a):
                want = ctypes.c_double
            elif re.fullmatch(r"int \*\w+", a):
                want = _lib.p_int
            elif re.fullmatch(r"(const )?double \w+\[\d\]", a):
                want = _lib.p_dbl
            else:                                   # device arrays, the stream
                assert re.fullmatch(r"(const )?(double|void) \*\w+", a), (name, a)
                want = ctypes.c_void_p
            assert b is want, (name, a, b)


def _lib_coefficients(sums):
    s = np.ascontiguousarray(sums, dtype=np.float64)
    out = np.full(2, -7.0)
    ok = ctypes.CDLL(_lib.LIB_PATH).vrt_ng_coefficients(s.ctypes.data_as(_lib.p_dbl), out.ctypes.data_as(_lib.p_dbl))
    return ok, out


def _sample_sums():
    """sums of the arrays tests/test_accel.py runs on the device (numpy, exact sums), and a few of mixed magnitude"""
    out = [_reference(*_iterates(count, seed=count % 1000), result=False)["sums"] for count in (63, 64, 65, 4097)]
    out += [_reference(*_geometric(l1, l2, N=2000)[1], result=False)["sums"] for l1, l2 in ((0.9, 0.5), (0.99, 0.9), (0.95, -0.3))]
    rng = np.random.default_rng(12)
    for _ in range(50):
        q = rng.normal(size=(2, 3)) * 10.0 ** rng.uniform(-8, 8)
        A1, B1, B2 = q[0] @ q[0], q[0] @ q[1], q[1] @ q[1]                      # a Gram matrix, as the sums are
        out.append(np.array([A1, B1, rng.normal() * abs(A1), B2, rng.normal() * abs(B2)]))
    return out


def test_ng_coefficients_are_the_host_formulas_bit_for_bit():
    for sums in _sample_sums():
        a, b, _ = _coefficients(sums)
        assert np.isfinite([a, b]).all()
        ok, co = _lib_coefficients(sums)
        assert ok == 1 and co.tobytes() == np.array([a, b]).tobytes(), sums


@pytest.mark.parametrize("sums", [
    [0.0, 0.0, 0.0, 0.0, 0.0],                      # four equal arrays
    [4.0, 2.0, 1.0, 1.0, 1.0],                      # det = 4 - 4 = 0: a rank-one system
    [np.nan, 1.0, 1.0, 2.0, 1.0], [1.0, 1.0, np.nan, 2.0, 1.0], [1.0, 1.0, 1.0, 2.0, np.nan],
    [np.inf, 1.0, 1.0, 2.0, 1.0], [1.0, 1.0, -np.inf, 2.0, 1.0],
    [1e200, 1.0, 1.0, 1e200, 1.0],                  # finite sums, det overflows
])
def test_ng_coefficients_refuses_a_singular_or_non_finite_system(sums):
    ok, co = _lib_coefficients(sums)
    assert ok == 0 and np.array_equal(co, [-7.0, -7.0])          # coeffs left alone


def test_ng_coefficients_null_arguments():
    f = ctypes.CDLL(_lib.LIB_PATH).vrt_ng_coefficients
    s, c = np.array([2.0, 1.0, 1.0, 2.0, 1.0]), np.zeros(2)
    assert f(None, c.ctypes.data_as(_lib.p_dbl)) == _lib.VRT_EINVAL and f(s.ctypes.data_as(_lib.p_dbl), None) == _lib.VRT_EINVAL
    assert f(s.ctypes.data_as(_lib.p_dbl), c.ctypes.data_as(_lib.p_dbl)) == 1


def test_ng_pieces_refuse_bad_arguments_without_a_device():
    """NULL pointers, count < 1: VRT_EINVAL, in a child process that sees no device"""
    script = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from voronoirt_amd import _lib
L = _lib.load()
d = lambda a: a.ctypes.data_as(_lib.p_dbl)
sums, co, good = np.zeros(5), np.zeros(2), ctypes.c_int(7)
fake = ctypes.c_void_p(64)
rc = []
for count in (0, -5):
    rc.append(L.vrt_ng_sums_dev(count, fake, fake, fake, fake, d(sums), None))
    rc.append(L.vrt_ng_apply_dev(count, 0.5, 0.25, fake, fake, fake, fake, ctypes.byref(good), None))
for hole in range(4):
    ptrs = [fake] * 4
    ptrs[hole] = None
    rc.append(L.vrt_ng_sums_dev(8, *ptrs, d(sums), None))
    rc.append(L.vrt_ng_apply_dev(8, 0.5, 0.25, *ptrs, ctypes.byref(good), None))
rc.append(L.vrt_ng_sums_dev(8, fake, fake, fake, fake, None, None))
rc.append(L.vrt_ng_apply_dev(8, 0.5, 0.25, fake, fake, fake, fake, None, None))
print(" ".join(str(r) for r in rc))
"""
    env = dict(os.environ, VRT_NO_TORCH="1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    codes = r.stdout.split()
    assert len(codes) == 14 and all(int(c) == _lib.VRT_EINVAL for c in codes), r.stdout


def test_header_with_the_new_entries_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "voronoirt.h"\n'
                   "int use(const double *x, double *o) {\n"
                   "    double sums[5], co[2]; int good = 0;\n"
                   "    vrt_ng_sums_dev(8, x, x, x, x, sums, 0);\n"
                   "    if (vrt_ng_coefficients(sums, co) == 1) vrt_ng_apply_dev(8, co[0], co[1], x, x, x, o, &good, 0);\n"
                   "    return good;\n"
                   "}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]

