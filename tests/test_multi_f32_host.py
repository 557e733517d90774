"""CPU tests of the float-storage multi-device line Λ-iteration: the new C entries are declared, exported and bound with the
header's signatures (the companion header of the acceleration entries untouched), the Python keyword refuses what it must
before it touches the library, and the rate integrals regrouped per wavelength -- the shares of tests/multi_f32_model.py,
which tests/test_multi_f32.py (GPU) splits over devices -- equal the oracle's trapezoid sums."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import voronoirt_amd as vrt
from multi_f32_model import (CASES, REGROUPING, R_of_shares, oracle_R, partition, partitions, population_sensitivity, ranges,
                             rates_case, rates_case_of, rel_per_transition, shares_model, sigma_bb, small_lambda_case, widened_J)
from voronoirt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrt_multi_lambda_create_f32", "vrt_multi_lambda_storage", "vrt_rate_shares_native_dev",
       "vrt_rate_shares_native_dev_f32", "vrt_populations_from_shares_dev")


def _kind(ctype):
    """a bound argument type reduced to what the header can tell: a scalar's type, or `pointer`"""
    return {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_double: "double"}.get(ctype, "pointer")


def test_new_entries_are_declared_exported_and_bound_with_the_headers_signatures():
    header = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if " T " in line}
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in voronoirt.h"
        declared = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            if "*" in arg or "[" in arg:
                declared.append("pointer")
            else:
                declared.append(re.match(r"(?:const )?(int64_t|int|double)\b", arg).group(1))
        assert name in exported, f"{name} is not exported"
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and [_kind(a) for a in args] == declared, (name, declared)
    # the shares entries mirror the rate entries: (handle, nlam, l0, l1, ...) and the same arguments up to pref_ji
    whole = _lib.PROTOTYPES["vrt_rates_populations_native_dev_f32"][1]
    for name in ("vrt_rate_shares_native_dev", "vrt_rate_shares_native_dev_f32"):
        args = _lib.PROTOTYPES[name][1]
        assert args[2:4] == [ctypes.c_int64, ctypes.c_int64] and args[:2] + args[4:-2] == whole[:-5]
    # the acceleration entries stay in their companion header and library, as they were
    accel = open(os.path.join(ROOT, "include", "voronoirt_multi_accel.h")).read()
    assert "f32" not in accel and "storage" not in accel
    assert set(_lib.MULTI_ACCEL_PROTOTYPES) == {"vrt_multi_lambda_set_acceleration", "vrt_multi_lambda_last_acceleration"}


def test_lambda_iteration_refuses_a_bad_storage_before_it_touches_the_library(monkeypatch):
    """ValueError for a storage that is neither 'f64' nor 'f32' and for 'f32' together with ng, as Lambda_voronoi_host;
    raised before the library is loaded or the case is read (a plan without a handle and a case that is no case)."""
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    mp = object.__new__(vrt.MultiDevicePlan)
    for storage in ("f16", "F32", None, 4):
        with pytest.raises(ValueError):
            mp.lambda_iteration(0.0, 4, None, None, storage=storage)
    with pytest.raises(ValueError):
        mp.lambda_iteration(0.0, 4, None, None, storage="f32", ng=(4, 4))
    with pytest.raises(AssertionError):                        # a good storage goes on to the library
        mp.lambda_iteration(0.0, 4, None, None, storage="f32")


@pytest.mark.parametrize("nbb, nbf", CASES)
def test_regrouped_sums_over_the_splits_equal_the_trapezoids(nbb, nbf):
    """Σ_l W_l f_l, prefactor last, summed over each partition of [0, nlam) the GPU file uses (1, 2, 3 and nlam ranges, in
    range order) against oracle.calculate_R on the same J: the largest relative difference of any of the six rates is
    printed and is at most 1e-12.  The ranges of GPU test 1 add up the same way, and a transition without a wavelength in
    a range gets exactly 0 from it."""
    n = 48
    c, r, C0 = rates_case(n, 7, nbb, nbf)
    nlam = r["lam"].size
    J = widened_J(r["J_up"], r["J_down"])
    sig = sigma_bb(c, r, C0)
    R_ref = oracle_R(c, r, C0, J)
    worst = 0.0
    for parts in partitions(nlam):
        assert parts[0][0] == 0 and parts[-1][1] == nlam and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        total = np.zeros((6, n))
        for l0, l1 in parts:
            total = total + shares_model(c, r, J, l0, l1, sig)
        worst = max(worst, max(rel_per_transition(R_of_shares(total), R_ref)))
    print(f"nbb {nbb}, nbf {nbf}: regrouped sums against calculate_R, largest relative difference {worst:.2e}")
    assert worst <= REGROUPING
    assert [b - a for a, b in partition(33, 4)] == [9, 8, 8, 8] and [b - a for a, b in partition(6, 7)] == [1] * 6 + [0]
    rg = ranges(nbb, nbf)
    assert (shares_model(c, r, J, *rg["even, from blocks[1]"], sig)[4:] == 0.0).all()
    assert (shares_model(c, r, J, *rg["odd, the bound-bound block"], sig)[:4] == 0.0).all()
    assert (shares_model(c, r, J, *rg["empty"], sig) == 0.0).all()
    l0, l1 = rg["inside the bound-bound block"]
    inside = shares_model(c, r, J, l0, l1, sig)
    assert (inside[4:] > 0).all() and (inside[:4] == 0.0).all()
    rest = shares_model(c, r, J, 0, l0, sig) + inside + shares_model(c, r, J, l1, nlam, sig)
    assert max(rel_per_transition(R_of_shares(rest), R_ref)) <= REGROUPING


def _first_sites(c, r, m):
    """the first m sites of a rates case (every per-site array cut)"""
    c = dict(c, **{k: c[k][:m] for k in ("doppler", "gamma", "T")})
    r = dict(r, **{k: r[k][:m] for k in ("J_up", "J_down", "C", "atom")}, lte=r["lte"][:, :m])
    return c, r


def test_partition_cases_of_the_gpu_file_are_well_conditioned_and_regroup(voro_small):
    """GPU test 2 holds populations to 1e-12, so it needs atmospheres on which the ORACLE's populations do not move by
    that much when its R is rounded: the largest relative change under a +-1e-15 change of every rate is printed, and is
    below 1e-13 on _lambda_case and small_lambda_case in LTE -- and above 1e-12 on the random rates of GPU test 1, which
    leave 1e-37 of the atoms in level 2.  The regrouped sums equal calculate_R on the two atmospheres as on those."""
    from test_physics import _lambda_case
    pos, _, bounds = voro_small
    for name, case in (("lambda33", _lambda_case(pos, bounds, 11)), ("small6", small_lambda_case(pos, bounds, 11))):
        c, r, C0 = rates_case_of(case, 5)
        k = population_sensitivity(c, r, C0)
        print(f"{name}: the oracle's populations move by {k:.2e} under a 1e-15 change of its R")
        assert k < 1e-13
        c, r = _first_sites(c, r, 48)
        J = widened_J(r["J_up"], r["J_down"])
        sig, R_ref = sigma_bb(c, r, C0), oracle_R(c, r, C0, J)
        for parts in partitions(r["lam"].size):
            total = sum(shares_model(c, r, J, l0, l1, sig) for l0, l1 in parts)
            worst = max(rel_per_transition(R_of_shares(total), R_ref))
            print(f"{name} in {len(parts)} ranges: regrouped sums against calculate_R {worst:.2e}")
            assert worst <= REGROUPING
    for nbb, nbf in CASES:
        k = population_sensitivity(*rates_case(1500, 7, nbb, nbf))
        print(f"random rates ({nbb}, {nbf}): the oracle's populations move by {k:.2e} under a 1e-15 change of its R")
        assert k > REGROUPING
