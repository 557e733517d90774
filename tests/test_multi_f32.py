"""GPU tests (-m gpu) of float storage in the multi-device line Λ-iteration session: the float shares kernel
(vrt_rate_shares_native_dev_f32) against the double one on the widened J, bit for bit, over the wavelength ranges a device
can own; the shares of a partition against the one-device rates and the oracle; the session vrt_multi_lambda_create_f32
against the one-device float session (first iterate bit for bit, later ones by the conditions of oracle/f32_model.py), on
blocks down to one wavelength and none; its state entries, refusals, the Python keyword and the RCCL leg.  The bounds are
the project's figure for the regrouped sums (1e-12) and figures of the oracle runs of tests/f32_lambda_model.py."""
import ctypes
import os

import numpy as np
import pytest

import voronoirt_amd as vrt
from f32_lambda_model import deviations, f32, oracle_runs
from multi_f32_model import (CASES, REGROUPING, oracle_R, partition, partitions, ranges, rates_case, rates_case_of,
                             rel_per_transition, small_lambda_case, widened_J)
from oracle import oracle as orc
from oracle.f32_model import within_conditions
from oracle.layout_ref import pair_index as _pair_index
from voronoirt_amd import _lib, api

pytestmark = pytest.mark.gpu

W, TH, PH, NQ = vrt.read_quadrature("ul7n12.dat")
DIRS = [1 if t > 90 else -1 for t in TH]
QUAD = "ul7n12.dat"
ORACLE_ITERATES = 6             # as tests/test_f32_lambda.py: one set of oracle runs per process serves both files
# plans of the three float plane layouts (tests/test_f32_lambda.py): pairs per block 2 (default), 1 and 8
LAYOUTS = {"default": ({}, 2), "pairs": ({"VRT_PATCH_QUAD": "0"}, 1), "block8": ({"VRT_PAIR_BLOCK": "8"}, 8)}


@pytest.fixture(scope="module")
def sites(voro_small):
    pos, nbr, bounds = voro_small
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    yield hs
    hs.close()


@pytest.fixture(scope="module")
def plans(sites):
    made = {}

    def get(layout):
        if layout not in made:
            env, B = LAYOUTS[layout]
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made[layout] = vrt.FormalPlan(sites, vrt.quadrature_directions(TH, PH), 3, dirs=DIRS)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            assert made[layout].native_pair_block_f32 == B
        return made[layout]

    yield get
    for p in made.values():
        p.close()


class _Planes:
    """plane sets of `nb` wavelengths: float32 in the layout of `plan`, float64 in the grid's (made by `plan64`)"""

    def __init__(self, plan, plan64, nb):
        import torch
        self.torch, self.plan, self.plan64, self.nb, self.n = torch, plan, plan64, nb, plan.sites.n
        self.dev = torch.device("cuda", 0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.count = plan.native_plane_count(nb)
        assert plan64.native_plane_count(nb) == self.count == 2 * ((nb + 1) // 2) * self.n

    def f32_planes(self, a, down, poison_pad):
        t = self.torch
        out = t.full((self.count,), float("nan"), dtype=t.float32, device=self.dev)
        src = t.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)
        self.plan.to_native_dev(self.nb, self.nb, src.data_ptr(), 0 if down else out.data_ptr(), out.data_ptr() if down else 0,
                                stream=self.st, f32=True)
        if poison_pad and self.nb & 1:                  # the padding wavelength: the last element of the last pair
            npair, B = (self.nb + 1) // 2, self.plan.native_pair_block_f32
            idx = np.array([2 * _pair_index(npair - 1, p, self.n, B, npair) + 1 for p in range(self.n)])
            out[t.from_numpy(idx).to(self.dev)] = float("nan")
        return out

    def f64_up(self, a):
        t = self.torch
        out = t.full((self.count,), float("nan"), dtype=t.float64, device=self.dev)
        src = t.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)
        self.plan64.to_native_dev(self.nb, self.nb, src.data_ptr(), out.data_ptr(), 0, stream=self.st)
        return out


class _Rates:
    """a rates case on the device and the calls of the three new entries on it"""

    def __init__(self, sites, case3):
        import torch
        self.torch, self.sites, self.n = torch, sites, sites.n
        self.c, self.r, self.C0 = case3
        self.nlam = self.r["lam"].size
        self.dev = torch.device("cuda", 0)
        self.st = torch.cuda.current_stream().cuda_stream
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        c, r = self.c, self.r
        self.d_dop, self.d_gam, self.d_T, self.d_lte = t(c["doppler"]), t(c["gamma"]), t(c["T"]), t(r["lte"])
        self.d_C, self.d_atom = t(r["C"]), t(r["atom"])

    def _mid(self):
        c, r = self.c, self.r
        return (r["planck2"], c["lambda0"], self.C0, self.d_dop.data_ptr(), self.d_gam.data_ptr(), r["sigma_bb_const"], r["sig1"],
                r["sig2"], self.d_T.data_ptr(), self.d_lte.data_ptr(), r["hc_over_kB"], r["pref_ij"], r["pref_ji"])

    def shares(self, owner, l0, l1, up, down, f32_planes):
        torch = self.torch
        out = torch.full((6, self.n), float("nan"), dtype=torch.float64, device=self.dev)
        entry = api.rate_shares_native_dev_f32 if f32_planes else api.rate_shares_native_dev
        ptr = lambda x: 0 if x is None else x.data_ptr()
        entry(owner, self.r["lam"], self.c["blocks"], l0, l1, ptr(up), ptr(down), *self._mid(), out.data_ptr(), stream=self.st)
        torch.cuda.synchronize()
        return out

    def populations(self, shares):
        torch = self.torch
        R = torch.full((self.n, 3, 3), float("nan"), dtype=torch.float64, device=self.dev)
        pops = torch.full((3, self.n), float("nan"), dtype=torch.float64, device=self.dev)
        api.populations_from_shares_dev(self.n, shares.data_ptr(), self.d_C.data_ptr(), self.d_atom.data_ptr(), R.data_ptr(),
                                        pops.data_ptr(), stream=self.st)
        torch.cuda.synchronize()
        return R.cpu().numpy(), pops.cpu().numpy()

    def whole_f32(self, plan, up, down):
        torch = self.torch
        R = torch.full((self.n, 3, 3), float("nan"), dtype=torch.float64, device=self.dev)
        pops = torch.full((3, self.n), float("nan"), dtype=torch.float64, device=self.dev)
        api.rates_populations_native_dev_f32(plan, self.r["lam"], self.c["blocks"], up.data_ptr(), down.data_ptr(), *self._mid(),
                                             self.d_C.data_ptr(), self.d_atom.data_ptr(), R.data_ptr(), pops.data_ptr(),
                                             stream=self.st)
        torch.cuda.synchronize()
        return R.cpu().numpy(), pops.cpu().numpy()


# ---- 1. the float shares kernel is the double shares kernel on the widened J, bit for bit -----------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("nbb, nbf", CASES)
def test_float_shares_kernel_is_the_double_kernel_on_the_widened_J(sites, plans, layout, nbb, nbf):
    plan, plan64 = plans(layout), plans("default")
    rc = _Rates(sites, rates_case(sites.n, 7, nbb, nbf))
    Ju, Jd = rc.r["J_up"], rc.r["J_down"]
    for name, (l0, l1) in ranges(nbb, nbf).items():
        nb = l1 - l0
        if nb == 0:                                     # no wavelength, no J: six zero planes from either entry
            for owner, is_f32 in ((plan, True), (sites, False)):
                got = rc.shares(owner, l0, l1, None, None, is_f32).cpu().numpy()
                assert (got == 0.0).all() and not np.signbit(got).any(), (layout, name)
            continue
        P = _Planes(plan, plan64, nb)
        out = {}
        for which, (a, b) in {"both": (Ju, Jd), "up": (Ju, None), "down": (None, Jd)}.items():
            cut = lambda x: None if x is None else x[:, l0:l1]
            J = widened_J(cut(a), cut(b))
            ref = rc.shares(sites, l0, l1, P.f64_up(J), None, False).cpu().numpy()
            for poison in ((False, True) if nb & 1 else (False,)):
                up = None if a is None else P.f32_planes(cut(a), False, poison)
                down = None if b is None else P.f32_planes(cut(b), True, poison)
                got = rc.shares(plan, l0, l1, up, down, True).cpu().numpy()
                assert np.isfinite(got).all(), (layout, name, which, poison)
                assert np.array_equal(got, ref), (layout, name, which, poison)
            out[which] = ref
        assert not np.array_equal(out["both"], out["up"]) and not np.array_equal(out["both"], out["down"])
        # a transition without a wavelength in the range gets exactly 0, one with a wavelength something positive
        for tr, b in ((0, 2), (1, 4), (2, 0)):
            lo, hi = rc.c["blocks"][b], rc.c["blocks"][b + 1]
            rows = out["both"][2 * tr: 2 * tr + 2]
            assert ((rows > 0).all() if max(lo, l0) < min(hi, l1) else (rows == 0.0).all()), (layout, name, tr)


# ---- 2. the shares of a partition against the one-device rates and the oracle ----------------------------------------------
# The atmospheres: _lambda_case (33 wavelengths) and small_lambda_case (6) in LTE, where the oracle's own populations move by
# less than 1e-13 under a rounding of its R (tests/test_multi_f32_host.py); the random rates of test 1 leave 1e-37 of the
# atoms in level 2 and the oracle's populations move by 1.4e-12 there -- no populations can be held to 1e-12 on them.
def _partition_case(voro_small, name):
    from test_physics import _lambda_case
    pos, _, bounds = voro_small
    return rates_case_of(_lambda_case(pos, bounds, 11) if name == "lambda33" else small_lambda_case(pos, bounds, 11), 5)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", ["lambda33", "small6"])
def test_shares_of_a_partition_add_up_to_the_one_device_rates(voro_small, sites, plans, layout, name):
    """For the partitions of [0, nlam) into 1, 2, 3 and nlam ranges: the shares added in range order and passed through
    vrt_populations_from_shares_dev give R within 1e-12, relative per transition, of vrt_rates_populations_native_dev_f32
    on the whole-range planes of the same J and of oracle.calculate_R on that J; the populations within 1e-12 of that
    kernel's and of oracle.revised_populations of the oracle's R."""
    plan, plan64 = plans(layout), plans("default")
    rc = _Rates(sites, _partition_case(voro_small, name))
    Ju, Jd = rc.r["J_up"], rc.r["J_down"]
    whole = _Planes(plan, plan64, rc.nlam)
    R_dev, p_dev = rc.whole_f32(plan, whole.f32_planes(Ju, False, False), whole.f32_planes(Jd, True, False))
    R_orc = oracle_R(rc.c, rc.r, rc.C0, widened_J(Ju, Jd))
    p_orc = orc.revised_populations(R_orc, rc.r["C"], rc.r["atom"])
    for parts in partitions(rc.nlam):
        total = None
        for l0, l1 in parts:
            P = _Planes(plan, plan64, l1 - l0)
            s = rc.shares(plan, l0, l1, P.f32_planes(Ju[:, l0:l1], False, True), P.f32_planes(Jd[:, l0:l1], True, True), True)
            total = s if total is None else total + s
        R, pops = rc.populations(total)
        assert np.array_equal(pops, orc.revised_populations(R, rc.r["C"], rc.r["atom"]))        # (the 2 x 2 solve alone)
        figs = (max(rel_per_transition(R, R_dev)), max(rel_per_transition(R, R_orc)),
                float(np.abs(pops / p_dev - 1).max()), float(np.abs(pops / p_orc - 1).max()))
        print(f"{layout}, {rc.nlam} wavelengths in {len(parts)} ranges: R against the one-device kernel {figs[0]:.2e}, against "
              f"the oracle {figs[1]:.2e}; populations {figs[2]:.2e}, {figs[3]:.2e}")
        assert max(figs) <= REGROUPING, (layout, len(parts), figs)


# ---- the sessions, stepped by hand -------------------------------------------------------------------------------------------
class _Single:
    """the one-device session (tests/test_f32_lambda.py: _Session)"""

    def __init__(self, plan, case, f32_storage=True):
        self.L = _lib.load()
        lc, self.keep = case.c_struct()
        self.n, self.nlam = plan.sites.n, int(self.keep["lam"].size)
        self.h = ctypes.c_void_p()
        create = self.L.vrt_lambda_create_f32 if f32_storage else self.L.vrt_lambda_create
        self.rc = create(plan._h, ctypes.byref(lc), api._d(api._f64(W)), ctypes.byref(self.h))
        self.prefix = "vrt_lambda"

    def iterate(self):
        d = ctypes.c_double()
        _lib.check(getattr(self.L, self.prefix + "_iterate")(self.h, ctypes.byref(d)))
        return d.value

    def get(self):
        J, S, pops = np.zeros((self.n, self.nlam)), np.zeros((self.n, self.nlam)), np.zeros((3, self.n))
        _lib.check(getattr(self.L, self.prefix + "_get")(self.h, api._d(J), api._d(S), api._d(pops), None, None))
        return J, S, pops

    def set_state(self, S, pops):
        return getattr(self.L, self.prefix + "_set_state")(self.h, None if S is None else api._d(api._f64(S)),
                                                          None if pops is None else api._d(api._f64(pops)))

    def storage(self):
        return getattr(self.L, self.prefix + "_storage")(self.h)

    def run(self, iterates):
        states, hist = [], []
        for _ in range(iterates):
            hist.append(self.iterate())
            states.append(self.get())
        for st in states:
            for a in st:
                a.setflags(write=False)
        return states, hist

    def close(self):
        if self.h:
            getattr(self.L, self.prefix + "_destroy")(self.h)
            self.h = None


class _Multi(_Single):
    """vrt_multi_lambda_* on a MultiDevicePlan"""

    def __init__(self, mp, case, f32_storage=True):
        self.L = _lib.load()
        lc, self.keep = case.c_struct()
        self.n, self.nlam = mp.n, int(self.keep["lam"].size)
        self.h = ctypes.c_void_p()
        create = self.L.vrt_multi_lambda_create_f32 if f32_storage else self.L.vrt_multi_lambda_create
        self.rc = create(mp._h, ctypes.byref(lc), api._d(api._f64(W)), ctypes.byref(self.h))
        self.prefix = "vrt_multi_lambda"


def _multi_plan(voro_small, world):
    pos, nbr, bounds = voro_small
    return vrt.MultiDevicePlan(pos, nbr, bounds, vrt.quadrature_directions(TH, PH), dirs=DIRS, devices=(0,) * world)


@pytest.fixture(scope="module")
def runs(voro_small):
    return oracle_runs(*voro_small, ORACLE_ITERATES)


@pytest.fixture(scope="module")
def single(plans, runs):
    """four iterates of the one-device float session: the state after each, and the history; computed once"""
    s = _Single(plans("default"), runs["case"])
    assert s.rc == 0
    out = s.run(4)
    s.close()
    return out


@pytest.fixture(scope="module")
def multi(voro_small, runs):
    """the same of the float multi session over 1, 2, 3 and 4 members of device 0, made on demand and kept"""
    made = {}

    def get(world):
        if world not in made:
            mp = _multi_plan(voro_small, world)
            s = _Multi(mp, runs["case"])
            assert s.rc == 0 and s.storage() == 4
            made[world] = s.run(4)
            s.close()
            mp.close()
        return made[world]

    return get


# ---- 3. the session against the one-device float session ---------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_session_is_the_one_device_float_session_block_by_block(runs, single, multi, world):
    """33 wavelengths in blocks of 33; 17, 16; 11, 11, 11; 9, 8, 8, 8.  First iterate: J, S and the criterion bit for bit
    (every wavelength is solved by one member from LTE populations, and a solve does not see the other wavelengths of
    its block).  Iterates 2-4: the populations of the members differ from the one-device session's by the regrouping of
    the rate integrals, so J and S are held to the conditions of oracle/f32_model.py and the populations to 4 x the
    largest deviation between the model loop and its perturbed copy."""
    case = runs["case"]
    assert [b - a for a, b in partition(33, world)] == {1: [33], 2: [17, 16], 3: [11, 11, 11], 4: [9, 8, 8, 8]}[world]
    states, hist = multi(world)
    ref, ref_hist = single
    B0, eps = f32(case.B0), np.asarray(case.eps)[:, None]
    for J, S, pops in states:
        assert np.array_equal(f32(J), J) and np.array_equal(f32(S), S)
        assert np.array_equal(S, f32((1.0 - eps) * J + eps * B0))
        assert np.isfinite(J).all() and (pops > 0).all()
    assert np.array_equal(states[0][0], ref[0][0]) and np.array_equal(states[0][1], ref[0][1]) and hist[0] == ref_hist[0]
    pert = max(deviations(a, b)[2] for a, b in zip(runs["perturbed"], runs["model"]))
    print(f"bound: populations against the one-device float session 4 x {pert:.2e}")
    for k in range(4):
        figs = [within_conditions(states[k][q], ref[k][q]) for q in range(2)]
        dp = float(np.abs(states[k][2] / ref[k][2] - 1).max())
        print(f"{world} members, iterate {k + 1}: J differs in {figs[0][1]} of {figs[0][2]} ({figs[0][3]:g} ulp), S in {figs[1][1]} "
              f"({figs[1][3]:g} ulp), populations {dp:.2e}, criterion {hist[k]:.17g} against {ref_hist[k]:.17g}")
        assert figs[0][0] and figs[1][0], (world, k, figs)
        assert dp <= 4 * pert, (world, k, dp, pert)


def test_double_session_reports_eight_bytes(voro_small, runs):
    L = _lib.load()
    mp = _multi_plan(voro_small, 2)
    s = _Multi(mp, runs["case"], f32_storage=False)
    assert s.rc == 0 and s.storage() == 8 and L.vrt_multi_lambda_storage(None) == _lib.VRT_EINVAL
    s.close()
    mp.close()


# ---- 4. members with one wavelength and with none ----------------------------------------------------------------------------
def test_members_with_one_wavelength_and_with_none(voro_small, plans):
    """six wavelengths over seven members: six hold a single pair with its padding, one holds nothing"""
    pos, nbr, bounds = voro_small
    case = small_lambda_case(pos, bounds, 11)
    assert [b - a for a, b in partition(6, 7)] == [1, 1, 1, 1, 1, 1, 0]
    one = _Single(plans("default"), case)
    assert one.rc == 0
    d1 = one.iterate()
    J1, S1, _ = one.get()
    one.close()
    mp = _multi_plan(voro_small, 7)
    s = _Multi(mp, case)
    assert s.rc == 0
    states, hist = s.run(4)
    s.close()
    mp.close()
    assert hist[0] == d1 and np.array_equal(states[0][0], J1) and np.array_equal(states[0][1], S1)
    for J, S, pops in states:
        assert np.isfinite(J).all() and np.isfinite(S).all() and np.isfinite(pops).all() and (pops > 0).all()
    assert all(np.isfinite(h) for h in hist)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_eight_members_with_one_wavelength_each_and_one_without(voro_small, plans, runs, storage):
    """Seven wavelengths (tests/test_resume_host.py's small_lambda_case with nbb = 3, nbf = 2) over eight members of
    device 0: blocks 1, 1, 1, 1, 1, 1, 1, 0, in double storage in sweep order and in float storage.  Three iterates against
    the one-device session of the same storage, as test_session_is_the_one_device_float_session_block_by_block compares
    them: iterate 1 bit for bit; later iterates by the conditions of oracle/f32_model.py and 4 x the model's perturbation
    (float storage), or by the 1e-12 of the regrouped rate sums (double storage: REGROUPING, the bound of
    tests/test_physics.py's multi-device session against the one-device one).  Then the one-device state after iterate 3
    through set_state and one more iterate: the same S and populations go in, and every wavelength is solved by one
    member, so J, S and the criterion are the one-device session's fourth bit for bit; the populations behind them differ
    by the regrouping again."""
    from test_resume_host import small_lambda_case as lambda_case_of
    pos, nbr, bounds = voro_small
    f32s = storage == "f32"
    assert os.environ.get("VRT_LAMBDA_NATIVE", "1") == "1"           # (double storage: sweep-order planes)
    case = lambda_case_of(pos, bounds, 11, 3, 2)
    assert [b - a for a, b in partition(7, 8)] == [1, 1, 1, 1, 1, 1, 1, 0]
    one = _Single(plans("default"), case, f32_storage=f32s)
    assert one.rc == 0 and one.storage() == (4 if f32s else 8)
    ref, ref_hist = one.run(4)
    one.close()
    pert = max(deviations(a, b)[2] for a, b in zip(runs["perturbed"], runs["model"]))
    B0, eps = f32(case.B0), np.asarray(case.eps)[:, None]

    def compare(k, got, d):
        J, S, pops = got
        assert np.isfinite(J).all() and np.isfinite(S).all() and (pops > 0).all()
        dp = float(np.abs(pops / ref[k][2] - 1).max())
        if f32s:
            assert np.array_equal(f32(J), J) and np.array_equal(f32(S), S)
            assert np.array_equal(S, f32((1.0 - eps) * J + eps * B0))
            figs = [within_conditions(got[q], ref[k][q]) for q in range(2)]
            print(f"float storage, iterate {k + 1}: J differs in {figs[0][1]} of {figs[0][2]} ({figs[0][3]:g} ulp), S in "
                  f"{figs[1][1]} ({figs[1][3]:g} ulp), populations {dp:.2e} (bound 4 x {pert:.2e}), criterion {d:.17g} "
                  f"against {ref_hist[k]:.17g}")
            assert figs[0][0] and figs[1][0], (k, figs)
            assert dp <= 4 * pert, (k, dp, pert)
        else:
            dJ = float(np.abs(J - ref[k][0]).max() / np.abs(ref[k][0]).max())     # (J is 0 at the never-solved site)
            dS = float(np.abs(S / ref[k][1] - 1).max())
            print(f"double storage, iterate {k + 1}: J {dJ:.2e}, S {dS:.2e}, populations {dp:.2e}, criterion {d:.17g} against "
                  f"{ref_hist[k]:.17g}")
            assert max(dJ, dS, dp) <= REGROUPING, (k, dJ, dS, dp)

    mp = _multi_plan(voro_small, 8)
    s = _Multi(mp, case, f32_storage=f32s)
    try:
        assert s.rc == 0 and s.storage() == (4 if f32s else 8)
        states, hist = s.run(3)
        assert np.array_equal(states[0][0], ref[0][0]) and np.array_equal(states[0][1], ref[0][1]) and hist[0] == ref_hist[0]
        for k in range(3):
            compare(k, states[k], hist[k])
        assert s.set_state(ref[2][1], ref[2][2]) == 0
        d4 = s.iterate()
        got4 = s.get()
        assert d4 == ref_hist[3] and np.array_equal(got4[0], ref[3][0]) and np.array_equal(got4[1], ref[3][1])
        compare(3, got4, d4)
    finally:
        s.close()
        mp.close()


# ---- 5. state and refusals ---------------------------------------------------------------------------------------------------
def test_state_and_refusals(voro_small, runs, multi, monkeypatch):
    case = runs["case"]
    states, hist = multi(2)
    L = _lib.load()
    mp = _multi_plan(voro_small, 2)
    s = _Multi(mp, case)
    assert s.rc == 0
    # _get -> _set_state -> _iterate continues an uninterrupted session bit for bit
    J2, S2, p2 = states[1]
    assert s.set_state(S2, p2) == 0
    assert s.iterate() == hist[2] and all(np.array_equal(a, b) for a, b in zip(s.get(), states[2]))
    # an S that is no float is accepted and is the state of its float rounding
    rng = np.random.default_rng(3)
    S_odd = S2 * (1 + 1e-9 * rng.random(S2.shape))
    assert not np.array_equal(f32(S_odd), S_odd)
    assert s.set_state(S_odd, p2) == 0
    d_odd, after_odd = s.iterate(), s.get()
    assert s.set_state(f32(S_odd), p2) == 0
    assert s.iterate() == d_odd and all(np.array_equal(a, b) for a, b in zip(s.get(), after_odd))
    # a refused state (a zero in S) leaves the session as it was
    assert s.set_state(S2, p2) == 0
    bad = S2.copy()
    bad[5, 20] = 0.0
    assert s.set_state(bad, p2) == _lib.VRT_EINVAL
    assert s.iterate() == hist[2] and all(np.array_equal(a, b) for a, b in zip(s.get(), states[2]))
    # ... and so does a refused acceleration
    assert s.set_state(S2, p2) == 0
    assert L.vrt_multi_lambda_set_acceleration(s.h, 2, 4, 4) == _lib.VRT_EINVAL
    assert b"float" in L.vrt_last_error()
    assert s.iterate() == hist[2] and all(np.array_equal(a, b) for a, b in zip(s.get(), states[2]))
    s.close()
    mp.close()
    # no fp64 fallback: plans off the patch path, or with caller-layout sessions, are refused and *out stays NULL
    for var, value in (("VRT_PATH", "steps"), ("VRT_LAMBDA_NATIVE", "0")):
        monkeypatch.setenv(var, value)
        other = _multi_plan(voro_small, 2)
        monkeypatch.delenv(var)
        refused = _Multi(other, case)
        assert refused.rc == _lib.VRT_EINVAL and not refused.h, var
        accepted = _Multi(other, case, f32_storage=False)           # (the double session takes such a plan as before)
        assert accepted.rc == 0 and accepted.storage() == 8
        accepted.close()
        other.close()


# ---- 6. the Python keyword and the RCCL leg ----------------------------------------------------------------------------------
def test_python_keyword_checkpoints_and_the_rccl_leg(voro_small, runs, multi, monkeypatch, tmp_path):
    case = runs["case"]
    states, hist = multi(2)
    mp = _multi_plan(voro_small, 2)
    J, S, pops, h = mp.lambda_iteration(0.0, 4, case, W, storage="f32")
    assert h == hist and all(np.array_equal(a, b) for a, b in zip((J, S, pops), states[3]))
    ck = str(tmp_path / "run.npz")
    mp.lambda_iteration(0.0, 2, case, W, storage="f32", checkpoint=ck)
    Jr, Sr, pr, hr = mp.lambda_iteration(0.0, 2, case, W, storage="f32", resume=ck)
    assert hr == hist and all(np.array_equal(a, b) for a, b in zip((Jr, Sr, pr), states[3]))
    assert mp.lambda_iteration(1.0, 10, case, W, storage="f32")[3] == []      # the criterion starts at 1: no iterate
    with pytest.raises(ValueError):
        mp.lambda_iteration(0.0, 4, case, W, storage="f32", ng=(4, 4))
    with pytest.raises(ValueError):
        mp.lambda_iteration(0.0, 4, case, W, storage="single")
    mp.close()
    # the all-reduce of the shares on a one-rank communicator, behind float sweeps: a one-rank sum is the identity
    out = {}
    for force in ("0", "1"):
        monkeypatch.setenv("VRT_MULTI_FORCE_RCCL", force)
        one = _multi_plan(voro_small, 1)
        assert one.uses_rccl == (force == "1")
        it = one.lambda_iteration(0.0, 3, case, W, storage="f32")
        out[force] = tuple(it[:3]) + (np.array(it[3]),)
        one.close()
    monkeypatch.delenv("VRT_MULTI_FORCE_RCCL")
    for a, b in zip(out["0"], out["1"]):
        assert np.array_equal(a, b)
    assert all(np.array_equal(a, b) for a, b in zip(out["0"][:3], multi(1)[0][2]))
