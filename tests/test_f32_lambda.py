"""GPU tests (-m gpu) of the float-storage line Λ-iteration: the two device entry points on float sweep-order plane sets
(vrt_lambda_update_native_dev_f32 against a numpy model, vrt_rates_populations_native_dev_f32 against the fp64 kernel,
both bit for bit, in every float plane layout), the session vrt_lambda_create_f32 against the public entries (bit for
bit) and against the CPU model loop of tests/f32_lambda_model.py (the conditions of oracle/f32_model.py for the first
iterate, distances only after four), its state entries and its refusals.  Every bound is a figure of the oracle alone
(tests/test_f32_lambda_host.py prints them)."""
import ctypes
import os

import numpy as np
import pytest

import voronoirt_amd as vrt
from f32_lambda_model import deviations, f32, oracle_runs, update_model
from oracle.f32_model import float_compare, within_conditions
from oracle.layout_ref import pair_index as _pair_index
from voronoirt_amd import _lib, api

pytestmark = pytest.mark.gpu

W, TH, PH, NQ = vrt.read_quadrature("ul7n12.dat")
DIRS = [1 if t > 90 else -1 for t in TH]
QUAD = "ul7n12.dat"
ORACLE_ITERATES = 6             # as tests/test_f32_lambda_host.py: the bounds are the largest figures of its six iterates
# plans of the three float plane layouts: pairs per block 2 (default: a site's four wavelengths are one 16-byte access),
# 1 (VRT_PATCH_QUAD=0) and 8 (VRT_PAIR_BLOCK=8); the options are read when the plan is created
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
    """float32 torch plane sets of one plan and wavelength count, filled from and read back to caller-layout arrays"""

    def __init__(self, plan, nlam):
        import torch
        self.torch, self.plan, self.nlam, self.n = torch, plan, nlam, plan.sites.n
        self.dev = torch.device("cuda", 0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.count = plan.native_plane_count(nlam)

    def dev_f32(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)

    def up(self, a):
        out = self.torch.full((self.count,), float("nan"), dtype=self.torch.float32, device=self.dev)
        self.plan.to_native_dev(self.nlam, self.nlam, self.dev_f32(a).data_ptr(), out.data_ptr(), 0, stream=self.st, f32=True)
        return out

    def down(self, a):
        out = self.torch.full((self.count,), float("nan"), dtype=self.torch.float32, device=self.dev)
        self.plan.to_native_dev(self.nlam, self.nlam, self.dev_f32(a).data_ptr(), 0, out.data_ptr(), stream=self.st, f32=True)
        return out

    def back(self, d, planes):
        out = self.torch.full((self.n, self.nlam), float("nan"), dtype=self.torch.float32, device=self.dev)
        self.plan.from_native_dev(d, self.nlam, self.nlam, planes.data_ptr(), out.data_ptr(), stream=self.st, f32=True)
        self.torch.cuda.synchronize()
        return out.cpu().numpy()

    def pad_indices(self):
        """raw float indices of the pad wavelength of an odd nlam: the last element of the last pair, every position"""
        npair, B = (self.nlam + 1) // 2, self.plan.native_pair_block_f32
        return np.array([2 * _pair_index(npair - 1, p, self.n, B, npair) + 1 for p in range(self.n)])


# ---- 1. the update kernel against the numpy model, bit for bit ---------------------------------------------------------
# nλ 2: one pair; 4: one quad; 6: quad + pair; 7: two quads with a pad; 33: 16 pairs + one pair with a pad
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("nlam", [2, 4, 6, 7, 33])
def test_update_kernel_is_its_numpy_model(plans, layout, nlam):
    import torch
    plan = plans(layout)
    P = _Planes(plan, nlam)
    n = P.n
    rng = np.random.default_rng(100 * nlam + len(layout))
    # J_up, J_down in (0.5, 1), B and S_old in (1, 2): S_new in (1, 2) and every |1 - S_old / S_new| < 1
    Ju, Jd = (0.5 + 0.5 * rng.random((n, nlam))).astype(np.float32), (0.5 + 0.5 * rng.random((n, nlam))).astype(np.float32)
    B, So = (1 + rng.random((n, nlam))).astype(np.float32), (1 + rng.random((n, nlam))).astype(np.float32)
    eps = rng.random(n)
    eps[0], eps[1] = 0.0, 1.0
    d_eps = torch.from_numpy(eps).to(P.dev)
    pad = torch.from_numpy(P.pad_indices()).to(P.dev) if nlam & 1 else None

    def run(Ju_, Jd_, So_, poison_pad=False):
        pJu, pJd = (None if Ju_ is None else P.up(Ju_)), (None if Jd_ is None else P.down(Jd_))
        pB, pSu = P.up(B), P.up(So_)
        pSd = torch.full((P.count,), float("nan"), dtype=torch.float32, device=P.dev)
        if poison_pad:                                  # the pad takes no part: whatever it holds, it is written as 0
            for t in (pJu, pJd, pB, pSu):
                t[pad] = float("nan")
        d = api.lambda_update_native_dev_f32(plan, nlam, 0 if pJu is None else pJu.data_ptr(), 0 if pJd is None else pJd.data_ptr(),
                                             pB.data_ptr(), d_eps.data_ptr(), pSu.data_ptr(), pSd.data_ptr(), stream=P.st)
        raw = (pSu.cpu().numpy(), pSd.cpu().numpy())
        return P.back(1, pSu), P.back(-1, pSd), d, raw

    Su, Sd, d, raw = run(Ju, Jd, So, poison_pad=pad is not None)
    _, Sm, dm = update_model(Ju, Jd, B, So, eps)
    assert np.array_equal(Su, Sm) and np.array_equal(Sd, Sm), (layout, nlam)
    assert np.array_equal(np.sort(raw[0]), np.sort(raw[1]))             # the two orders: permutations of each other
    assert d == dm and 0 < d < 1, (layout, nlam, d, dm)
    if pad is not None:
        idx = P.pad_indices()
        assert not raw[0][idx].any() and not raw[1][idx].any()
    # one direction without angles
    for a, b in ((Ju, None), (None, Jd)):
        Su, Sd, d, _ = run(a, b, So)
        _, Sm, dm = update_model(a, b, B, So, eps)
        assert np.array_equal(Su, Sm) and np.array_equal(Sd, Sm) and d == dm
    # a NaN in J makes the scalar NaN (and that S); an S_old of 0 gives exactly 1
    Jn = Ju.copy()
    Jn[n // 2, nlam - 1] = np.nan
    Su, Sd, d, _ = run(Jn, Jd, So)
    assert np.isnan(d) and np.isnan(Su[n // 2, nlam - 1]) and np.isnan(Su).sum() == 1
    S0 = So.copy()
    S0[n - 1, 0] = 0.0
    Su, Sd, d, _ = run(Ju, Jd, S0)
    assert d == 1.0 and np.array_equal(Su, update_model(Ju, Jd, B, S0, eps)[1])


def test_update_entry_checks_its_arguments_before_it_launches(plans):
    """VRT_EINVAL, nothing launched: no plan, no J at all, and plane sets that are not 16-byte aligned where the layout
    makes 16-byte accesses."""
    import torch
    L, plan, out = _lib.load(), plans("default"), ctypes.c_double()
    P = _Planes(plan, 4)
    z = torch.zeros(P.count + 2, dtype=torch.float32, device=P.dev)
    eps = torch.zeros(P.n, dtype=torch.float64, device=P.dev)
    ok, odd = z.data_ptr(), z.data_ptr() + 8
    assert L.vrt_lambda_update_native_dev_f32(None, 4, ok, ok, ok, eps.data_ptr(), ok, ok, ctypes.byref(out), None) == _lib.VRT_EINVAL
    assert L.vrt_lambda_update_native_dev_f32(plan._h, 4, None, None, ok, eps.data_ptr(), ok, ok, ctypes.byref(out), None) == _lib.VRT_EINVAL
    assert L.vrt_lambda_update_native_dev_f32(plan._h, 4, odd, None, ok, eps.data_ptr(), ok, ok, ctypes.byref(out), None) == _lib.VRT_EINVAL
    assert b"aligned" in L.vrt_last_error()


# ---- 2. the rates kernel against the fp64 kernel, bit for bit ----------------------------------------------------------
def _rates_case(n, seed, nbb, nbf):
    """_rates_case of tests/test_physics.py for any block sizes (an even nbb: the first nbb line wavelengths)"""
    from test_physics import C0, H_PLANCK, K_B, _line_case
    c = _line_case(n, seed, nbb, nbf)
    rng = c["rng"]
    lam = np.concatenate([c["lam"][:nbb], c["lam"][c["lam"].size - 2 * nbf:]])
    nlam = lam.size
    assert nlam == nbb + 2 * nbf == c["blocks"][5]
    r = dict(lam=lam, J_up=(10 ** rng.uniform(-12, -3, (n, nlam))).astype(np.float32),
             J_down=(10 ** rng.uniform(-12, -3, (n, nlam))).astype(np.float32), planck2=2 * H_PLANCK * C0 ** 2 / lam ** 5,
             lte=np.stack([c["n_i"], c["n_j"] * 3.0, c["n_i"] * 10 ** rng.uniform(-6, 0, n)]),
             sig1=7.9e-22 * (lam[nbb:nbb + nbf] / lam[nbb + nbf - 1]) ** 3, sig2=1.4e-21 * (lam[nbb + nbf:] / lam[-1]) ** 3,
             C=10 ** rng.uniform(-2, 4, (n, 3, 3)), sigma_bb_const=H_PLANCK * C0 / (4 * np.pi * c["lambda0"]) * c["Bij"],
             hc_over_kB=H_PLANCK * C0 / K_B, pref_ij=2 * np.pi / (H_PLANCK * C0) / 1000.0, pref_ji=2 * np.pi / (H_PLANCK * C0))
    for d in range(3):
        r["C"][:, d, d] = 0.0
    r["atom"] = r["lte"].sum(axis=0) * rng.uniform(0.9, 1.1, n)
    return c, r, C0


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("nbb, nbf", [(2, 2), (3, 2), (21, 6)])
def test_rates_kernel_is_the_fp64_kernel_on_the_widened_J(sites, plans, layout, nbb, nbf):
    import torch
    plan = plans(layout)
    n = sites.n
    c, r, C0 = _rates_case(n, 7, nbb, nbf)
    nlam = r["lam"].size
    P = _Planes(plan, nlam)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(P.dev)
    pJu, pJd = P.up(r["J_up"]), P.down(r["J_down"])
    d_dop, d_gam, d_T, d_lte, d_C, d_atom = t(c["doppler"]), t(c["gamma"]), t(c["T"]), t(r["lte"]), t(r["C"]), t(r["atom"])
    out = {}
    for which, (ju, jd) in {"both": (pJu, pJd), "up": (pJu, None), "down": (None, pJd)}.items():
        ptr = lambda x: 0 if x is None else x.data_ptr()
        R32, p32 = (torch.full((n, 3, 3), float("nan"), dtype=torch.float64, device=P.dev),
                    torch.full((3, n), float("nan"), dtype=torch.float64, device=P.dev))
        api.rates_populations_native_dev_f32(plan, r["lam"], c["blocks"], ptr(ju), ptr(jd), r["planck2"], c["lambda0"], C0,
                                             d_dop.data_ptr(), d_gam.data_ptr(), r["sigma_bb_const"], r["sig1"], r["sig2"],
                                             d_T.data_ptr(), d_lte.data_ptr(), r["hc_over_kB"], r["pref_ij"], r["pref_ji"],
                                             d_C.data_ptr(), d_atom.data_ptr(), R32.data_ptr(), p32.data_ptr(), stream=P.st)
        J = torch.full((n, nlam), float("nan"), dtype=torch.float32, device=P.dev)
        plan.J_from_native_dev(nlam, nlam, ptr(ju), ptr(jd), J.data_ptr(), stream=P.st, f32=True)
        J64 = J.double()
        R64, p64 = torch.full_like(R32, float("nan")), torch.full_like(p32, float("nan"))
        api.rates_populations_dev(sites, r["lam"], c["blocks"], nlam, J64.data_ptr(), r["planck2"], c["lambda0"], C0,
                                  d_dop.data_ptr(), d_gam.data_ptr(), r["sigma_bb_const"], r["sig1"], r["sig2"],
                                  d_T.data_ptr(), d_lte.data_ptr(), r["hc_over_kB"], r["pref_ij"], r["pref_ji"],
                                  d_C.data_ptr(), d_atom.data_ptr(), R64.data_ptr(), p64.data_ptr(), stream=P.st)
        torch.cuda.synchronize()
        out[which] = R32.cpu().numpy()
        assert np.isfinite(out[which]).all() and np.isfinite(p32.cpu().numpy()).all()
        assert np.array_equal(out[which], R64.cpu().numpy()), (layout, nlam, which)
        assert np.array_equal(p32.cpu().numpy(), p64.cpu().numpy()), (layout, nlam, which)
    assert not np.array_equal(out["both"], out["up"]) and not np.array_equal(out["both"], out["down"])


# ---- the session, stepped by hand ------------------------------------------------------------------------------------------
class _Session:
    def __init__(self, plan, case, f32_storage=True):
        self.L = _lib.load()
        lc, self.keep = case.c_struct()
        self.n, self.nlam = plan.sites.n, int(self.keep["lam"].size)
        self.h = ctypes.c_void_p()
        create = self.L.vrt_lambda_create_f32 if f32_storage else self.L.vrt_lambda_create
        self.rc = create(plan._h, ctypes.byref(lc), api._d(api._f64(W)), ctypes.byref(self.h))

    def iterate(self):
        d = ctypes.c_double()
        _lib.check(self.L.vrt_lambda_iterate(self.h, ctypes.byref(d)))
        return d.value

    def get(self):
        J, S, pops = np.zeros((self.n, self.nlam)), np.zeros((self.n, self.nlam)), np.zeros((3, self.n))
        _lib.check(self.L.vrt_lambda_get(self.h, api._d(J), api._d(S), api._d(pops), None, None))
        return J, S, pops

    def set_state(self, S, pops):
        return self.L.vrt_lambda_set_state(self.h, None if S is None else api._d(api._f64(S)),
                                           None if pops is None else api._d(api._f64(pops)))

    def close(self):
        if self.h:
            self.L.vrt_lambda_destroy(self.h)
            self.h = None


@pytest.fixture(scope="module")
def runs(voro_small):
    return oracle_runs(*voro_small, ORACLE_ITERATES)


@pytest.fixture(scope="module")
def stepped(sites, plans, runs):
    """four iterates of a float-storage session: the state after each, and the history; computed once"""
    s = _Session(plans("default"), runs["case"])
    assert s.rc == 0
    states, hist = [], []
    for _ in range(4):
        hist.append(s.iterate())
        states.append(s.get())
    s.close()
    for st in states:
        for a in st:
            a.setflags(write=False)
    return states, hist


# ---- 3. the session equals the public entries, bit for bit --------------------------------------------------------------
def test_session_is_the_loop_over_the_public_entries(sites, runs, stepped):
    case = runs["case"]
    Jh, Sh, ph_, hh = vrt.Lambda_voronoi_host(0.0, 4, sites, case, QUAD, storage="f32")
    Jn, Sn, pn, hn = vrt.Lambda_voronoi(0.0, 4, sites, case, QUAD, native=True, storage="f32")
    assert len(hh) == 4 and hh == hn
    assert np.array_equal(Jh, Jn) and np.array_equal(Sh, Sn) and np.array_equal(ph_, pn)
    states, hist = stepped
    assert hist == hh and all(np.array_equal(a, b) for a, b in zip(states[3], (Jh, Sh, ph_)))
    B0, eps = f32(case.B0), np.asarray(case.eps)[:, None]
    for J, S, pops in states:                                   # every iterate, from the downloaded arrays alone
        assert np.array_equal(f32(J), J) and np.array_equal(f32(S), S)
        assert np.array_equal(S, f32((1.0 - eps) * J + eps * B0))
        assert (pops > 0).all()
    # the stop rule: criterion(S_new = B, S_old = 0) = 1, so a tolerance of 1 or more gives no iterate; one just above
    # hist[k] stops after k + 1
    assert vrt.Lambda_voronoi_host(1.0, 10, sites, case, QUAD, storage="f32")[3] == []
    assert vrt.Lambda_voronoi(1.0, 10, sites, case, QUAD, native=True, storage="f32")[3] == []
    k = next(i for i, h in enumerate(hist) if h < 1.0)
    tol = hist[k] * 1.0001
    expect = next(i for i, h in enumerate(hist) if h <= tol) + 1
    assert vrt.Lambda_voronoi_host(tol, 10, sites, case, QUAD, storage="f32")[3] == hist[:expect]
    assert vrt.Lambda_voronoi(tol, 10, sites, case, QUAD, native=True, storage="f32")[3] == hist[:expect]
    with pytest.raises(ValueError):
        vrt.Lambda_voronoi_host(0.0, 4, sites, case, QUAD, storage="f32", ng=(4, 4))
    with pytest.raises(ValueError):
        vrt.Lambda_voronoi(0.0, 4, sites, case, QUAD, storage="f32")


# ---- 4. the first iterate against the CPU model loop ----------------------------------------------------------------------
def test_first_iterate_is_the_model_loop(runs, stepped):
    """J and S: at least 99.9 % of the elements bit-identical, the rest within 2 float ulps (the model loop against its
    perturbed copy: 29 and 22 of 49 500, 1 ulp -- inside the cap of 49)."""
    for name, q in (("J", 0), ("S", 1)):
        ok, ndiff, size, ulps = within_conditions(stepped[0][0][q], runs["model"][0][q])
        print(f"first iterate {name}: differs from the model loop in {ndiff} of {size}, largest distance {ulps:g} ulp")
        assert ok, (name, ndiff, size, ulps)
    assert abs(stepped[1][0] / runs["hist"][0] - 1) < 1e-6


# ---- 5. four iterates against the CPU model loop, by distance only ---------------------------------------------------------
def test_four_iterates_stay_beside_the_model_loop_and_the_fp64_session(sites, plans, runs, stepped):
    """J and S within 4 float ulps of the model loop at every iterate (its perturbed copy reaches 2); the populations
    within 4x the largest deviation of the perturbed copy; against the fp64 SESSION, J, S and the populations within 4x
    the largest deviations between the two oracle loops.  Every bound is computed from the oracle runs here."""
    states, _ = stepped
    pert = max(deviations(a, b)[2] for a, b in zip(runs["perturbed"], runs["model"]))
    between = [max(deviations(a, b)[q] for a, b in zip(runs["model"], runs["f64"])) for q in range(3)]
    print(f"bounds: populations against the model loop 4 x {pert:.2e}; against the fp64 session 4 x "
          f"(J {between[0]:.2e}, S {between[1]:.2e}, populations {between[2]:.2e})")
    s64 = _Session(plans("default"), runs["case"], f32_storage=False)
    assert s64.rc == 0
    try:
        for k in range(4):
            s64.iterate()
            figs = [float_compare(states[k][q], runs["model"][k][q]) for q in range(2)]
            dp = deviations(states[k], runs["model"][k])[2]
            d64 = deviations(states[k], s64.get())
            print(f"iterate {k + 1}: against the model loop J differs in {figs[0][0]} ({figs[0][1]:g} ulp), S in {figs[1][0]} "
                  f"({figs[1][1]:g} ulp), populations {dp:.2e}; against the fp64 session J {d64[0]:.2e}, S {d64[1]:.2e}, "
                  f"populations {d64[2]:.2e}")
            assert figs[0][1] <= 4 and figs[1][1] <= 4, (k, figs)
            assert dp <= 4 * pert, (k, dp, pert)
            for q in range(3):
                assert d64[q] <= 4 * between[q], (k, q, d64, between)
    finally:
        s64.close()


# ---- 6. state and refusals ------------------------------------------------------------------------------------------------
def test_state_and_refusals(sites, plans, runs, stepped, voro_small, monkeypatch, tmp_path):
    case, plan = runs["case"], plans("default")
    states, hist = stepped
    L = _lib.load()
    # _get -> _set_state -> iterate continues an uninterrupted session bit for bit
    s = _Session(plan, case)
    assert s.rc == 0 and L.vrt_lambda_storage(s.h) == 4 and L.vrt_lambda_storage(None) == _lib.VRT_EINVAL
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
    # a refused state (a zero in S) and a refused acceleration leave the session as it was
    assert s.set_state(S2, p2) == 0
    bad = S2.copy()
    bad[5, 5] = 0.0
    assert s.set_state(bad, p2) == _lib.VRT_EINVAL
    assert L.vrt_lambda_set_acceleration(s.h, 2, 4, 4) == _lib.VRT_EINVAL
    assert b"float" in L.vrt_last_error()
    assert s.iterate() == hist[2] and all(np.array_equal(a, b) for a, b in zip(s.get(), states[2]))
    s.close()
    # no fp64 fallback: a plan that is not on the patch path is refused
    monkeypatch.setenv("VRT_PATH", "steps")
    steps_plan = vrt.FormalPlan(sites, vrt.quadrature_directions(TH, PH), 3, dirs=DIRS)
    monkeypatch.delenv("VRT_PATH")
    refused = _Session(steps_plan, case)
    assert refused.rc == _lib.VRT_EINVAL and not refused.h
    steps_plan.close()
    monkeypatch.setenv("VRT_LAMBDA_NATIVE", "0")
    caller_plan = vrt.FormalPlan(sites, vrt.quadrature_directions(TH, PH), 3, dirs=DIRS)
    monkeypatch.delenv("VRT_LAMBDA_NATIVE")
    refused = _Session(caller_plan, case)
    assert refused.rc == _lib.VRT_EINVAL and not refused.h
    caller_plan.close()
    # checkpoints work unchanged: two iterates saved, two more resumed, equal to four in one go
    ck = str(tmp_path / "run.npz")
    vrt.Lambda_voronoi_host(0.0, 2, sites, case, QUAD, storage="f32", checkpoint=ck)
    Jr, Sr, pr, hr = vrt.Lambda_voronoi_host(0.0, 2, sites, case, QUAD, storage="f32", resume=ck)
    assert hr == hist and all(np.array_equal(a, b) for a, b in zip((Jr, Sr, pr), states[3]))
    s64 = _Session(plan, case, f32_storage=False)
    assert s64.rc == 0 and L.vrt_lambda_storage(s64.h) == 8
    s64.close()
    # an fp64 session after all this is what it was
    from test_physics import test_gpu_lambda_voronoi_device_resident_loop
    test_gpu_lambda_voronoi_device_resident_loop(voro_small)
