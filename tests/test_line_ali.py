"""Accelerated Λ-iteration of the line session on the device: vrt_line_lambda_diagonal_dev, vrt_lambda_ali_update_dev /
_native_dev, vrt_lambda_use_operator / _get_operator and Lambda_voronoi[_host](operator="diagonal"), against the
continuum operator's kernel (bit for bit, angle by angle), the numpy restatement of Λ* and the oracle-driven line ALI loop
of tests/test_line_ali_host.py.

Tolerances: Λ* against vrt_plan_lambda_diagonal: equality of bits; against its numpy restatement the two-tier 1e-12 rule of
tests/test_ali.py; the standalone updates against oracle/update_ref.py bit for bit (the build is -ffp-contract=off);
the session against the oracle loop as tests/test_physics.py has the plain session (J, S, populations 1e-9, the history
rtol 1e-8); distances between converged runs: the δ / (1 - ρ) terms of the CPU oracle runs (BOUND_TERMS of
tests/test_line_ali_host.py); iterate caps: the oracle's counts plus two."""
import ctypes

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from oracle import update_ref
from voronoirt_amd import _lib, api, synth
from test_accel import _Session
from test_ali_host import lambda_star_ref, oracle_table, updated_mask
from test_continuum_host import bcc_case
from test_line_ali_host import (BOUND_TERMS, COUNTS, MARGIN, QUAD, TARGET, hard_case, line_lambda_star_ref,
                                oracle_line_loop)
from test_physics import _lambda_case

pytestmark = pytest.mark.gpu

NLAMS = (1, 2, 3, 5, 33)


def _d(a):
    return a.ctypes.data_as(_lib.p_dbl)


def _own_plan(sites):
    w, th, ph, _ = vrt.read_quadrature(QUAD)
    plan = vrt.FormalPlan(sites, vrt.quadrature_directions(th, ph), 3, dirs=[1 if t > 90 else -1 for t in th])
    return plan, np.ascontiguousarray(w, dtype=np.float64)


def _random_alpha(base, nlam, seed):
    """one α per angle: the grid's continuum α (n,) times a random factor per (angle, site, wavelength), the columns ×
    {1, 1e3, 1e-4} in turn, so that every branch of linear_weights contributes (as tests/test_ali.py scales it; the thin
    column never stands alone: the max-norm tier of the 1e-12 rule is stated for an array that holds the thick ones too)"""
    rng = np.random.default_rng(seed)
    scale = np.array([1.0, 1e3, 1e-4])[np.arange(nlam) % 3]
    return np.ascontiguousarray(base[None, :, None] * 10.0 ** rng.uniform(-0.3, 0.3, (12, base.size, nlam)) * scale)


@pytest.fixture(scope="module")
def grids(voro_small):
    """bcc 648 sites and voro_small: sites, oracle sites and tables, and per nλ the random per-angle α with its Λ* summed
    angle by angle from the continuum operator's kernel -- the reference, computed once"""
    out = {}
    pos, nbr, bounds, case1 = bcc_case(1)
    base = {"bcc": case1.alpha[:, 0], "voro": synth.continuum_case(voro_small[0], voro_small[2], 2, 3)["alpha"][:, 0]}
    for name, (p, nb, b) in (("bcc", (pos, nbr, bounds)), ("voro", voro_small)):
        sites = vrt.VoronoiSites(p, nb, b)
        so = orc.make_sites(p, nb, b)
        table, w = oracle_table(so, QUAD)
        plan, wq = api._quadrature_plan(sites, QUAD, 3)
        wq = np.ascontiguousarray(wq, dtype=np.float64)
        ref = {}
        for nlam in NLAMS:
            alpha = _random_alpha(base[name], nlam, 100 + nlam)
            total = None
            for a in range(12):
                only = np.zeros(12)
                only[a] = wq[a]
                part = np.zeros((sites.n, nlam))
                assert _lib.load().vrt_plan_lambda_diagonal(plan._h, nlam, nlam, _d(alpha[a]), _d(only), _d(part)) == 0
                total = part if total is None else total + part
            ref[nlam] = (alpha, total)
        out[name] = {"sites": sites, "so": so, "table": table, "w": w, "ref": ref}
    return out


def _line_diag_dev(plan, w, alpha, ld):
    """vrt_plan_alpha_to_native_dev then vrt_line_lambda_diagonal_dev with leading dimension ld and -7 in the padding"""
    import torch
    dev = torch.device("cuda", 0)
    nq, n, nlam = alpha.shape
    wide = np.full((nq, n, ld), np.nan)                        # (NaN in every column nothing should read)
    wide[:, :, :nlam] = alpha
    d_alpha = torch.from_numpy(wide).to(dev)
    native = torch.full((plan.native_alpha_count(nlam),), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full((n, ld), -7.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    plan.alpha_to_native_dev(nlam, ld, d_alpha.data_ptr(), native.data_ptr(), stream=st)
    plan.line_lambda_diagonal_dev(nlam, native.data_ptr(), w, ld, out.data_ptr(), stream=st)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1: Λ* against the existing kernel, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("pair_block", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("grid", ["bcc", "voro"])
def test_gpu_line_lambda_diagonal_is_the_continuum_kernel_angle_by_angle(grids, grid, pair_block, monkeypatch):
    """every pair block the plan option offers against nλ = 1, 2, 3, 5, 33 (1, 1, 2, 3, 17 pairs: blocks that divide the
    pair count, blocks that do not -- 17 pairs in blocks of 8, 8, 1 -- and the half pair of an odd nλ)"""
    g = grids[grid]
    sites, so = g["sites"], g["so"]
    monkeypatch.setenv("VRT_PAIR_BLOCK", str(pair_block))      # read when the plan is created
    plan, w = _own_plan(sites)
    try:
        print(f"{grid}: VRT_PAIR_BLOCK={pair_block}, the plan's native pair block {plan.native_pair_block}")
        if grid == "voro":
            assert plan.native_pair_block == pair_block
        never = ~(updated_mask(so, True) | updated_mask(so, False))
        for nlam in NLAMS:
            alpha, ref = g["ref"][nlam]
            ld = nlam + 2
            got = _line_diag_dev(plan, w, alpha, ld)
            assert (got[:, nlam:] == -7.0).all()
            got = got[:, :nlam]
            assert np.array_equal(got, ref), (nlam, np.abs(got - ref).max())
            assert np.array_equal(_line_diag_dev(plan, w, alpha, ld)[:, :nlam], got)      # the same bits twice
            assert never.sum() >= 1 and (got[never] == 0.0).all() and (got[~never] > 0).all()
            if pair_block == 1:                                 # the formula itself, once per (grid, nλ)
                table = g["table"]
                num = line_lambda_star_ref(so, table, alpha, g["w"])
                mid_min = np.full(num.shape, np.inf)
                branches = set()
                for a in range(12):
                    only = [e if b == a else None for b, e in enumerate(table)]
                    _, br, mm = lambda_star_ref(so, only, alpha[a], g["w"], return_branches=True)
                    branches |= br
                    mid_min = np.minimum(mid_min, mm)
                if nlam >= 3:
                    assert branches == {0, 1, 2}
                err = np.abs(got - num) / np.where(num > 0, num, 1.0)
                well = mid_min >= 0.03
                print(f"{grid} nλ={nlam}: max-norm {np.abs(got - num).max() / np.abs(num).max():.3g}; entry-wise "
                      f"{err.max():.3g} over all entries, {err[well].max() if well.any() else 0:.3g} over the "
                      f"{int(well.sum())} of {well.size} well-conditioned ones")
                assert np.abs(got - num).max() <= 1e-12 * np.abs(num).max()
                assert not well.any() or err[well].max() <= 1e-12
    finally:
        plan.close()


def test_gpu_line_lambda_diagonal_python_entry_and_inactive_angle(grids):
    g = grids["bcc"]
    alpha, ref = g["ref"][5]
    assert np.array_equal(vrt.line_lambda_diagonal(g["sites"], alpha, QUAD), ref)
    with pytest.raises(ValueError):
        vrt.line_lambda_diagonal(g["sites"], alpha[:11], QUAD)
    # a plan with a θ = 90 direction: per-angle α needs every angle active
    import torch
    k = np.ascontiguousarray(np.stack([vrt.direction(150.0, 20.0), vrt.direction(90.0, 0.0), vrt.direction(30.0, 70.0)]))
    plan = vrt.FormalPlan(g["sites"], k, 3, dirs=[1, 0, -1])
    try:
        buf = torch.zeros(3 * 2 * g["sites"].n + 64, dtype=torch.float64, device="cuda:0")
        out = torch.full((g["sites"].n, 2), -7.0, dtype=torch.float64, device="cuda:0")
        rc = _lib.load().vrt_line_lambda_diagonal_dev(plan._h, 2, buf.data_ptr(), _d(np.ones(3)), 2, out.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == _lib.VRT_EINVAL and bool((out == -7.0).all())
    finally:
        plan.close()


# ---- 2: the standalone ALI updates -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlam", [1, 2, 3, 5])
def test_gpu_line_ali_updates_on_hand_made_arrays(grids, nlam):
    """rows (ld > nlam) and sweep-order planes against the numpy formula; one planted entry with ε = 0 and Λ* = 1 takes the
    plain value and is counted; a planted NaN makes the scalar NaN"""
    import torch
    sites = grids["bcc"]["sites"]
    n, ld = sites.n, nlam + 2
    rng = np.random.default_rng(20 + nlam)
    J, B, S_old = (1.0 + rng.random((n, ld)) for _ in range(3))
    eps = 10.0 ** rng.uniform(-7, 0, n)
    diag = rng.random((n, ld)) * 0.999
    J += diag * S_old                                          # (J >= Λ* S_old, as every true J is)
    at = (n // 3, nlam - 1)
    eps[at[0]] = 0.0
    diag[at] = 1.0
    e = eps[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = ((1 - e) * (J - diag * S_old) + e * B) / (1 - (1 - e) * diag)
    plain = (1 - e) * J + e * B
    ref[at] = plain[at]
    dev = torch.device("cuda", sites.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def rows(B_):
        S_new = torch.full((n, ld), -7.0, dtype=torch.float64, device=dev)
        args = [t(a) for a in (J, B_, eps, diag, S_old)]        # (alive until the call has returned)
        d, c = vrt.lambda_ali_update_dev(sites, nlam, ld, *(a.data_ptr() for a in args), S_new.data_ptr(), stream=st)
        return d, c, S_new.cpu().numpy()

    d, c, S_new = rows(B)
    assert c == 1 and S_new[at] == plain[at] and (S_new[:, nlam:] == -7.0).all()
    model = update_ref.update_model("line_ali", J, B, eps, S_old, diag=diag, nlam=nlam)
    assert np.array_equal(S_new[:, :nlam], model.S_new[:, :nlam]) and np.array_equal(model.S_new[:, :nlam], ref[:, :nlam])
    assert d == np.abs(1 - S_old / S_new)[:, :nlam].max()      # (the criterion of the S the device wrote: exact)
    Bn = B.copy()
    Bn[5, 0] = np.nan
    dn, cn, Sn = rows(Bn)
    assert np.isnan(dn) and cn == 1 and np.isnan(Sn[5, 0])
    # the same numbers through the sweep-order planes: S, the scalar and the count of the rows form, bit for bit
    plan, _ = api._quadrature_plan(sites, QUAD, 3)
    cnt = plan.native_plane_count(nlam)

    def planes(a, both=False):
        up, down = (torch.zeros(cnt, dtype=torch.float64, device=dev) for _ in range(2))
        rows_ = t(a)
        plan.to_native_dev(nlam, ld, rows_.data_ptr(), up.data_ptr(), down.data_ptr() if both else 0, stream=st)
        torch.cuda.synchronize()                                # (rows_ goes here)
        return (up, down) if both else up

    J_up, J_dn = planes(J / 2, both=True)                      # (J / 2 + J / 2 is J exactly)
    S_up, S_dn = planes(S_old, both=True)
    B_up, L_up, d_eps = planes(B), planes(diag), t(eps)
    d2, c2 = vrt.lambda_ali_update_native_dev(sites, nlam, J_up.data_ptr(), J_dn.data_ptr(), B_up.data_ptr(), d_eps.data_ptr(),
                                              L_up.data_ptr(), S_up.data_ptr(), S_dn.data_ptr(), stream=st)
    back = torch.zeros((n, nlam), dtype=torch.float64, device=dev)
    plan.from_native_dev(1, nlam, nlam, S_up.data_ptr(), back.data_ptr(), stream=st)
    back_dn = torch.zeros((n, nlam), dtype=torch.float64, device=dev)
    plan.from_native_dev(-1, nlam, nlam, S_dn.data_ptr(), back_dn.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert (d2, c2) == (d, c)
    assert np.array_equal(back.cpu().numpy(), S_new[:, :nlam]) and torch.equal(back, back_dn)


# ---- 3 ... 9: the session -----------------------------------------------------------------------------------------------------------
class _Line(_Session):
    """test_accel._Session on vrt_lambda_* with the operator entries"""

    def select(self, op):
        return self.L.vrt_lambda_use_operator(self.h, op)

    def operator(self):
        op, fb = ctypes.c_int(-1), ctypes.c_int64(-1)
        assert self.L.vrt_lambda_get_operator(self.h, ctypes.byref(op), ctypes.byref(fb)) == 0
        return op.value, fb.value

    def set_state(self, S, pops):
        _lib.check(self.L.vrt_lambda_set_state(self.h, _d(np.ascontiguousarray(S)), _d(np.ascontiguousarray(pops))))


def _sessions(voro_small, count, case=None, f32=False):
    pos, nbr, bounds = voro_small
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    case = _lambda_case(pos, bounds, 11) if case is None else case
    plan, w = api._quadrature_plan(hs, QUAD, 3)
    lc, keep = case.c_struct()
    wd = np.ascontiguousarray(w, dtype=np.float64)
    entry = _lib.load().vrt_lambda_create_f32 if f32 else _lib.load().vrt_lambda_create
    create = lambda out: entry(plan._h, ctypes.byref(lc), _d(wd), out)
    sessions = [_Line("vrt_lambda", create, hs.n, int(keep["lam"].size)) for _ in range(count)]
    return hs, case, sessions, (lc, keep, wd)


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def test_gpu_line_ali_session_matches_the_oracle_loop(voro_small):
    """four iterates of the standard case: J, S, populations and the history as tests/test_physics.py has them for the
    plain session; and S is not the plain session's"""
    pos, nbr, bounds = voro_small
    so = orc.make_sites(pos, nbr, bounds)
    table, _ = oracle_table(so, QUAD)
    hs, case, (ali, plain), keep = _sessions(voro_small, 2)
    try:
        assert ali.select(1) == 0 and ali.operator() == (1, 0) and plain.operator() == (0, 0)
        hist = [ali.iterate() for _ in range(4)]
        for _ in range(4):
            plain.iterate()
        J, S, pops = ali.get()[:3]
        J_ref, S_ref, pops_ref, hist_ref, seen = oracle_line_loop(case, so, table, 4, ali=True)
        print(f"|J - ref| / max {np.abs(J - J_ref).max() / np.abs(J_ref).max():.3g}, S {np.abs(S / S_ref - 1).max():.3g}, "
              f"populations {np.abs(pops / pops_ref - 1).max():.3g}; history {hist} against {hist_ref}")
        assert np.abs(J - J_ref).max() < 1e-9 * np.abs(J_ref).max() and np.abs(S / S_ref - 1).max() < 1e-9
        assert np.abs(pops / pops_ref - 1).max() < 1e-9
        assert np.allclose(hist, hist_ref, rtol=1e-8)
        assert ali.operator() == (1, 0) and seen["fallback"] == 0
        assert np.abs(S / plain.get()[1] - 1).max() > 1e-3     # a different iteration
    finally:
        ali.close()
        plain.close()
        hs.close()


def test_gpu_line_ali_layouts_and_public_entries_agree(voro_small, monkeypatch):
    """VRT_LAMBDA_NATIVE = 1 (Λ* written as an up-order plane set; 33 wavelengths: a padding wavelength) and = 0 (rows), and
    the loops over the public entries in both forms: the same bits"""
    results = {}
    for native in ("1", "0"):
        monkeypatch.setenv("VRT_LAMBDA_NATIVE", native)              # read when the plan is made
        hs, case, (s,), _ = _sessions(voro_small, 1)
        try:
            assert s.select(1) == 0
            hist = [s.iterate() for _ in range(3)]
            results[native] = (s.get()[:3], hist)
        finally:
            s.close()
            hs.close()
    monkeypatch.delenv("VRT_LAMBDA_NATIVE")
    (g1, h1), (g0, h0) = results["1"], results["0"]
    assert h1 == h0 and _same(g1, g0)
    pos, nbr, bounds = voro_small
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    try:
        for native in (True, False):
            J, S, pops, hist = vrt.Lambda_voronoi(0.0, 3, hs, case, QUAD, native=native, operator="diagonal")
            assert hist == h1 and _same((J, S, pops), g1), native
        Jh, Sh, ph, hh = vrt.Lambda_voronoi_host(0.0, 3, hs, case, QUAD, operator="diagonal")
        assert hh == h1 and _same((Jh, Sh, ph), g1)
    finally:
        hs.close()


def test_gpu_line_operator_switched_off_again_is_the_plain_session(voro_small):
    hs, case, (plain, s), _ = _sessions(voro_small, 2)
    try:
        assert s.operator() == (0, 0)
        assert s.select(1) == 0 and s.operator()[0] == 1
        assert s.select(0) == 0 and s.operator() == (0, 0)
        for it in range(3):
            assert plain.iterate() == s.iterate()
            assert _same(plain.get(), s.get()), it
    finally:
        plain.close()
        s.close()
        hs.close()


@pytest.fixture(scope="module")
def hard_runs(voro_small):
    """the hard variant on the device to TARGET: plain, ALI, ALI + Ng"""
    pos, nbr, bounds = voro_small
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    case = hard_case(_lambda_case(pos, bounds, 11))
    cap = COUNTS["hard"][0] + 50
    try:
        return {"plain": vrt.Lambda_voronoi_host(TARGET, cap, hs, case, QUAD),
                "ali": vrt.Lambda_voronoi_host(TARGET, cap, hs, case, QUAD, operator="diagonal"),
                "ali_ng": vrt.Lambda_voronoi_host(TARGET, cap, hs, case, QUAD, operator="diagonal", ng=(4, 4))}
    finally:
        hs.close()


def test_gpu_line_ali_needs_fewer_iterates_on_the_hard_variant(hard_runs):
    (_, S0, _, h0), (_, S1, _, h1) = hard_runs["plain"], hard_runs["ali"]
    dist = np.abs(S1 / S0 - 1).max()
    print(f"hard variant to {TARGET:g}: plain {len(h0)} iterates, ALI {len(h1)} (oracle: {COUNTS['hard']}); "
          f"|S_ali / S_plain - 1| = {dist:.3g}, bound {sum(BOUND_TERMS['hard']):.3g}")
    assert h0[-1] <= TARGET and h1[-1] <= TARGET
    assert len(h1) <= COUNTS["hard"][1] + MARGIN and len(h1) < len(h0)
    assert dist < sum(BOUND_TERMS["hard"])


def test_gpu_line_ali_composes_with_ng(hard_runs):
    """a step is applied, the run converges, and it ends where the ALI run ends: between its steps an accelerated run is an
    ALI run, so at TARGET it is within the ALI term of the fixed point, as the ALI run is"""
    (_, S1, _, h1), (_, S2, pops2, h2, steps) = hard_runs["ali"], hard_runs["ali_ng"]
    dist = np.abs(S2 / S1 - 1).max()
    print(f"ALI + Ng(4, 4): {len(h2)} iterates (ALI alone {len(h1)}), steps {[(i, ok) for i, ok, _, _ in steps]}; "
          f"|S_ng / S_ali - 1| = {dist:.3g}, bound {2 * BOUND_TERMS['hard'][1]:.3g}")
    assert any(ok for _, ok, _, _ in steps)
    assert h2[-1] <= TARGET
    assert np.isfinite(S2).all() and (S2 > 0).all() and (pops2 > 0).all()
    assert dist < 2 * BOUND_TERMS["hard"][1]


def test_gpu_line_ali_run_resumes_bit_for_bit(voro_small):
    """the state after iterate 3 into a fresh session with the operator selected: iterates 4-6 of the uninterrupted run"""
    hs, case, (whole, fresh), _ = _sessions(voro_small, 2)
    try:
        assert whole.select(1) == 0 and fresh.select(1) == 0
        for _ in range(3):
            whole.iterate()
        _, S3, pops3 = whole.get()[:3]
        fresh.set_state(S3, pops3)
        for it in (4, 5, 6):
            assert whole.iterate() == fresh.iterate(), it
            assert _same(whole.get(), fresh.get()), it
    finally:
        whole.close()
        fresh.close()
        hs.close()


def test_gpu_line_operator_refusals(voro_small):
    hs, case, (f,), _ = _sessions(voro_small, 1, f32=True)
    hs2, _, (s,), _ = _sessions(voro_small, 1)
    L = _lib.load()
    try:
        assert L.vrt_lambda_storage(f.h) == 4
        assert f.select(1) == _lib.VRT_EINVAL and L.vrt_lambda_storage(f.h) == 4 and f.operator() == (0, 0)
        d_f = f.iterate()                                       # and it goes on as a float session
        assert np.isfinite(d_f)
        assert s.select(2) == _lib.VRT_EINVAL and s.select(-1) == _lib.VRT_EINVAL and s.operator() == (0, 0)
        assert L.vrt_lambda_use_operator(None, 1) == _lib.VRT_EINVAL
        assert L.vrt_lambda_get_operator(None, None, None) == _lib.VRT_EINVAL
        with pytest.raises(ValueError):
            vrt.Lambda_voronoi_host(1e-3, 3, hs2, case, QUAD, storage="f32", operator="diagonal")
        with pytest.raises(ValueError):
            vrt.Lambda_voronoi(1e-3, 3, hs2, case, QUAD, native=True, storage="f32", operator="diagonal")
    finally:
        f.close()
        s.close()
        hs.close()
        hs2.close()
