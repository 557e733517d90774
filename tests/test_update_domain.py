"""GPU tests (-m gpu) of the Λ-iteration's "update + criterion" kernels at their value edges and launch seams (DESIGN.md
§7r): k_lambda_update<false/true>, k_lambda_update_native<false/true>, k_lambda_update_native_f32 (vrt_kernels.hip),
k_continuum_update<false/true>, k_continuum_update_native<false/true> and k_ali_min_den (vrt_continuum.hip) against
oracle/update_ref.py, whose case list tests/test_update_domain_host.py proves sufficient on the CPU.

Every comparison with the model is bit for bit -- S_new, the down-order copy, the scalar's bits or its NaN-ness, the third
word, untouched padding columns (rows) and zero pad wavelengths (planes); there is no tolerance in this file.

Grids: vrt.voro on seeded random sites in the voro_small box, 63 ... 257 sites, built once per module, one quadrature plan
per grid (and one per float layout of test_f32_lambda.LAYOUTS).  A seam of a sweep-order kernel is a storage POSITION of
the up order (the kernel's thread index); the site planted at is vrt_grid_get_storage_order's site of that position.

Out of reach: the sweep-order kernels' own second grid-stride trip needs more than 2^20 sites; a grid and a plan of that
size do not fit a test of a few seconds.  The row kernels' second trip is here (257 x 4081 entries).
"""
import ctypes
import os

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import update_ref as R
from oracle.layout_ref import pair_index
from voronoirt_amd import _lib, api

pytestmark = pytest.mark.gpu

QUAD = "ul7n12.dat"
BOUNDS = (0.0, 2.0, 0.0, 1.0, 0.0, 1.0)                        # the box of conftest.voro_small
SITES = (63, 64, 65, 255, 256, 257)
NLAMS = {"line": (1, 2, 7, 8, 9, 17), "line_ali": (1, 2, 7, 8, 9, 17), "continuum": (1, 2, 3, 4, 5),
         "continuum_ali": (1, 2, 3, 4, 5), "line_f32": (1, 2, 3, 5, 7, 8, 9, 17)}
LAYOUTS = {"default": ({}, 2), "pairs": ({"VRT_PATCH_QUAD": "0"}, 1), "block8": ({"VRT_PAIR_BLOCK": "8"}, 8)}     # test_f32_lambda
BIG = (257, 4081)
PAD = 2                                                         # padding columns of the row forms, filled with -7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bit for bit, a NaN matching a NaN (its sign and payload are not the model's business)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def same_scalar(got, want):
    return bool(same(got, want))


class Grid:
    def __init__(self, n):
        rng = np.random.default_rng(1000 + n)
        z0, z1, x0, x1, y0, y1 = BOUNDS
        self.pos = np.ascontiguousarray(np.stack([z0 + rng.random(n) * (z1 - z0), x0 + rng.random(n) * (x1 - x0),
                                                  y0 + rng.random(n) * (y1 - y0)], axis=1))
        # the two sites nearest mid-height come first and last: the first and the last thread of k_ali_min_den are then cells
        # every angle updates, where Λ* can round to 1 (test_min_den_is_seen_at_every_seam)
        mid = np.argsort(np.abs(self.pos[:, 0] - 0.5 * (z0 + z1)))[:2]
        order = [i for i in range(n) if i not in mid]
        self.pos = np.ascontiguousarray(self.pos[[mid[0]] + order + [mid[1]]])
        self.nbr = vrt.voro(self.pos, BOUNDS, device=0)
        self.n = n
        self.sites = vrt.VoronoiSites(self.pos, self.nbr, BOUNDS, device=0)
        self.plan, w = api._quadrature_plan(self.sites, QUAD, 3)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.store_up = self.sites.storage_order(+1) - 1        # the site at every up position
        self.store_dn = self.sites.storage_order(-1) - 1
        self.rank_up, self.rank_dn = np.argsort(self.store_up), np.argsort(self.store_dn)
        self.f32_plans = {}

    def f32_plan(self, layout):
        if layout not in self.f32_plans:
            env, B = LAYOUTS[layout]
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                _, th, ph, _ = vrt.read_quadrature(QUAD)
                self.f32_plans[layout] = vrt.FormalPlan(self.sites, vrt.quadrature_directions(th, ph), 3,
                                                        dirs=[1 if t > 90 else -1 for t in th])
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            assert self.f32_plans[layout].native_pair_block_f32 == B
        return self.f32_plans[layout]

    def close(self):
        self.sites.close()


@pytest.fixture(scope="module")
def grids():
    made = {}

    def get(n):
        if n not in made:
            made[n] = Grid(n)
        return made[n]

    yield get
    for g in made.values():
        g.close()


# ---- one entry point on one grid and wavelength count: arrays on the device, poked in place ---------------------------
class Rows:
    """the caller-layout entries: (n, nlam + PAD) arrays, the padding columns -7 in S_new and NaN in what is read"""
    form = "rows"

    def __init__(self, kind, grid, nlam, case):
        import torch
        self.torch, self.kind, self.g, self.nlam, self.n = torch, kind, grid, nlam, grid.n
        self.dev = torch.device("cuda", 0)
        self.ld = nlam + PAD
        self.st = torch.cuda.current_stream(self.dev).cuda_stream
        self.launch = R.launch_of(kind, "rows")
        self.d = {}
        for key in ("J", "B", "S_old", "diag"):
            if case[key] is not None:
                self.d[key] = self.wide(case[key])
        self.d["eps"] = self.wide(case["eps"]) if kind in R.CONTINUUM else torch.from_numpy(np.ascontiguousarray(case["eps"])).to(self.dev)
        self.eps_thick = case["eps_thick"]
        self.S_new = torch.empty((self.n, self.ld), dtype=torch.float64, device=self.dev)

    def wide(self, a):
        w = np.full((self.n, self.ld), np.nan)
        w[:, :self.nlam] = a
        return self.torch.from_numpy(w).to(self.dev)

    def poke(self, key, site, l, value):
        """set one entry (l None: ε of a site), returning what it held"""
        t = self.d[key]
        at = (site,) if l is None else (site, l)
        old = t[at].clone()
        t[at] = value
        return old

    def site_of(self, row):
        return row                                              # (the row kernels' index is the site)

    def run(self):
        d, p = self.d, lambda key: self.d[key].data_ptr()
        self.S_new.fill_(-7.0)
        third = None
        if self.kind == "line":
            scalar = api.lambda_update_dev(self.g.sites, self.nlam, self.ld, p("J"), p("B"), p("eps"), p("S_old"),
                                           self.S_new.data_ptr(), stream=self.st)
        elif self.kind == "line_ali":
            scalar, third = api.lambda_ali_update_dev(self.g.sites, self.nlam, self.ld, p("J"), p("B"), p("eps"), p("diag"),
                                                      p("S_old"), self.S_new.data_ptr(), stream=self.st)
        elif self.kind == "continuum":
            scalar, third = vrt.continuum_update_dev(self.g.sites, d["J"], d["B"], d["eps"], d["S_old"], self.S_new,
                                                     self.eps_thick, nlam=self.nlam)
        else:
            scalar, third = vrt.continuum_ali_update_dev(self.g.sites, d["J"], d["B"], d["eps"], d["diag"], d["S_old"],
                                                         self.S_new, self.eps_thick, nlam=self.nlam)
        out = self.S_new.cpu().numpy()
        assert (out[:, self.nlam:] == -7.0).all()               # the padding columns are not written
        return out[:, :self.nlam], None, scalar, third

    def restore(self):
        pass                                                    # (S_old is only read)


class Planes:
    """the sweep-order entries (line, line_ali, line_f32): plane sets filled through to_native_dev, J as J / 2 up and J / 2
    down (or as the caller says), S read from and written to S_up, the down-order copy to S_dn"""
    form = "planes"

    def __init__(self, kind, grid, nlam, case, layout=None, J_split="halves"):
        import torch
        self.torch, self.kind, self.g, self.nlam, self.n = torch, kind, grid, nlam, grid.n
        self.f32 = kind == "line_f32"
        self.plan = grid.f32_plan(layout) if self.f32 else grid.plan
        self.B = self.plan.native_pair_block_f32 if self.f32 else 1
        assert self.f32 or self.plan.native_pair_block == 1
        self.launch = R.launch_of(kind, "planes", self.B)
        self.dev = torch.device("cuda", 0)
        self.dtype = torch.float32 if self.f32 else torch.float64
        self.st = torch.cuda.current_stream(self.dev).cuda_stream
        self.count = self.plan.native_plane_count(nlam)
        npair, n = (nlam + 1) // 2, self.n
        l = np.arange(2 * npair)
        value_index = lambda rank: 2 * pair_index((l >> 1)[None, :], rank[:, None], n, self.B, npair) + (l & 1)[None, :]
        self.idx_up, self.idx_dn = value_index(grid.rank_up), value_index(grid.rank_dn)     # [site, l] (l = nlam: the pad)
        assert self.count == 2 * npair * n and np.array_equal(np.sort(self.idx_up.ravel()), np.arange(self.count))
        J = np.asarray(case["J"], dtype=np.float64)
        up, down = {"halves": (J / 2, J / 2), "up": (J, np.zeros(J.shape)), "up_null": (J, None), "null_down": (None, J),
                    "both": (J, J)}[J_split]
        self.d = {"J_up": self.to_planes(up, +1), "J_dn": self.to_planes(down, -1), "B": self.to_planes(case["B"], +1),
                  "S_old": self.to_planes(case["S_old"], +1)}
        self.index = {"J_up": self.idx_up, "J_dn": self.idx_dn, "B": self.idx_up, "S_old": self.idx_up, "diag": self.idx_up}
        if case["diag"] is not None:
            self.d["diag"] = self.to_planes(case["diag"], +1)
        self.d["eps"] = torch.from_numpy(np.ascontiguousarray(case["eps"])).to(self.dev)
        self.pristine = self.d["S_old"].clone()
        self.S_dn = torch.empty(self.count, dtype=self.dtype, device=self.dev)

    def to_planes(self, a, d):
        """a caller-layout array -> the plane set of direction d through vrt_plan_to_native_dev[_f32] (None stays None)"""
        if a is None:
            return None
        torch = self.torch
        rows = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if self.f32 else np.float64)).to(self.dev)
        out = torch.full((self.count,), float("nan"), dtype=self.dtype, device=self.dev)
        self.plan.to_native_dev(self.nlam, self.nlam, rows.data_ptr(), out.data_ptr() if d > 0 else 0,
                                0 if d > 0 else out.data_ptr(), stream=self.st, f32=self.f32)
        torch.cuda.synchronize()
        return out

    def back(self, d, planes):
        torch = self.torch
        out = torch.full((self.n, self.nlam), float("nan"), dtype=self.dtype, device=self.dev)
        self.plan.from_native_dev(d, self.nlam, self.nlam, planes.data_ptr(), out.data_ptr(), stream=self.st, f32=self.f32)
        torch.cuda.synchronize()
        return out.cpu().numpy().astype(np.float64)

    def poke(self, key, site, l, value):
        if l is None:
            old = self.d["eps"][site].clone()
            self.d["eps"][site] = value
            return old
        if key == "J":                                          # (J / 2 up and J / 2 down: only a value whose half is exact)
            for k in ("J_up", "J_dn"):
                self.d[k][int(self.index[k][site, l])] = value / 2
            return None
        t, i = self.d[key], int(self.index[key][site, l])
        old = t[i].clone()
        t[i] = value
        return old

    def site_of(self, row):
        return int(self.g.store_up[row])                        # (a sweep-order kernel's index is the up position)

    def run(self, through_from_native=False):
        p = lambda key: 0 if self.d.get(key) is None else self.d[key].data_ptr()
        self.S_dn.fill_(float("nan"))
        S_up, third = self.d["S_old"], None
        if self.kind == "line":
            scalar = api.lambda_update_native_dev(self.g.sites, self.nlam, p("J_up"), p("J_dn"), p("B"), p("eps"),
                                                  S_up.data_ptr(), self.S_dn.data_ptr(), stream=self.st)
        elif self.kind == "line_ali":
            scalar, third = api.lambda_ali_update_native_dev(self.g.sites, self.nlam, p("J_up"), p("J_dn"), p("B"), p("eps"),
                                                             p("diag"), S_up.data_ptr(), self.S_dn.data_ptr(), stream=self.st)
        else:
            scalar = api.lambda_update_native_dev_f32(self.plan, self.nlam, p("J_up"), p("J_dn"), p("B"), p("eps"),
                                                      S_up.data_ptr(), self.S_dn.data_ptr(), stream=self.st)
        raw_up, raw_dn = S_up.cpu().numpy().astype(np.float64), self.S_dn.cpu().numpy().astype(np.float64)
        if self.nlam & 1:                                       # the pad wavelength: written as zero in both orders
            assert not raw_up[self.idx_up[:, self.nlam]].any() and not raw_dn[self.idx_dn[:, self.nlam]].any()
        up, dn = raw_up[self.idx_up[:, :self.nlam]], raw_dn[self.idx_dn[:, :self.nlam]]
        if through_from_native:                                 # the index map above is the library's own
            assert same(self.back(+1, S_up), up).all() and same(self.back(-1, self.S_dn), dn).all()
        return up, dn, scalar, third

    def restore(self):
        self.d["S_old"].copy_(self.pristine)


def check(runner, want, what, **kw):
    """one call against an Update of the model: S_new in both orders, the scalar, the third word -- bit for bit"""
    up, dn, scalar, third = runner.run(**kw)
    S = want.S_new[:, :runner.nlam]
    ok = same(up, S)
    assert ok.all(), (what, np.argwhere(~ok)[:5], up[~ok][:5], S[~ok][:5])
    if dn is not None:
        assert same(dn, S).all(), what
    print(f"{what}: scalar {scalar!r} (model {want.scalar!r}), third word {third} (model {want.third})")
    assert same_scalar(scalar, want.scalar), (what, scalar, want.scalar)
    assert third == want.third, (what, third, want.third)
    return up


def runners(kind, grid, nlam, case, **kw):
    """every entry of the kind: rows and planes (the float kind: planes of every layout; the continuum: rows alone -- its
    sweep-order kernel has no entry of its own)"""
    if kind == "line_f32":
        return [(f"planes/{layout}", Planes(kind, grid, nlam, case, layout=layout, **kw)) for layout in LAYOUTS]
    if kind in R.CONTINUUM:
        return [("rows", Rows(kind, grid, nlam, case))]
    return [("rows", Rows(kind, grid, nlam, case)), ("planes", Planes(kind, grid, nlam, case, **kw))]


# ---- 1: the value grid ---------------------------------------------------------------------------------------------------------
def _embed(kind, g, n, rows_at):
    """the value grid's rows at the sites rows_at of an n-site benign case"""
    nlam = g["B"].shape[1]
    c = R.benign_case(kind, n, nlam, seed=5)
    for key in ("J", "B", "S_old", "diag"):
        if g[key] is not None:
            c[key][rows_at] = g[key]
    c["eps"][rows_at] = g["eps"]
    c["eps_thick"] = g["eps_thick"]
    return c


@pytest.mark.parametrize("kind", R.KINDS)
def test_value_grid(grids, kind):
    """the edge set through every entry of the kind; class by class, and whole, the device agrees with the model: the bits
    of S_new, the words, and the class of every entry as the device's S_new gives it"""
    grid = grids(257)
    n = grid.n
    g = R.value_grid(kind)
    g["eps_thick"] = R.VALUE_EPS_THICK if kind in R.CONTINUUM else None
    rows, nlam = g["B"].shape
    rows_at = np.linspace(0, n - 1, rows).astype(int)          # spread over the waves and workgroups of the launch
    assert np.unique(rows_at).size == rows and nlam == 343
    cls = R.classify(kind, R.run_case(kind, g))
    filler = R.benign_case(kind, rows, nlam, seed=11)
    variants = [("whole", g)] + [(f"class {name}", R.class_case(kind, g, filler, cls == k))
                                 for k, name in enumerate(R.CLASSES) if (cls == k).any()]
    # (J = J + 0: 2^-1074 has no exact half; the float kind's sum J + J overflows as a float at the largest one)
    splits = ["up", "up_null", "null_down"] + (["both"] if kind == "line_f32" else [])
    for vname, v in variants:
        c = _embed(kind, v, n, rows_at)
        for split in (splits if vname == "whole" else splits[:1]):
            want = R.run_case(kind, dict(c, J=2 * c["J"]) if split == "both" else c)
            want_cls = R.classify(kind, want)
            for rname, r in runners(kind, grid, nlam, c, J_split=split):
                if split != "up" and r.form == "rows":
                    continue
                up = check(r, want, f"{kind} {rname} {vname} J:{split}", **({"through_from_native": True} if r.form == "planes" else {}))
                # the class of every entry from what the device wrote
                got = R.Update(up, None, None, dict(want.parts, term=R._terms(np.asarray(c["S_old"], dtype=np.float64), up)))
                assert np.array_equal(R.classify(kind, got), want_cls)
        counts = {name: int((want_cls[rows_at] == k).sum()) for k, name in enumerate(R.CLASSES)}
        print(f"{kind} {vname}: classes of the grid's entries {counts}")


# ---- 2: the seams --------------------------------------------------------------------------------------------------------------
def _planted(kind, runner, base, what, site, l):
    """poke the plant `what` at (site, l) into the runner's device arrays, run, check against the model of the planted
    case, and put everything back"""
    c, scalar, third, nan_at = R.plant(kind, base, what, site, l)
    undo = []
    for key in ("J", "B", "S_old", "diag"):
        if c[key] is None:
            continue
        for at in np.argwhere(~same(c[key], base[key])):
            old = runner.poke(key, int(at[0]), int(at[1]), float(c[key][tuple(at)]))
            undo.append((key, int(at[0]), int(at[1]), float(base[key][tuple(at)]) if old is None else old))
    e_changed = np.argwhere(~same(c["eps"], base["eps"]))
    for at in e_changed:
        if kind in R.CONTINUUM:
            undo.append(("eps", int(at[0]), int(at[1]), runner.poke("eps", int(at[0]), int(at[1]), float(c["eps"][tuple(at)]))))
        else:
            undo.append(("eps", int(at[0]), None, runner.poke("eps", int(at[0]), None, float(c["eps"][at[0]]))))
    thick_before = getattr(runner, "eps_thick", None)
    if kind in R.CONTINUUM:
        runner.eps_thick = c["eps_thick"]
    want = R.run_case(kind, c)
    up, dn, got_scalar, got_third = runner.run()
    where = (kind, runner.form, what, site, l)
    S = want.S_new[:, :runner.nlam]
    assert same(up, S).all() and (dn is None or same(dn, S).all()), where
    # what the plant states by itself, from the planted entry alone
    if scalar is not None:
        assert same_scalar(got_scalar, scalar), (where, got_scalar, scalar)
        assert what != "term" or R.PLANT_FLOOR < got_scalar < 0.7
    assert got_third == third, (where, got_third, third)
    if nan_at is not None:
        assert np.isnan(up[nan_at]) and np.isnan(up).sum() == 1, where
    if what == "fallback":
        assert same(up[site, l], want.parts["plain"][site, l]), where
    # ... and the whole model
    assert same_scalar(got_scalar, want.scalar) and got_third == want.third, (where, got_scalar, want.scalar, got_third, want.third)
    for key, a, b, old in undo:
        runner.poke(key, a, b, old)
    if kind in R.CONTINUUM:
        runner.eps_thick = thick_before
    runner.restore()


def _plants(kind):
    return ["term", "nan", "inf"] + (["fallback", "fallback_site"] if kind == "line_ali" else []) + \
        (["only_thick"] if kind in R.CONTINUUM else [])


@pytest.mark.parametrize("n", SITES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_planted_extreme_is_seen_at_every_seam(grids, kind, n):
    """benign data (every term below 0.1); at every case of seam_cases in turn: a term of about 0.5 (the scalar is that
    term's bits), a NaN (the scalar is NaN, S_new is NaN there only), a term of +Inf, ε = 0 with Λ* = 1 (line ALI: counted
    once, the plain value; a whole site: counted nlam times), the only thick entry (continuum: counted once, the scalar its
    term).  On 65 and 257 sites every site is planted once more at the first and the last wavelength (of the largest nlam),
    so that the result does not rest on knowing the storage order."""
    grid = grids(n)
    planted = 0
    for nlam in NLAMS[kind]:
        base = R.benign_case(kind, n, nlam, seed=n + nlam)
        want = R.run_case(kind, base)
        assert want.scalar < R.BENIGN_BOUND
        for rname, r in runners(kind, grid, nlam, base):
            check(r, want, f"{kind} {rname} {n} x {nlam} benign")
            r.restore()
            for name, row, l in R.seam_cases(n, nlam, r.launch):
                for what in _plants(kind):
                    _planted(kind, r, base, what, r.site_of(row), l)
                    planted += 1
            if n in (65, 257) and nlam == NLAMS[kind][-1]:
                for site in range(n):
                    for l in {0, nlam - 1}:
                        _planted(kind, r, base, "term", site, l)
                        planted += 1
    print(f"{kind}, {n} sites: {planted} planted calls")


# ---- 3: a clean call after a dirty one -----------------------------------------------------------------------------------------
def test_clean_call_after_a_dirty_one(grids):
    """the result words live in the grid's scalars and are cleared per call, two or three of them: after a NaN call, a call
    with five fallback entries and a continuum call with a thick count, the plain update and the clean ALI update return
    the clean model's words -- rows and planes"""
    grid = grids(257)
    n, nlam = grid.n, 7
    base = {k: R.benign_case(k, n, nlam, seed=21) for k in ("line", "line_ali", "continuum")}
    clean = {k: R.run_case(k, base[k]) for k in base}
    for form in (Rows, Planes):
        ali, plain = form("line_ali", grid, nlam, base["line_ali"]), form("line", grid, nlam, base["line"])
        cont = Rows("continuum", grid, nlam, base["continuum"])
        # 1: a NaN
        old = ali.poke("B", 100, 3, float("nan"))
        _, _, d, c = ali.run()
        assert np.isnan(d) and c == 0
        ali.poke("B", 100, 3, old)
        ali.restore()
        # 2: five fallback entries
        sites = (0, 63, 64, 200, 256)
        undo = [(s, ali.poke("eps", s, None, 0.0), ali.poke("diag", s, 6, 1.0)) for s in sites]
        _, _, d, c = ali.run()
        assert c == 5
        for s, e, L in undo:
            ali.poke("eps", s, None, e)
            ali.poke("diag", s, 6, L)
        ali.restore()
        # 3: a continuum call with a thick count
        _, _, d, c = cont.run()
        assert c == n * nlam == clean["continuum"].third
        # 4, 5: the clean calls
        check(plain, clean["line"], f"{form.__name__}: plain update after the dirty calls")
        check(ali, clean["line_ali"], f"{form.__name__}: ALI update after the dirty calls")


def test_clean_iterate_after_the_operator_was_on(voro_small):
    """a line session with the operator switched on for an iterate and off again: from the same state, its next iterate is a
    session's that never had the operator -- the scalar, S and J bit for bit, and no fallback count left over"""
    from test_accel import _Session
    from test_physics import _lambda_case
    pos, nbr, bounds = voro_small
    hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    case = _lambda_case(pos, bounds, 11)
    plan, w = api._quadrature_plan(hs, QUAD, 3)
    lc, keep = case.c_struct()
    wd = np.ascontiguousarray(w, dtype=np.float64)
    L = _lib.load()
    create = lambda out: L.vrt_lambda_create(plan._h, ctypes.byref(lc), wd.ctypes.data_as(_lib.p_dbl), out)
    a, b = (_Session("vrt_lambda", create, hs.n, int(keep["lam"].size)) for _ in range(2))
    try:
        b.iterate()
        _, S, pops = b.get()[:3]
        assert L.vrt_lambda_use_operator(a.h, 1) == 0
        a.iterate()
        assert L.vrt_lambda_use_operator(a.h, 0) == 0
        for s in (a, b):
            _lib.check(L.vrt_lambda_set_state(s.h, np.ascontiguousarray(S).ctypes.data_as(_lib.p_dbl),
                                              np.ascontiguousarray(pops).ctypes.data_as(_lib.p_dbl)))
        da, db = a.iterate(), b.iterate()
        op, fb = ctypes.c_int(-1), ctypes.c_int64(-1)
        assert L.vrt_lambda_get_operator(a.h, ctypes.byref(op), ctypes.byref(fb)) == 0 and (op.value, fb.value) == (0, 0)
        assert same_scalar(da, db) and np.isfinite(da) and da > 0
        for x, y in zip(a.get()[:3], b.get()[:3]):
            assert same(x, y).all()
    finally:
        a.close()
        b.close()
        hs.close()


# ---- 4: the second grid-stride trip of the row kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["line_ali", "continuum", "continuum_ali"])
def test_second_trip_of_the_row_kernels(grids, kind):
    """257 x 4081 entries, 241 more than the 2^20 of one trip: S_new of all of them, and the planted term, NaN and count
    at entries 2^20 - 1, 2^20 and the last"""
    grid = grids(257)
    n, nlam = BIG
    assert n * nlam > R.SECOND_TRIP and grid.n == n
    base = R.benign_case(kind, n, nlam, seed=3)
    r = Rows(kind, grid, nlam, base)
    check(r, R.run_case(kind, base), f"{kind} rows {n} x {nlam} benign")
    for t in (R.SECOND_TRIP - 1, R.SECOND_TRIP, n * nlam - 1):
        assert (t // nlam, t % nlam) in {(row, l) for _, row, l in R.seam_cases(n, nlam, r.launch)}
        for what in ("term", "nan", "fallback" if kind == "line_ali" else "only_thick"):
            _planted(kind, r, base, what, t // nlam, t % nlam)


# ---- 5: the continuum session: the sweep-order kernel has no entry of its own ---------------------------------------------
def _continuum_case(grid, nlam, seed):
    rng = np.random.default_rng(seed)
    n = grid.n
    alpha = 10.0 ** rng.uniform(-1.0, 2.0, (n, nlam))
    B0 = 1.0 + rng.random((n, nlam))
    eps = 10.0 ** rng.uniform(-3.0, np.log10(0.3), (n, nlam))
    return alpha, eps, B0


@pytest.mark.parametrize("operator", [None, "diagonal"])
@pytest.mark.parametrize("nlam", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [65, 257])
def test_continuum_session_native_and_rows_agree_at_the_seams(grids, n, nlam, operator):
    """one iterate of Lambda_continuum in sweep order (k_continuum_update_native) and in rows (k_continuum_update): S, J and
    the scalar bit for bit, and both are the model's on the session's own J -- all entries thick, all thick with
    eps_thick < 0 (a counted padding wavelength would be thick too, and its 0 / 0 a NaN), and with the one thick entry at
    every site in turn, at the first and at the last wavelength: the scalar is that entry's term.  (The session returns no
    thick count: it refuses a case without a thick entry, before the device is touched.)"""
    grid = grids(n)
    kind = "continuum_ali" if operator else "continuum"
    alpha, eps, B0 = _continuum_case(grid, nlam, 10 * n + nlam)
    diag = vrt.lambda_diagonal(grid.sites, alpha, QUAD) if operator else None

    def one_iterate(eps_, eps_thick, native):
        case = vrt.ContinuumCase(alpha, eps_, B0, eps_thick)
        J, S, hist = vrt.Lambda_continuum(0.0, 1, grid.sites, case, QUAD, native=native, operator=operator)
        return J, S, hist[0]

    J = None
    for eps_thick in (1e-4, -1.0):
        Jn, Sn, dn = one_iterate(eps, eps_thick, True)
        Jr, Sr, dr = one_iterate(eps, eps_thick, False)
        assert same(Jn, Jr).all() and same(Sn, Sr).all() and same_scalar(dn, dr)
        want = R.update_model(kind, Jn, B0, eps, B0, diag=diag, eps_thick=eps_thick)
        assert same(Sn, want.S_new).all() and same_scalar(dn, want.scalar) and want.third == n * nlam
        J = Jn
    for site in range(n):
        for l in {0, nlam - 1}:
            e = eps.copy()
            e[site, l] = 0.9
            _, S, d = one_iterate(e, R.ONLY_THICK, True)
            want = R.update_model(kind, J, B0, e, B0, diag=diag, eps_thick=R.ONLY_THICK)
            one = R.update_model(kind, J[site:site + 1, l:l + 1], B0[site:site + 1, l:l + 1], e[site:site + 1, l:l + 1],
                                 B0[site:site + 1, l:l + 1], diag=None if diag is None else diag[site:site + 1, l:l + 1],
                                 eps_thick=R.ONLY_THICK)
            assert want.third == 1 and same_scalar(d, one.scalar) and same_scalar(d, want.scalar), (site, l, d, one.scalar)
            assert same(S, want.S_new).all(), (site, l)


# ---- 6: k_ali_min_den, reached through vrt_continuum_set_operator alone -------------------------------------------------
class _Continuum:
    """vrt_continuum_* through ctypes on a grid's quadrature plan"""

    def __init__(self, grid, alpha, eps, B0, eps_thick=1e-4):
        self.L, self.case = _lib.load(), vrt.ContinuumCase(alpha, eps, B0, eps_thick)
        self.cc, self.h = self.case.c_struct(), ctypes.c_void_p()
        _lib.check(self.L.vrt_continuum_create(grid.plan._h, ctypes.byref(self.cc), grid.w.ctypes.data_as(_lib.p_dbl),
                                               ctypes.byref(self.h)))

    def set_operator(self, op):
        return self.L.vrt_continuum_set_operator(self.h, op)

    def operator(self):
        op = ctypes.c_int(-1)
        assert self.L.vrt_continuum_get_operator(self.h, ctypes.byref(op), None) == 0
        return op.value

    def iterate(self):
        d = ctypes.c_double()
        _lib.check(self.L.vrt_continuum_iterate(self.h, ctypes.byref(d)))
        return d.value

    def close(self):
        if self.h:
            self.L.vrt_continuum_destroy(self.h)
            self.h = ctypes.c_void_p()


@pytest.mark.parametrize("n", [65, 257])
def test_min_den_is_seen_at_every_seam(grids, n):
    """α = 1e17 makes Λ* (vrt_plan_lambda_diagonal) round to 1 or above at most entries; with ε = 1/2 everywhere the
    operator is accepted, with ε = 0 at ONE entry whose Λ* >= 1 -- exactly one den <= 0 -- vrt_continuum_set_operator
    returns VRT_EINVAL and the session stays as it was.  That entry is moved over the seams of the n nlam threads of
    k_ali_min_den: a seam is a thread index, so the wavelength count (1 ... 5) is chosen per seam such that the entry
    there has Λ* >= 1; every seam must be reached with one of them."""
    grid = grids(n)
    reached, names = set(), set()
    for nlam in (1, 2, 3, 4, 5):
        alpha, B0 = np.full((n, nlam), 1e17), np.ones((n, nlam))
        diag = vrt.lambda_diagonal(grid.sites, alpha, QUAD)
        ok_eps = np.full((n, nlam), 0.5)
        assert R.min_den_model(ok_eps, diag) == (float((1.0 - 0.5 * diag).min()), False)
        s = _Continuum(grid, alpha, ok_eps, B0)
        try:
            assert s.set_operator(1) == 0 and s.operator() == 1
            assert s.set_operator(0) == 0
            d_plain = s.iterate()
        finally:
            s.close()
        for name, site, l in R.seam_cases(n, nlam, R.launch_of("continuum_ali", "rows")):
            names.add(name)
            if name in reached or not diag[site, l] >= 1.0:
                continue
            eps = ok_eps.copy()
            eps[site, l] = 0.0
            lo, bad = R.min_den_model(eps, diag)
            assert bad and lo > 0 and int((1.0 - (1.0 - eps) * diag <= 0).sum()) == 1
            s = _Continuum(grid, alpha, eps, B0)
            try:
                assert s.set_operator(1) == _lib.VRT_EINVAL, (n, nlam, name, site, l)
                assert b"Lambda*" in s.L.vrt_last_error()
                assert s.operator() == 0                        # unchanged: still the plain session
                d = s.iterate()
                assert np.isfinite(d) or np.isnan(d)
            finally:
                s.close()
            reached.add(name)
        del d_plain
    print(f"{n} sites: seams reached {sorted(reached)}")
    assert reached == names
