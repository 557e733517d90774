"""GPU tests (-m gpu) of every layout change between the caller's (n, ld) rows and the sweep-order plane sets
(voronoirt_amd/csrc/vrt_layout_kernels.h) over the shapes that decide which form runs: wavelength counts either side of
the narrow/wide switch (16) and of the second tile row (64), odd counts (a pad wavelength), pair blocks of 1 ... 16 with
ragged remainder blocks, a leading dimension wider than the row, and a site count that is no multiple of the 64-site tile.

The model is oracle/layout_ref.py (tests/test_layout_host.py checks the model itself).  The layout changes are pure
data movement plus one addition, so every comparison is BIT FOR BIT: the pure movements carry random bit patterns (NaN
payloads, -0, infinities, subnormals) and are compared as integers; every output starts as a sentinel pattern that no
input holds, so a value that was never written, or written where it does not belong, shows.

(a)-(d) the public entries (always the 64 x 64 tile kernels) against the model; (e) the internal forms -- the narrow
kernels, k_chain_prepare, the boundary kernel -- against the public ones through two routes to the same J, and the
caller-layout per-angle alpha against the native one; (f) every pair block and every layer path against the CPU oracle."""
import os

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import layout_ref as lr
from oracle import oracle as orc
from oracle.f32_model import PATH_MODEL, draw_case, within_conditions
from oracle.parity import rel as _rel
from voronoirt_amd import _lib

pytestmark = pytest.mark.gpu

RTOL = 1e-10
W, TH, PH, NQ = vrt.read_quadrature("ul7n12.dat")
DIRS = [1 if t > 90 else -1 for t in TH]
GRIDS = ["voro_small", "bcc_small"]
NLAMS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 129]
NLAMS_E = [1, 2, 3, 4, 15, 16, 17, 64, 65, 129]
NLAMS_F = [17, 65, 129]
# the plans: VRT_PAIR_BLOCK 1 ... 16, and the float layout of one pair per block (VRT_PATCH_QUAD=0); the options are read
# when the plan is created.  (pairs per block of the double layout, of the float layout)
PLANS = {"b1": ({"VRT_PAIR_BLOCK": "1"}, 1, 2), "b2": ({"VRT_PAIR_BLOCK": "2"}, 2, 2), "b4": ({"VRT_PAIR_BLOCK": "4"}, 4, 4),
         "b8": ({"VRT_PAIR_BLOCK": "8"}, 8, 8), "b16": ({"VRT_PAIR_BLOCK": "16"}, 16, 16),
         "b1q0": ({"VRT_PAIR_BLOCK": "1", "VRT_PATCH_QUAD": "0"}, 1, 1)}
BLOCK_PLANS = ["b1", "b2", "b4", "b8", "b16"]
# every layout the sweep-order S and J entries serve: doubles need one pair per block, floats run in every float layout
NATIVE_LAYOUTS = [("b1", False), ("b1q0", True), ("b1", True), ("b4", True), ("b8", True), ("b16", True)]
KEPT_OUT = ("VRT_PATH", "VRT_PAIR_BLOCK", "VRT_PATCH_QUAD", "VRT_PATCH_CHAIN", "VRT_STEP_STREAMS", "VRT_STEP_GROUP_DIR", "VRT_PATCH_SPLIT")

NP = {False: (np.dtype(np.float64), np.int64, np.uint64), True: (np.dtype(np.float32), np.int32, np.uint32)}
# sentinels: signalling-NaN patterns (positive as signed integers) that the random inputs are kept clear of
SENT = {False: 0x7FF45EA71E550BAD, True: 0x7FA5E17B}
OTHER = {False: 0x7FF4000000000BAD, True: 0x7FA00BAD}            # a second signalling pattern for the columns nobody reads
SPECIAL = {False: [0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF4000000000001, 0xFFF8000000ABCDEF,
                   0x0000000000000001, 0x800FFFFFFFFFFFFF, 0],
           True: [0x80000000, 0x7F800000, 0xFF800000, 0x7FA00001, 0xFFC0ABCD, 0x00000001, 0x807FFFFF, 0]}


def _make_plan(hs, env, dirs=DIRS, k=None):
    """a plan created under `env` (and none of the options that shape a plan); the environment is put back"""
    names = set(KEPT_OUT) | set(env)
    old = {name: os.environ.get(name) for name in names}
    for name in names:
        os.environ.pop(name, None)
    os.environ.update(env)
    try:
        return vrt.FormalPlan(hs, vrt.quadrature_directions(TH, PH) if k is None else k, 3, dirs=dirs)
    finally:
        for name, v in old.items():
            os.environ.pop(name, None) if v is None else os.environ.__setitem__(name, v)


class _Grid:
    def __init__(self, name, pos, nbr, bounds):
        self.name = name
        self.hs = vrt.VoronoiSites(pos, nbr, bounds, device=0)
        self.so = orc.make_sites(pos, nbr, bounds)
        self.n = self.hs.n
        self.order = {1: self.hs.storage_order(1) - 1, -1: self.hs.storage_order(-1) - 1}      # 0-based site per position
        for o in self.order.values():
            assert np.array_equal(np.sort(o), np.arange(self.n))
        self.plans = {}

    def plan(self, key):
        if key not in self.plans:
            env, B64, B32 = PLANS[key]
            self.plans[key] = p = _make_plan(self.hs, env)
            assert p.native_pair_block == B64 and p.native_pair_block_f32 == B32, (key, p.native_pair_block, p.native_pair_block_f32)
        return self.plans[key]

    def block(self, key, f32):
        return PLANS[key][2 if f32 else 1]

    def close(self):
        self.hs.close()            # (closes every plan of the grid)


@pytest.fixture(scope="module")
def grids(voro_small, bcc_small):
    made = {"voro_small": _Grid("voro_small", *voro_small), "bcc_small": _Grid("bcc_small", *bcc_small)}
    # a partial last tile of 64 sites and more than one workgroup of the 256-thread forms
    assert any(g.n % 64 != 0 and g.n > 256 for g in made.values()), [g.n for g in made.values()]
    yield made
    for g in made.values():
        g.close()


# ---- device buffers as integers ---------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch, torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream


def _up(a, f32):
    """numpy array (floats or their unsigned patterns) -> device tensor of the signed integers of the same width"""
    torch, dev, _ = _torch()
    return torch.from_numpy(np.array(a, order="C").view(NP[f32][1])).to(dev)         # (a copy: the shared cases are read-only)


def _sentinel(shape, f32):
    torch, dev, _ = _torch()
    return torch.full(shape, SENT[f32], dtype=torch.int32 if f32 else torch.int64, device=dev)


def _down(t, f32):
    """device tensor -> the unsigned bit patterns"""
    return t.cpu().numpy().view(NP[f32][2])


def _bits(a, f32):
    return np.ascontiguousarray(a, dtype=NP[f32][0]).view(NP[f32][2])


def _random_bits(rng, shape, f32):
    """uniform bit patterns with every special among them, none of them a sentinel"""
    u = NP[f32][2]
    a = rng.integers(0, np.iinfo(u).max, shape, dtype=u, endpoint=True)
    flat = a.reshape(-1)
    at = rng.choice(flat.size, size=min(flat.size, len(SPECIAL[f32])), replace=False)
    flat[at] = np.array(SPECIAL[f32], dtype=u)[:at.size]
    flat[(flat == SENT[f32]) | (flat == OTHER[f32])] ^= u(1)
    return a


def _rows(rng, n, nlam, ld, f32, fill=None):
    """(n, ld) caller rows: random patterns in the nlam columns, a signalling pattern in the rest"""
    a = np.full((n, ld), OTHER[f32] if fill is None else fill, dtype=NP[f32][2])
    a[:, :nlam] = _random_bits(rng, (n, nlam), f32)
    return a


def _pad_indices(n, nlam, B):
    npair = (nlam + 1) // 2
    return 2 * lr.pair_index(npair - 1, np.arange(n), n, B, npair) + 1


def _form(nlam):
    return f"tile form, {(nlam + 63) // 64} tile row(s)"


# ---- (a) caller rows -> plane sets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlam", NLAMS)
@pytest.mark.parametrize("key, f32", NATIVE_LAYOUTS)
@pytest.mark.parametrize("grid", GRIDS)
def test_to_native_is_the_model(grids, grid, key, f32, nlam):
    g = grids[grid]
    plan, B, n = g.plan(key), g.block(key, f32), g.n
    dt, _, u = NP[f32]
    _, _, st = _torch()
    cnt = plan.native_plane_count(nlam)
    assert cnt == 2 * ((nlam + 1) // 2) * n
    rng = np.random.default_rng(1000 * nlam + 10 * B + f32)
    for ld in (nlam, nlam + 3):
        rows = _rows(rng, n, nlam, ld, f32)
        want = {d: lr.to_planes(rows[:, :nlam].view(dt), g.order[d], B, dt).view(u) for d in (1, -1)}
        d_in = _up(rows, f32)
        got = {}
        for call in ("up", "down", "both"):
            out = {1: _sentinel((cnt,), f32), -1: _sentinel((cnt,), f32)}
            plan.to_native_dev(nlam, ld, d_in.data_ptr(), out[1].data_ptr() if call != "down" else 0,
                               out[-1].data_ptr() if call != "up" else 0, stream=st, f32=f32)
            for d in (1, -1):
                h = _down(out[d], f32)
                if (call == "up" and d == -1) or (call == "down" and d == 1):
                    assert (h == SENT[f32]).all(), (grid, key, f32, nlam, ld, call, d)
                    continue
                assert not (h == SENT[f32]).any(), (grid, key, f32, nlam, ld, call, d, int((h == SENT[f32]).sum()))
                assert np.array_equal(h, want[d]), (grid, key, f32, nlam, ld, call, d, int((h != want[d]).sum()))
                if nlam & 1:
                    assert not h[_pad_indices(n, nlam, B)].any(), (grid, key, f32, nlam, ld, call, d)
                got[d] = h
        if ld > nlam:               # the columns nlam ... ld-1 are never read: other patterns there, the same planes
            rows[:, nlam:] = _random_bits(rng, (n, ld - nlam), f32)
            out = {1: _sentinel((cnt,), f32), -1: _sentinel((cnt,), f32)}
            plan.to_native_dev(nlam, ld, _up(rows, f32).data_ptr(), out[1].data_ptr(), out[-1].data_ptr(), stream=st, f32=f32)
            for d in (1, -1):
                assert np.array_equal(_down(out[d], f32), got[d]), (grid, key, f32, nlam, ld, d)
    print(f"{grid} {key} {'f32' if f32 else 'f64'} nlam {nlam}: blocks {lr.block_widths((nlam + 1) // 2, B)}, {_form(nlam)}")


# ---- (b) plane sets -> caller rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlam", NLAMS)
@pytest.mark.parametrize("key, f32", NATIVE_LAYOUTS)
@pytest.mark.parametrize("grid", GRIDS)
def test_from_native_is_the_model_and_the_round_trip_is_exact(grids, grid, key, f32, nlam):
    g = grids[grid]
    plan, B, n = g.plan(key), g.block(key, f32), g.n
    dt, _, u = NP[f32]
    _, _, st = _torch()
    cnt = plan.native_plane_count(nlam)
    rng = np.random.default_rng(2000 * nlam + 10 * B + f32)
    for ld in (nlam, nlam + 3):
        for d in (1, -1):
            planes = _random_bits(rng, (cnt,), f32)
            out = _sentinel((n, ld), f32)
            plan.from_native_dev(d, nlam, ld, _up(planes, f32).data_ptr(), out.data_ptr(), stream=st, f32=f32)
            h = _down(out, f32)
            want = lr.from_planes(planes.view(dt), g.order[d], nlam, B).view(u)
            assert np.array_equal(h[:, :nlam], want), (grid, key, f32, nlam, ld, d, int((h[:, :nlam] != want).sum()))
            assert (h[:, nlam:] == SENT[f32]).all(), (grid, key, f32, nlam, ld, d)
            # from(to(x)) == x
            rows = _rows(rng, n, nlam, ld, f32)
            mid, back = _sentinel((cnt,), f32), _sentinel((n, ld), f32)
            plan.to_native_dev(nlam, ld, _up(rows, f32).data_ptr(), mid.data_ptr() if d > 0 else 0, mid.data_ptr() if d < 0 else 0,
                               stream=st, f32=f32)
            plan.from_native_dev(d, nlam, ld, mid.data_ptr(), back.data_ptr(), stream=st, f32=f32)
            h = _down(back, f32)
            assert np.array_equal(h[:, :nlam], rows[:, :nlam]) and (h[:, nlam:] == SENT[f32]).all(), (grid, key, f32, nlam, ld, d)
    print(f"{grid} {key} {'f32' if f32 else 'f64'} nlam {nlam}: blocks {lr.block_widths((nlam + 1) // 2, B)}, {_form(nlam)}")


# ---- (c) J = J_up + J_down --------------------------------------------------------------------------------------------------
def _J_rows(rng, n, nlam, f32):
    """finite values of both signs over the format's decades, with -0, +-inf and a NaN at known places"""
    dt = NP[f32][0]
    span = 30 if f32 else 300
    a = (rng.standard_normal((n, nlam)) * 10.0 ** rng.uniform(-span, span, (n, nlam))).astype(dt)
    b = (rng.standard_normal((n, nlam)) * 10.0 ** rng.uniform(-span, span, (n, nlam))).astype(dt)
    b[n // 2:] = -a[n // 2:] * dt.type(1 + 2.0 ** -20)              # near cancellation: the sum is a few ulps of a
    l = nlam - 1
    a[0, 0], b[0, 0] = -0.0, -0.0                                   # -0 + -0 = -0
    a[1, l], b[1, l] = -0.0, 0.0                                    # -0 + +0 = +0
    a[2, 0], b[2, 0] = np.inf, -np.inf                              # NaN
    a[3, l], b[3, l] = np.inf, 1.0
    a[4, 0], b[4, 0] = -np.inf, -np.inf
    a[5, l], b[5, l] = -0.0, 3.0
    a[6, 0], b[6, 0] = 2.0, -0.0
    a[7, l], b[8, 0] = np.nan, np.nan
    return a, b


@pytest.mark.parametrize("nlam", NLAMS)
@pytest.mark.parametrize("key, f32", NATIVE_LAYOUTS)
@pytest.mark.parametrize("grid", GRIDS)
def test_J_from_native_is_the_model(grids, grid, key, f32, nlam):
    g = grids[grid]
    plan, B, n = g.plan(key), g.block(key, f32), g.n
    dt, _, u = NP[f32]
    _, _, st = _torch()
    rng = np.random.default_rng(3000 * nlam + 10 * B + f32)
    a, b = _J_rows(rng, n, nlam, f32)
    planes = {1: lr.to_planes(a, g.order[1], B, dt).view(u), -1: lr.to_planes(b, g.order[-1], B, dt).view(u)}
    if nlam & 1:                    # whatever the pad wavelength holds, it reaches no column of J
        for d in (1, -1):
            planes[d][_pad_indices(n, nlam, B)] = OTHER[f32]
    dev = {d: _up(planes[d], f32) for d in (1, -1)}
    for ld in (nlam, nlam + 3):
        for call in ("both", "up", "down"):
            Ju, Jd = (planes[1] if call != "down" else None), (planes[-1] if call != "up" else None)
            want = lr.combine(None if Ju is None else Ju.view(dt), None if Jd is None else Jd.view(dt), g.order[1], g.order[-1],
                              nlam, B, dt)
            out = _sentinel((n, ld), f32)
            plan.J_from_native_dev(nlam, ld, dev[1].data_ptr() if call != "down" else 0, dev[-1].data_ptr() if call != "up" else 0,
                                   out.data_ptr(), stream=st, f32=f32)
            h = _down(out, f32)
            got = np.ascontiguousarray(h[:, :nlam]).view(dt)
            nan = np.isnan(want)
            assert nan.any() and np.array_equal(np.isnan(got), nan), (grid, key, f32, nlam, ld, call)
            same = _bits(got, f32)[~nan] == _bits(want, f32)[~nan]
            assert same.all(), (grid, key, f32, nlam, ld, call, int((~same).sum()))
            assert (h[:, nlam:] == SENT[f32]).all(), (grid, key, f32, nlam, ld, call)
    print(f"{grid} {key} {'f32' if f32 else 'f64'} nlam {nlam}: blocks {lr.block_widths((nlam + 1) // 2, B)}, {_form(nlam)}")


# ---- (d) per-angle alpha -> the native buffer -------------------------------------------------------------------------------
@pytest.mark.parametrize("nlam", NLAMS)
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("key", BLOCK_PLANS + ["b1q0"])
@pytest.mark.parametrize("grid", GRIDS)
def test_alpha_to_native_is_the_model(grids, grid, key, f32, nlam):
    g = grids[grid]
    plan, B, n = g.plan(key), g.block(key, f32), g.n
    dt, _, u = NP[f32]
    _, _, st = _torch()
    cnt = plan.native_alpha_count(nlam)
    assert cnt == NQ * 2 * ((nlam + 1) // 2) * n
    rng = np.random.default_rng(4000 * nlam + 10 * B + f32)
    for ld in (nlam, nlam + 3):
        al = np.full((NQ, n, ld), OTHER[f32], dtype=u)
        al[:, :, :nlam] = _random_bits(rng, (NQ, n, nlam), f32)
        want = lr.alpha_native(al[:, :, :nlam].view(dt), [g.order[d] for d in DIRS], B, dt).view(u)
        out = _sentinel((cnt,), f32)
        plan.alpha_to_native_dev(nlam, ld, _up(al, f32).data_ptr(), out.data_ptr(), stream=st, f32=f32)
        h = _down(out, f32)
        assert not (h == SENT[f32]).any(), (grid, key, f32, nlam, ld, int((h == SENT[f32]).sum()))
        assert np.array_equal(h, want), (grid, key, f32, nlam, ld, int((h != want).sum()))
    print(f"{grid} {key} {'f32' if f32 else 'f64'} nlam {nlam}: blocks {lr.block_widths((nlam + 1) // 2, B)}, {_form(nlam)}")


# ---- (e) the internal forms against the public ones -------------------------------------------------------------------------
_cases = {}


def _case(g, nlam, per_angle=False):
    """float32-valued S, alpha, I_0 of both directions (oracle/f32_model.py: draw_case), once per shape and read-only"""
    key = (g.name, nlam, per_angle)
    if key not in _cases:
        _cases[key] = draw_case(g.so, nlam, n_angles=NQ if per_angle else 0, seed=100 + nlam)
        for a in _cases[key]:
            a.setflags(write=False)
    return _cases[key]


def _wide(a, ld, f32):
    """the last axis widened to ld columns, a signalling pattern in the added ones, as integers on the device"""
    dt, _, u = NP[f32]
    out = np.full(a.shape[:-1] + (ld,), OTHER[f32], dtype=u)
    out[..., :a.shape[-1]] = np.ascontiguousarray(a, dtype=dt).view(u)
    return _up(out, f32)


def _which(plan, nlam, lb, f64_site_lam=False):
    """the form of the execute's own layout changes, read off the shape as LayerRun does (csrc/vrt_layers.hip), and the
    launch count the plan reports; f64_site_lam: doubles, one pair per block, alpha per (site, wavelength) -- a CHAINED step
    of one or two pairs then prepares everything in k_chain_prepare (vrt_patch.cpp: patch_shape, VRT_CHAIN_DATAFLAG unset)"""
    launches = plan.last_launches
    form = "narrow" if lb != 1 and nlam <= 16 else "tiles"
    if f64_site_lam and lb == 2 and launches == 1 and nlam <= 4:
        form = "prepare"
    return launches, f"{form} layout changes, {launches} sweep launch(es){' (chained)' if launches == 1 else ''}"


@pytest.mark.parametrize("nlam", NLAMS_E)
@pytest.mark.parametrize("storage, chain", [("f64", 1), ("f64", 0), ("f32", 1)])
@pytest.mark.parametrize("grid", GRIDS)
def test_caller_layout_execute_is_the_sweep_order_execute(grids, grid, storage, chain, nlam):
    """execute_dev lays S and alpha out itself (nlam <= 16: the narrow kernels, or k_chain_prepare for a chained step of
    one or two pairs; the boundary kernel otherwise) and combines J itself; to_native_dev -> execute_native_dev ->
    J_from_native_dev runs the tile kernels around the same sweep.  One J, bit for bit."""
    g = grids[grid]
    f32, n = storage == "f32", g.n
    _, _, st = _torch()
    S, al, I0u, I0d = _case(g, nlam)
    plan = _make_plan(g.hs, PLANS["b1"][0])
    try:
        plan.set_option("VRT_PATCH_CHAIN", chain)
        ld = nlam + 3
        dS, dA, dU, dD = _wide(S, ld, f32), _wide(al, ld, f32), _up(np.asarray(I0u, NP[f32][0]), f32), _up(np.asarray(I0d, NP[f32][0]), f32)
        J1 = _sentinel((n, ld), f32)
        plan.execute_dev(nlam, ld, dS.data_ptr(), dA.data_ptr(), _lib.ALPHA_SITE_LAM, W, dJ=J1.data_ptr(), dI0_up=dU.data_ptr(),
                         dI0_down=dD.data_ptr(), stream=st, f32=f32)
        h1 = _down(J1, f32)
        plan.check()
        assert plan.last_path == "patches"
        launches, text = _which(plan, nlam, 2 * plan.native_pair_block_f32 if f32 else 2, f64_site_lam=not f32)
        cnt = plan.native_plane_count(nlam)
        size = 4 if f32 else 8
        Sn, An, Jn = (_sentinel((2 * cnt,), f32) for _ in range(3))
        plan.to_native_dev(nlam, ld, dS.data_ptr(), Sn.data_ptr(), Sn.data_ptr() + size * cnt, stream=st, f32=f32)
        plan.to_native_dev(nlam, ld, dA.data_ptr(), An.data_ptr(), An.data_ptr() + size * cnt, stream=st, f32=f32)
        plan.execute_native_dev(nlam, Sn.data_ptr(), Sn.data_ptr() + size * cnt, An.data_ptr(), _lib.ALPHA_SITE_LAM_NATIVE, W,
                                dJ_up=Jn.data_ptr(), dJ_down=Jn.data_ptr() + size * cnt, dI0_up=dU.data_ptr(), dI0_down=dD.data_ptr(),
                                stream=st, f32=f32)
        J2 = _sentinel((n, ld), f32)
        plan.J_from_native_dev(nlam, ld, Jn.data_ptr(), Jn.data_ptr() + size * cnt, J2.data_ptr(), stream=st, f32=f32)
        h2 = _down(J2, f32)
        plan.check()
        assert plan.last_path == "patches"
    finally:
        plan.close()
    print(f"{grid} {storage} chain {chain} nlam {nlam}: {text}")
    for h in (h1, h2):
        assert (h[:, nlam:] == SENT[f32]).all() and not (h[:, :nlam] == SENT[f32]).any()
    J = np.ascontiguousarray(h1[:, :nlam]).view(NP[f32][0])
    assert np.isfinite(J).all() and (J > 0).all()
    assert np.array_equal(h1, h2), (grid, storage, chain, nlam, int((h1 != h2).sum()))


@pytest.mark.parametrize("nlam", NLAMS_E)
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("key", BLOCK_PLANS)
@pytest.mark.parametrize("grid", GRIDS)
def test_caller_layout_per_angle_alpha_is_the_native_one(grids, grid, key, f32, nlam):
    """ALPHA_ANGLE_SITE_LAM (laid out inside the execute) against ALPHA_ANGLE_NATIVE fed by alpha_to_native_dev: J and every
    I_out bit for bit, in every pair block."""
    g = grids[grid]
    plan, n = g.plan(key), g.n
    _, _, st = _torch()
    S, al, I0u, I0d = _case(g, nlam, per_angle=True)
    ld = nlam + 3
    dS, dA, dU, dD = _wide(S, ld, f32), _wide(al, ld, f32), _up(np.asarray(I0u, NP[f32][0]), f32), _up(np.asarray(I0d, NP[f32][0]), f32)
    nat = _sentinel((plan.native_alpha_count(nlam),), f32)
    plan.alpha_to_native_dev(nlam, ld, dA.data_ptr(), nat.data_ptr(), stream=st, f32=f32)
    res = []
    for alpha, mode in ((dA, _lib.ALPHA_ANGLE_SITE_LAM), (nat, _lib.ALPHA_ANGLE_NATIVE)):
        J, I = _sentinel((n, ld), f32), _sentinel((NQ, n, ld), f32)
        plan.execute_dev(nlam, ld, dS.data_ptr(), alpha.data_ptr(), mode, W, dJ=J.data_ptr(), dI0_up=dU.data_ptr(),
                         dI0_down=dD.data_ptr(), dI_out=I.data_ptr(), stream=st, f32=f32)
        res.append((_down(J, f32), _down(I, f32)))
        plan.check()
        assert plan.last_path == "patches"
    _, text = _which(plan, nlam, 2 * g.block(key, f32))
    print(f"{grid} {key} {'f32' if f32 else 'f64'} nlam {nlam}: {text}")
    (J1, I1), (J2, I2) = res
    for h in (J1, I1, J2, I2):
        assert (h[..., nlam:] == SENT[f32]).all() and not (h[..., :nlam] == SENT[f32]).any()
    Jv = np.ascontiguousarray(J1[:, :nlam]).view(NP[f32][0])
    assert np.isfinite(Jv).all() and (Jv > 0).all()
    assert np.array_equal(J1, J2), (grid, key, f32, nlam, int((J1 != J2).sum()))
    assert np.array_equal(I1, I2), (grid, key, f32, nlam, int((I1 != I2).sum()))


# ---- (f) every block and path against the oracle ----------------------------------------------------------------------------
_refs = {}


def _reference(g, nlam, f32, theta=None):
    """(J, I, J_up, J_down) of the oracle for _case(g, nlam): the plain fp64 oracle, or the storage model of the patch
    path for float storage; once per shape and read-only"""
    key = (g.name, nlam, f32, theta is not None)
    if key not in _refs:
        S, al, I0u, I0d = _case(g, nlam)
        f = lambda a: np.asarray(a, dtype=np.float64)
        model = PATH_MODEL["patches"] if f32 else {}
        out = orc.J_voronoi_model(W, TH if theta is None else theta, PH, f(S), f(al), g.so, I0_up=f(I0u), I0_down=f(I0d), nthreads=8, **model)
        for a in out:
            a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def _execute(g, plan, nlam, f32):
    """J and I_out of execute_dev for _case(g, nlam), ld = nlam + 3, as bit patterns (n, ld) and (NQ, n, ld)"""
    _, _, st = _torch()
    S, al, I0u, I0d = _case(g, nlam)
    ld = nlam + 3
    dS, dA, dU, dD = _wide(S, ld, f32), _wide(al, ld, f32), _up(np.asarray(I0u, NP[f32][0]), f32), _up(np.asarray(I0d, NP[f32][0]), f32)
    J, I = _sentinel((g.n, ld), f32), _sentinel((NQ, g.n, ld), f32)
    plan.execute_dev(nlam, ld, dS.data_ptr(), dA.data_ptr(), _lib.ALPHA_SITE_LAM, W, dJ=J.data_ptr(), dI0_up=dU.data_ptr(),
                     dI0_down=dD.data_ptr(), dI_out=I.data_ptr(), stream=st, f32=f32)
    hJ, hI = _down(J, f32), _down(I, f32)
    plan.check()
    return hJ, hI


def _against_oracle(label, g, nlam, f32, hJ, hI, ref, dirs):
    dt = NP[f32][0]
    S, al, I0u, I0d = _case(g, nlam)
    Jr, Ir = ref[0], ref[1]
    assert (hJ[:, nlam:] == SENT[f32]).all() and (hI[..., nlam:] == SENT[f32]).all(), label
    J, I = np.ascontiguousarray(hJ[:, :nlam]).view(dt), np.ascontiguousarray(hI[..., :nlam]).view(dt)
    for name, got, want in [("J", J, Jr)] + [(f"I[{a}]", I[a], Ir[a]) for a in range(NQ)]:
        if f32:
            ok, ndiff, size, ulps = within_conditions(got, want)
            print(f"{label} {name}: {ndiff} of {size} floats differ from the model, at most {ulps:g} ulp")
            assert ok, (label, name, ndiff, size, ulps)
        else:
            err = _rel(got, want)
            print(f"{label} {name}: element-wise relative error {float(err):.2e}")
            assert err < RTOL, (label, name, float(err))
    for a in range(NQ):
        if dirs[a] == 0:            # a theta = 90 angle is skipped: zeros in every wavelength column
            assert not hI[a, :, :nlam].any() and not Ir[a].any(), (label, a)
            continue
        perm, layers, I0 = (g.so.perm_up, g.so.layers_up, I0u) if dirs[a] > 0 else (g.so.perm_down, g.so.layers_down, I0d)
        # the never-visited last site of the direction keeps I = 0
        assert not hI[a, perm[-1] - 1, :nlam].any() and not Ir[a, perm[-1] - 1].any(), (label, a)
        # the boundary layer: where the oracle's I is I_0 bit for bit, so is the device's
        first = perm[:layers[1] - 1] - 1
        want0 = _bits(I0, f32)
        kept = _bits(Ir[a, first], f32) == want0
        assert kept.any(), (label, a)
        assert (_bits(I[a, first], f32)[kept] == want0[kept]).all(), (label, a)


@pytest.mark.parametrize("nlam", NLAMS_F)
@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("block", [1, 4, 16])
@pytest.mark.parametrize("grid", GRIDS)
def test_every_pair_block_of_the_patch_path_is_the_oracle(grids, grid, block, storage, nlam):
    g, f32 = grids[grid], storage == "f32"
    key = {1: "b1q0" if f32 else "b1", 4: "b4", 16: "b16"}[block]
    plan = g.plan(key)
    assert g.block(key, f32) == block
    hJ, hI = _execute(g, plan, nlam, f32)
    assert plan.last_path == "patches"
    label = f"{grid} patches block {block} {storage} nlam {nlam}"
    print(f"{label}: {_which(plan, nlam, 2 * block, f64_site_lam=not f32)[1]}, blocks {lr.block_widths((nlam + 1) // 2, block)}")
    _against_oracle(label, g, nlam, f32, hJ, hI, _reference(g, nlam, f32), DIRS)


@pytest.mark.parametrize("nlam", NLAMS_F)
@pytest.mark.parametrize("path, lb", [("steps", 2), ("tiles", 1)])
@pytest.mark.parametrize("grid", GRIDS)
def test_the_steps_and_tiles_paths_are_the_oracle(grids, grid, path, lb, nlam):
    """VRT_PATH=steps: wavelength pairs, one per block (lb = 2); VRT_PATH=tiles: plain planes (lb = 1)"""
    g = grids[grid]
    plan = _make_plan(g.hs, PLANS["b1"][0])
    try:
        plan.set_option("VRT_PATH", path)
        hJ, hI = _execute(g, plan, nlam, False)
        assert plan.last_path == path
        label = f"{grid} {path} (lb = {lb}) f64 nlam {nlam}"
        print(f"{label}: {_which(plan, nlam, lb)[1]}")
    finally:
        plan.close()
    _against_oracle(label, g, nlam, False, hJ, hI, _reference(g, nlam, False), DIRS)


@pytest.mark.parametrize("nlam", NLAMS_F)
@pytest.mark.parametrize("grid", GRIDS)
def test_a_skipped_angle_comes_back_as_zeros(grids, grid, nlam):
    """A theta = 90 angle in the plan (dirs entry 0) is never swept: its I_out is zeros in the nlam columns, the padding
    columns keep what they held, and J is the oracle's without that angle."""
    g = grids[grid]
    skipped = 4
    theta, dirs = np.array(TH, dtype=np.float64), list(DIRS)
    theta[skipped], dirs[skipped] = 90.0, 0
    plan = _make_plan(g.hs, PLANS["b1"][0], dirs=dirs, k=vrt.quadrature_directions(theta, PH))
    try:
        hJ, hI = _execute(g, plan, nlam, False)
        assert plan.last_path == "patches"
        label = f"{grid} angle {skipped} skipped f64 nlam {nlam}"
        print(f"{label}: {_which(plan, nlam, 2, f64_site_lam=True)[1]}")
    finally:
        plan.close()
    assert not hI[skipped, :, :nlam].any() and (hI[skipped, :, nlam:] == SENT[False]).all()
    _against_oracle(label, g, nlam, False, hJ, hI, _reference(g, nlam, False, theta=theta), dirs)
