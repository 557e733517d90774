"""The plan-time kernels k_delaunay_lines and k_upwind_table (csrc/vrt_kernels.hip) at their decision points, against the
CPU oracle: bit-equal dot products inside a chunk and across chunks, equal slot-2 candidates, dots of exactly 0.0 and
-1.0, the collapse on D2 == 0, the periodic test on its equality and its MIRROR branch, rows of 1 to 4 chunks inside one
wave, the clamped tail of the last wave, wall slots inside a chunk, NaN lines.  The grids and the 64 directions are built
and shown to hold these cases in tests/test_upwind_domain_host.py; ids, dots, path lengths and lines are compared bit for
bit, the weights at the 1 ulp of pow() that test_upwind_table_bit_exact allows, intensities at the suite's 1e-10.
Figures are printed before they are asserted (profiles/upwind_domain/test_upwind_domain_figures.txt)."""
import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle.parity import rel as _rel
from test_upwind_domain_host import (CLASSES, GRIDS, ORDER_GRIDS, ORDER_SEEDS, SOLVE_GRIDS, class_masks, direction_arrays,
                                     directions, grids, lines_equal, oracle_J, oracle_sites, oracle_solves, oracle_tables,
                                     reshuffled, solve_directions, solve_problem, valid_line_mask)

pytestmark = pytest.mark.gpu

RTOL = 1e-10                                 # fp64 tolerance of the north star (tests/test_gpu_parity.py)
W_RTOL, W_ATOL = 4e-15, 1e-300               # pow(): ulp-level (test_upwind_table_bit_exact)


@pytest.fixture(scope="module")
def device_sites():
    """name -> VoronoiSites on the device, created on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = vrt.VoronoiSites(*grids()[name], device=0)
        return made[name]

    yield get
    for hs in made.values():
        hs.close()


def _same_bits(a, b):
    """array_equal with NaN positions as "both NaN\""""
    return lines_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def _check_lines(hs, so, what):
    for key in ("layers_up", "layers_down", "perm_up", "perm_down"):
        assert np.array_equal(getattr(hs, key), getattr(so, key)), (what, key)
    m = valid_line_mask(so)
    lines = hs.Delaunay_lines
    nan_o, nan_g = np.isnan(so.delaunay_lines[m]).any(axis=1), np.isnan(lines[m]).any(axis=1)
    differ = int((~((lines[m] == so.delaunay_lines[m]) | (np.isnan(lines[m]) & np.isnan(so.delaunay_lines[m]))).all(axis=1)).sum())
    print("lines, %-22s: %5d valid slots, %4d NaN lines (oracle %4d), %d slots differ" % (what, int(m.sum()), int(nan_g.sum()), int(nan_o.sum()), differ))
    assert lines_equal(lines[m], so.delaunay_lines[m]), what
    assert (lines[~m] == 0).all(), what


def _check_tables(plan, name, what, order_seed=None, angles=None):
    """every direction's table of `plan` against orc.upwind_table; returns the device tables"""
    ds = directions()
    tabs = oracle_tables(name, order_seed)
    masks = class_masks(name, order_seed)
    angles = range(len(ds)) if angles is None else angles
    got = {}
    id_bad = {c: 0 for c in CLASSES}
    held = {c: 0 for c in CLASSES}
    bad = {"ids": 0, "dots": 0, "r": 0, "w_nan": 0}
    worst_w = 0.0
    for j, a in enumerate(angles):
        up, dots, wt, r, st = tabs[a]
        g = plan.upwind(j)
        got[a] = g
        gup, gd, gw, gr = g
        wrong = (gup != up).any(axis=1)
        for c in CLASSES:
            held[c] += int(masks[a][c].sum())
            id_bad[c] += int((wrong & masks[a][c]).sum())
        bad["ids"] += int(wrong.sum())
        bad["dots"] += int((gd != dots).sum())
        bad["r"] += int((gr != r).sum())
        bad["w_nan"] += int((np.isnan(gw) != np.isnan(wt)).sum())
        fin = np.isfinite(wt) & np.isfinite(gw)
        if fin.any():
            worst_w = max(worst_w, float(np.abs(gw[fin] - wt[fin]).max()))
    for c in CLASSES:
        print("upwind, %-22s %-22s: %5d (direction, site) pairs hold it, ids differ at %d" % (what, c, held[c], id_bad[c]))
    print("upwind, %-22s %d directions x %d sites: ids differ %d, dots %d, path lengths %d, NaN weights misplaced %d, "
          "worst |w - w_oracle| %.3e" % (what, len(got), tabs[0][0].shape[0], bad["ids"], bad["dots"], bad["r"], bad["w_nan"], worst_w))
    for a, (gup, gd, gw, gr) in got.items():
        up, dots, wt, r, st = tabs[a]
        assert (st == 0).all()
        assert np.array_equal(gup, up), (what, ds[a], "upwind neighbour ids must be bit-exact")
        assert np.array_equal(gd, dots), (what, ds[a])
        assert np.array_equal(gr, r), (what, ds[a])
        assert np.array_equal(np.isnan(gw), np.isnan(wt)), (what, ds[a])              # 0 / 0 where the oracle has it
        assert np.allclose(gw, wt, rtol=W_RTOL, atol=W_ATOL, equal_nan=True), (what, ds[a])
    return got


@pytest.mark.parametrize("name", GRIDS)
def test_delaunay_lines_at_the_periodic_decisions(device_sites, name):
    """hs.Delaunay_lines equals the oracle's on valid slots bit for bit, NaN where the oracle has NaN (a mirrored or a
    coincident neighbour on the site itself); layers and permutations equal; the coincident grid is accepted as the
    oracle accepts it"""
    _check_lines(device_sites(name), oracle_sites(name), name)


@pytest.mark.parametrize("name", GRIDS)
def test_upwind_table_at_the_decision_points(device_sites, name):
    """One plan that carries all 64 directions, then plans of one direction and a plan of a few in another order: the
    table of a direction must not depend on what else the plan holds, bit for bit"""
    hs = device_sites(name)
    ks, dirs = direction_arrays()
    plan = vrt.FormalPlan(hs, ks, 3, dirs=dirs)
    got = _check_tables(plan, name, name)
    plan.close()
    ds = directions()
    alone = [a for a in range(len(ds)) if a % 5 == 0 or ds[a].label in ("-z", "+x", "zx--", "b---")]
    differ = 0
    for a in alone:
        one = vrt.FormalPlan(hs, [ks[a]], 3, dirs=[dirs[a]])
        t = one.upwind(0)
        one.close()
        differ += sum(0 if _same_bits(x, y) else 1 for x, y in zip(t, got[a]))
        assert all(_same_bits(x, y) for x, y in zip(t, got[a])), (name, ds[a], "alone and among 64")
    some = alone[::-1][:9]
    part = vrt.FormalPlan(hs, ks[some], 1, dirs=[dirs[a] for a in some])
    for j, a in enumerate(some):
        t = part.upwind(j)
        differ += sum(0 if _same_bits(x, y) else 1 for x, y in zip(t, got[a]))
        assert all(_same_bits(x, y) for x, y in zip(t, got[a])), (name, ds[a], "among 9 in another order")
    part.close()
    print("upwind, %-22s %d directions alone and %d in another plan: %d tables differ from the plan of 64" % (name, len(alone), len(some), differ))


@pytest.mark.parametrize("seed", ORDER_SEEDS)
@pytest.mark.parametrize("name", ORDER_GRIDS)
def test_row_order_is_followed_under_ties(name, seed):
    """every row reshuffled: under ties the oracle's choice changes with the order (counted), and the device follows"""
    pos, nbr, bounds = grids()[name]
    hs = vrt.VoronoiSites(pos, reshuffled(nbr, seed), bounds, device=0)
    so = oracle_sites(name, seed)
    what = "%s order %d" % (name, seed)
    _check_lines(hs, so, what)
    base = oracle_tables(name)
    tabs = oracle_tables(name, seed)
    changed = sum(int((tabs[a][0] != base[a][0]).any(axis=1).sum()) for a in range(len(tabs)))
    print("upwind, %-22s the oracle's ids differ from the first order's at %d (direction, site) pairs" % (what, changed))
    assert changed >= 100
    ks, dirs = direction_arrays()
    plan = vrt.FormalPlan(hs, ks, 3, dirs=dirs)
    _check_tables(plan, name, what, order_seed=seed)
    plan.close()
    hs.close()


#          name          VRT_PATH   environment read at plan creation
FORMS = (("levels",     "levels",  {}),
         ("steps",      "steps",   {}),
         ("tiles",      "tiles",   {}),
         ("per-layer",  "patches", {"VRT_PATCH_CHAIN": "0", "VRT_CHAIN_DATAFLAG": "0"}),
         ("chain",      "patches", {"VRT_PATCH_CHAIN": "1", "VRT_CHAIN_DATAFLAG": "0"}),
         ("chain-df",   "patches", {"VRT_PATCH_CHAIN": "1", "VRT_CHAIN_DATAFLAG": "1"}))
SETTINGS = ((1, 1), (1, 3), (3, 1), (3, 3))                                          # (nlam, n_sweeps)


def _solve_all_forms(name, monkeypatch):
    """{form: {(nlam, n_sweeps): (per-angle I of solve_directions(name), J over ul7n12)}}, every path asserted to have run"""
    hs = vrt.VoronoiSites(*grids()[name], device=0)
    ks, dirs = direction_arrays()
    sel = list(solve_directions(name))
    ks, dirs = ks[sel], [dirs[a] for a in sel]
    w, th, ph, _ = vrt.read_quadrature("ul7n12.dat")
    qk, qd = vrt.quadrature_directions(th, ph), [1 if t > 90 else -1 for t in th]
    monkeypatch.setenv("VRT_PATCH_OWN", "10")                 # several patches per layer of 20 to 50 sites
    out = {}
    for form, path, env in FORMS:
        monkeypatch.setenv("VRT_PATH", path)
        for k in ("VRT_PATCH_CHAIN", "VRT_CHAIN_DATAFLAG"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out[form] = {}
        for nlam, n_sweeps in SETTINGS:
            S, alpha, I0u, I0d = solve_problem(name, nlam)
            plan = vrt.FormalPlan(hs, ks, n_sweeps, dirs=dirs)
            _, I = plan.execute(S, alpha, I0_up=I0u, I0_down=I0d, want_J=False, want_I=True)
            assert plan.last_path == path, (name, form, plan.last_path)               # no path declines these grids
            if path == "patches":
                assert (plan.last_launches == 1) == (form != "per-layer"), (name, form)
            plan.close()
            plan = vrt.FormalPlan(hs, qk, n_sweeps, dirs=qd)
            J, _ = plan.execute(S, alpha, weights=w, I0_up=I0u, I0_down=I0d)
            assert plan.last_path == path, (name, form, plan.last_path)
            plan.close()
            out[form][(nlam, n_sweeps)] = (I, J)
    hs.close()
    return out


@pytest.mark.parametrize("name", SOLVE_GRIDS)
def test_solves_follow_the_table_on_every_path(name, monkeypatch):
    """A wrong id that the table readback might mask shows in I: one solve per direction (a plan of all of them, per-angle
    I against Delaunay_upII / Delaunay_downII) and one J over ul7n12, on the level, layer-step, tile and patch paths, the
    patch path as per-layer launches, chained and chained with the data-as-flag hand-off; 1 and 3 wavelengths, 1 and 3
    sweeps; alpha over the three linear_weights branches; random I_0 of both sweeps.  The patch path's launch forms agree
    bit for bit."""
    ds = [directions()[a] for a in solve_directions(name)]
    res = _solve_all_forms(name, monkeypatch)
    fails = []
    for form, _, _ in FORMS:
        for nlam, n_sweeps in SETTINGS:
            I, J = res[form][(nlam, n_sweeps)]
            ref = oracle_solves(name, nlam, n_sweeps)
            errs = [float(_rel(I[a], ref[a])) for a in range(len(ds))]
            eJ = float(_rel(J, oracle_J(name, nlam, n_sweeps)))
            worst = int(np.argmax(errs))
            print("solves, %-14s %-9s nlam %d n_sweeps %d: %d directions, worst element-wise |gpu - oracle| / |oracle| %.3e (%s), "
                  "J over ul7n12 %.3e" % (name, form, nlam, n_sweeps, len(ds), errs[worst], ds[worst].label, eJ))
            fails += [(form, nlam, n_sweeps, ds[a].label, errs[a]) for a in range(len(ds)) if not errs[a] < RTOL]
            if not eJ < RTOL:
                fails.append((form, nlam, n_sweeps, "J", eJ))
    assert not fails, fails[:10]
    for form in ("chain", "chain-df"):
        for key in SETTINGS:
            assert np.array_equal(res[form][key][0], res["per-layer"][key][0]), (name, form, key, "I")
            assert np.array_equal(res[form][key][1], res["per-layer"][key][1]), (name, form, key, "J")
    print("solves, %-14s the patch path's launch forms (per-layer, chain, chain-df) agree bit for bit" % name)
