"""The regular-grid solver (csrc/vrt_regular.hip) over its direction domain and its launch forms, against the CPU
oracle at the solver's contract max|got - ref| / max|ref| < 1e-12.  The inputs -- directions on every decision of
xy_intersect and of the plane argmin, the shape table of regular_launch, the known answer with a gradient -- are built
and shown to be what they claim in tests/test_regular_domain_host.py.  Figures are printed before they are asserted
(profiles/regular_domain/test_regular_domain_figures.txt)."""
import functools
import os

import numpy as np
import pytest

import voronoirt_amd as vrt
from voronoirt_amd import _lib
from test_regular_domain_host import (ALL_FORMS, KAT_MEASURED, KAT_XZ_DOWN_MEASURED, SHAPES, expected_launch, kat_oracle,
                                      kat_run, oracle_solutions, rasters, rel_diff, shape_problem)

PARITY = 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("n_sweeps", [1, 3])
@pytest.mark.parametrize("name", ["generic", "ties", "mixed"])
def test_gpu_direction_domain(monkeypatch, name, n_sweeps):
    """One batch per raster carries the whole direction set with per-solve I_0: every solve against the oracle; the
    all-xy classes again as batches of their own in the three VRT_REG_XY modes, bit for bit (the host's all_xy choice
    against the kernels' own argmin: a batch the host calls all-xy of which a kernel marches one plane as yz differs);
    exact zeros against rounding residues."""
    ra = rasters()[name]
    sol = oracle_solutions(name, n_sweeps)
    got = vrt.short_characteristics_batch(ra.ks, ra.ups, ra.S, ra.I0s, ra.al, ra.z, ra.x, ra.y, n_sweeps)
    diffs = [rel_diff(got[i], sol[i][0]) for i in range(len(ra.cases))]
    classes = sorted({c.cls for c in ra.cases})
    for cls in classes:
        d = [diffs[i] for i, c in enumerate(ra.cases) if c.cls == cls]
        print("direction domain, %-7s n_sweeps %d, %-8s: %2d solves, worst |gpu - oracle| / max|oracle| %.3e"
              % (name, n_sweeps, cls, len(d), max(d)))
    for c, d in zip(ra.cases, diffs):
        assert d < PARITY, (c, d)
    for cls in classes:
        idx = [i for i, c in enumerate(ra.cases) if c.cls == cls and ra.all_xy(i)]
        if not idx:
            continue
        sub = {}
        for mode in ("0", "1", "2"):
            monkeypatch.setenv("VRT_REG_XY", mode)
            sub[mode] = vrt.short_characteristics_batch(ra.ks[idx], [ra.ups[i] for i in idx], ra.S, ra.I0s[idx], ra.al,
                                                        ra.z, ra.x, ra.y, n_sweeps)
        monkeypatch.delenv("VRT_REG_XY")
        for mode in ("1", "2"):
            for j, i in enumerate(idx):
                assert np.array_equal(sub["0"][j], sub[mode][j]), ("VRT_REG_XY=%s differs from the single kernel" % mode, ra.cases[i])
        for j, i in enumerate(idx):
            assert np.array_equal(sub["0"][j], got[i]), ("alone and in the mixed batch", ra.cases[i])
    for i, j in ra.pairs:
        d, d_orc = rel_diff(got[i], got[j]), rel_diff(sol[i][0], sol[j][0])
        if ra.cases[i].differs:                              # the `else` branch was taken for the exact zero, not "repaired"
            assert d > 1e-6, (ra.cases[i], d, d_orc)
        else:
            assert d < PARITY, (ra.cases[i], d, d_orc)
    if ra.pairs:
        dd = [rel_diff(got[i], got[j]) for i, j in ra.pairs if ra.cases[i].differs]
        print("direction domain, %-7s n_sweeps %d, exact zero against its residue where the branches differ: %.3e .. %.3e"
              % (name, n_sweeps, min(dd), max(dd)))


@functools.lru_cache(maxsize=None)
def _run_shape(shape, cls, mode):
    """one (shape, direction class) of the table through RegularSolver.execute_dev under VRT_REG_XY = mode:
    (last_launch_form(), I of every solve)"""
    import torch
    z, x, y, S, al, ks, ups, I0s, _ = shape_problem(shape, cls)
    dev = torch.device("cuda", 0)
    old = os.environ.get("VRT_REG_XY")
    os.environ["VRT_REG_XY"] = mode
    try:
        solver = vrt.RegularSolver(z, x, y, device=0)                # (the mode is read at creation)
    finally:
        if old is None:
            del os.environ["VRT_REG_XY"]
        else:
            os.environ["VRT_REG_XY"] = old
    with pytest.raises(vrt.VrtError):
        solver.last_launch_form()                                    # nothing launched yet
    dS, dA, dI0 = (torch.as_tensor(a, device=dev) for a in (S, al, I0s))
    dI = torch.full((len(ups),) + S.shape, np.nan, device=dev, dtype=torch.float64)
    solver.execute_dev(ks, ups, dS.data_ptr(), 0, dA.data_ptr(), 0, dI0.data_ptr(), dI.data_ptr(), 3,
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    form = solver.last_launch_form()
    got = dI.cpu().numpy()
    solver.close()
    got.setflags(write=False)
    return form, got


def _check_shape_row(row):
    shape, cls, mode, expect = row
    refs = shape_problem(shape, cls)[8]
    form, got = _run_shape(shape, cls, mode)
    d = max(rel_diff(got[j], refs[j][0]) for j in range(len(refs)))
    print("launch form %-16s threads %4d %-36s (nz, nx, ny) = %-14s %-5s VRT_REG_XY=%s: worst |gpu - oracle| / max|oracle| %.3e"
          % (form[0], form[1], form[2] or "", shape, cls, mode, d))
    assert form == expect, (shape, cls, mode)
    for j in range(len(refs)):
        assert rel_diff(got[j], refs[j][0]) < PARITY, (shape, cls, mode, j)
    if cls == "steep":                                               # the three forms of an all-xy batch: the same bits
        for other in ("0", "1", "2"):
            form_o, got_o = _run_shape(shape, cls, other)
            assert form_o == expected_launch(shape, cls, other), (shape, other)
            assert np.array_equal(got, got_o), (shape, mode, other)
    return form


@pytest.mark.gpu
@pytest.mark.parametrize("row", SHAPES, ids=["%dx%dx%d-%s-xy%s" % (r[0] + (r[1], r[2])) for r in SHAPES])
def test_gpu_launch_form(row):
    _check_shape_row(row)


@pytest.mark.gpu
def test_gpu_launch_forms_seen_are_all_the_solver_has():
    """Every form regular_launch can choose was launched by a row of the table, reported by the solver itself (a form
    may leave this list only when the code no longer has it), and both row loops ran under both solve kernels that can
    reach them."""
    seen, rows_seen = set(), set()
    for row in SHAPES:
        form, _ = _run_shape(*row[:3])
        seen.add(form[0])
        if form[2] and row[1] in ("yz", "xz"):
            rows_seen.add((form[0], form[2][row[1]]))
    assert seen == ALL_FORMS == set(_lib.REG_FORMS)
    assert rows_seen == {("solve<256>", "row_march"), ("solve<1024>", "row_march"), ("solve<1024>", "strided")}


@pytest.mark.gpu
def test_gpu_reproduces_a_linear_source_function():
    """I = S + k_z g / alpha for S = s0 + g z: the oracle's measured error, twice, plus the parity contract; xz_down_ray's
    documented miss (centre values from the plane above) stays what the oracle makes it."""
    def batch(ks, ups, S, I0s, al, z, x, y, n_sweeps):
        return vrt.short_characteristics_batch(ks, ups, S, I0s, al, z, x, y, n_sweeps)
    res, ref = kat_run(batch), kat_oracle()
    assert set(res) == {"xy_series", "xy", "rows", "xz_down"}
    for cls in sorted(res):
        errs, errs_o = [r[3] for r in res[cls]], [r[3] for r in ref[cls]]
        par = max(rel_diff(g[4], o[4]) for g, o in zip(res[cls], ref[cls]))
        print("known answer, %-9s: %2d runs, error gpu %.3e .. %.3e, oracle %.3e .. %.3e, worst |gpu - oracle| / max|oracle| %.3e"
              % (cls, len(errs), min(errs), max(errs), min(errs_o), max(errs_o), par))
    for cls, measured in KAT_MEASURED.items():
        for label, alpha, n_sweeps, err, _ in res[cls]:
            assert err <= 2 * measured + PARITY, (cls, label, alpha, n_sweeps, err)
    lo, hi = KAT_XZ_DOWN_MEASURED
    for g, o in zip(res["xz_down"], ref["xz_down"]):
        assert g[:3] == o[:3]
        assert rel_diff(g[4], o[4]) < PARITY, g[:4]
        assert lo / 2 <= g[3] <= 2 * hi, g[:4]
