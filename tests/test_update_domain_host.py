"""CPU tests of oracle/update_ref.py, the reference of the Λ-iteration's "update + criterion" kernels (DESIGN.md §7r;
tests/test_update_domain.py runs the device against it):

  1  forward_bound -- the only bound of this file, derived in its docstring -- holds for the fp64 model against update_mp
     over the ordinary class of value_grid and over 10^5 log-uniform random entries per kind; the ALI model also against
     the form S_old + (S_fs - S_old) / den
  2  every mutant of MUTANTS is caught by a case of seam_cases or value_grid (or the call order of the clean-after-dirty
     test) for every kind and form it applies to, and the true model by none: the case list suffices (-s prints the case
     that catches each)
  3  seam_cases against a brute-force thread map written as the kernels' own loops
  4  every public update entry and its Python wrapper exists with the prototype the GPU test uses
"""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import update_ref as R
from voronoirt_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the shapes of the issue: the smallest at which each seam exists
SITES = (63, 64, 65, 255, 256, 257)
NLAMS = {"line": (1, 2, 7, 8, 9, 17), "line_ali": (1, 2, 7, 8, 9, 17), "continuum": (1, 2, 3, 4, 5),
         "continuum_ali": (1, 2, 3, 4, 5), "line_f32": (1, 2, 3, 5, 7, 8, 9, 17)}
PAIR_BLOCKS = (2, 1, 8)                 # test_f32_lambda.LAYOUTS: default, pairs, block8
BIG = (257, 4081)                       # n nlam just above 2^20: the second grid-stride trip of the row kernels


def launches(kind, form):
    if form == "planes" and kind == "line_f32":
        return [R.launch_of(kind, form, B) for B in PAIR_BLOCKS]
    return [R.launch_of(kind, form)]


def forms(kind):
    return ("planes",) if kind == "line_f32" else ("rows", "planes")


# ---- 1: the bound --------------------------------------------------------------------------------------------------------------
def _model_minus_mp(kind, J, B, eps, S_old, diag, which):
    """|update_model - mp| / forward_bound per entry where all three exist (the largest ratio, the entries counted)"""
    u = R.update_model(kind, J, B, eps, S_old, diag=diag, eps_thick=0.0 if kind in R.CONTINUUM else None)
    ref = R.mp_reference(kind, J, B, eps, S_old, diag)
    mpf = R._mp().mpf
    worst, count = 0.0, 0
    S, bound = u.S_new.ravel(), ref["bound"].ravel()
    for key in which:
        for i, exact in enumerate(ref[key].ravel()):
            if exact is None or not np.isfinite(bound[i]) or not np.isfinite(S[i]):
                continue
            err = float(abs(mpf(S[i]) - exact))
            assert err <= bound[i], (kind, key, i, S[i], exact, err, bound[i])
            worst, count = max(worst, err / bound[i]), count + 1
    return worst, count


@pytest.mark.parametrize("kind", R.KINDS)
def test_forward_bound_holds_on_the_ordinary_class_of_the_value_grid(kind):
    g = R.value_grid(kind)
    u = R.update_model(kind, g["J"], g["B"], g["eps"], g["S_old"], diag=g["diag"], eps_thick=R.VALUE_EPS_THICK)
    cls = R.classify(kind, u)
    ordinary = cls == R.CLASSES.index("ordinary")
    # every class the kind has is present in the grid, and each entry has one class (classify returns one index per entry)
    want = {"line": {"nan", "inf_term", "ordinary"}, "line_f32": {"nan", "inf_term", "ordinary"},
            "line_ali": {"nan", "fallback", "inf_term", "ordinary"}, "continuum": {"thin", "nan", "inf_term", "ordinary"},
            "continuum_ali": {"thin", "nan", "den_zero", "inf_term", "ordinary"}}[kind]
    assert {R.CLASSES[i] for i in np.unique(cls)} == want
    e = np.broadcast_to(g["eps"] if kind in R.CONTINUUM else g["eps"][:, None], g["J"].shape)
    pick = lambda a: None if a is None else a[ordinary][:, None]
    worst, count = _model_minus_mp(kind, pick(g["J"]), pick(g["B"]), pick(e) if kind in R.CONTINUUM else e[ordinary],
                                   pick(g["S_old"]), pick(g["diag"]), ("S", "alt"))
    print(f"{kind}: {int(ordinary.sum())} ordinary entries of {cls.size}, {count} bounded comparisons, largest error / bound {worst:.3f}")
    assert count >= ordinary.sum() // 2


@pytest.mark.parametrize("kind", R.KINDS)
def test_forward_bound_holds_on_random_entries(kind):
    """10^5 log-uniform entries: J, B, S_old over 10^±30 (the float kind: 10^±15, as floats), ε over [1e-12, 1], Λ* uniform
    in [0, 1)"""
    rng = np.random.default_rng(KINDS_SEED[kind])
    n, span = 100000, 15 if kind == "line_f32" else 30
    J, B, S_old = (10.0 ** rng.uniform(-span, span, (n, 1)) for _ in range(3))
    eps = np.minimum(10.0 ** rng.uniform(-12, 0, (n, 1)), 1.0)
    diag = rng.random((n, 1)) if kind in R.ALI else None
    if kind == "line_f32":
        J, B, S_old = R.f32(J), R.f32(B), R.f32(S_old)
    worst, count = _model_minus_mp(kind, J, B, eps if kind in R.CONTINUUM else eps[:, 0], S_old, diag, ("S", "alt"))
    print(f"{kind}: {count} bounded comparisons, largest error / bound {worst:.3f}")
    assert count >= n


KINDS_SEED = {k: 7 + i for i, k in enumerate(R.KINDS)}


# ---- 2: the mutants ---------------------------------------------------------------------------------------------------------
def _same_word(a, b):
    if a is None or b is None:
        return True                                             # (a word the case does not state)
    if isinstance(a, float) and isinstance(b, float):
        return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
    return a == b


def _direct_words(kind, u):
    """the scalar and the third word of an Update by plain Python loops over its entries (no numpy reduction)"""
    p, worst, nan, third = u.parts, 0.0, False, 0
    term, seen, fb = p["term"], p["seen"], p["fallback"]
    for i in range(term.shape[0]):
        for l in range(term.shape[1]):
            third += int(fb[i, l]) if kind == "line_ali" else int(seen[i, l])
            if seen[i, l]:
                if math.isnan(term[i, l]):
                    nan = True
                else:
                    worst = max(worst, float(term[i, l]))
    return (float("nan") if nan else worst), (third if kind in ("line_ali",) + R.CONTINUUM else None)


def _plants(kind):
    out = ["term", "nan", "inf"]
    if kind == "line_ali":
        out += ["fallback", "fallback_site"]
    if kind in R.CONTINUUM:
        out += ["only_thick"]
    return out


def host_cases(kind, launch, sites=(65, 257)):
    """the cases of the GPU file as (name, case dict, nlam, expected scalar, expected third, previous third): every plant at
    every seam of the small shapes, the row kernels' second trip, the value grid class by class and whole, an odd nlam
    with every entry thick (eps_thick < 0: the continuum's padding wavelength would be thick too), and a clean call after
    a counted one"""
    form = launch.form
    for n in sites:
        for nlam in NLAMS[kind]:
            base = R.benign_case(kind, n, nlam, seed=n + nlam)
            u = R.run_case(kind, base)
            yield f"benign {n}x{nlam}", base, nlam, u.scalar, _direct_words(kind, u)[1], 0
            yield f"after a counted call {n}x{nlam}", base, nlam, u.scalar, _direct_words(kind, u)[1], 5
            if kind in R.CONTINUUM and nlam & 1:
                c = dict(base, eps_thick=-1.0)
                yield f"all thick {n}x{nlam}", c, nlam, R.run_case(kind, c).scalar, n * nlam, 0
            for name, row, l in R.seam_cases(n, nlam, launch):
                for what in _plants(kind):
                    c, scalar, third, _ = R.plant(kind, base, what, row, l)
                    yield f"{what} at {name} ({row}, {l}) of {n}x{nlam}", c, nlam, scalar, third, 0
    if form == "rows":
        n, nlam = BIG
        base = R.benign_case(kind, n, nlam, seed=3)
        for name, row, l in R.seam_cases(n, nlam, launch):
            if "trip1" in name or name == "last":
                for what in _plants(kind):
                    c, scalar, third, _ = R.plant(kind, base, what, row, l)
                    yield f"{what} at {name} ({row}, {l}) of {n}x{nlam}", c, nlam, scalar, third, 0
    g = R.value_grid(kind)
    g["eps_thick"] = R.VALUE_EPS_THICK if kind in R.CONTINUUM else None
    whole = R.run_case(kind, g)
    cls = R.classify(kind, whole)
    yield "value grid, whole", g, None, *_direct_words(kind, whole), 0
    filler = R.benign_case(kind, *g["B"].shape, seed=11)
    for k, cname in enumerate(R.CLASSES):
        if (cls == k).any():
            c = R.class_case(kind, g, filler, cls == k)
            yield f"value grid, class {cname}", c, None, *_direct_words(kind, R.run_case(kind, c)), 0


def _caught(kind, launch, mutant, case):
    name, c, nlam, scalar, third, previous = case
    u = R.run_case(kind, c, nlam=nlam, launch=launch, mutant=mutant, previous_third=previous)
    return not (_same_word(u.scalar, scalar) and _same_word(u.third, third))


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_mutant_is_caught_and_the_true_model_by_none(kind):
    for form in forms(kind):
        for launch in launches(kind, form):
            cases = list(host_cases(kind, launch))
            for case in cases:
                assert not _caught(kind, launch, None, case), (kind, launch, case[0])
            for mutant, (kinds, mforms, what) in R.MUTANTS.items():
                if kind not in kinds or form not in mforms:
                    continue
                killer = next((case[0] for case in cases if _caught(kind, launch, mutant, case)), None)
                print(f"{kind} {form}{'' if launch.pair_block is None else f' B={launch.pair_block}'}: {mutant} ({what}) "
                      f"caught by: {killer}")
                assert killer is not None, (kind, launch, mutant)
            print(f"{kind} {form}: the true model passes all {len(cases)} cases")


# ---- 3: the seams against the kernels' own loops ------------------------------------------------------------------------
def _brute_rows(n, nlam):
    """{(row, l): (workgroup, wave, lane, trip, slot)}: the grid-stride loop of k_lambda_update / k_continuum_update"""
    total = n * nlam
    grid = max(min((total + 255) // 256, 256 * 16), 1)
    out, active = {}, {}
    for block in range(grid):
        for thread in range(256):
            t, trip = block * 256 + thread, 0
            while t < total:
                out[(t // nlam, t - t // nlam * nlam)] = (block, thread >> 6, thread & 63, trip, 0)
                active.setdefault((block, trip), []).append(thread)
                t += grid * 256
                trip += 1
    return out, active


def _brute_planes(n, nlam, launch):
    """the same for one thread per position: the pair loops of k_lambda_update_native (U = 4), k_continuum_update_native
    (U = 2) and k_lambda_update_native_f32 (update_units_f32<2> over the quads, then <1>), slot = (which loop, trip, u)"""
    npair = (nlam + 1) // 2
    U = launch.U
    if launch.pair_block is None:
        runs = [(0, npair, 1)]
    else:
        nquad = npair >> 1 if launch.pair_block >= 2 else 0
        runs = [(0, 2 * nquad, 2), (2 * nquad, npair, 1)]
    grid = max(min((n + 255) // 256, 256 * 16), 1)
    out, active = {}, {}
    for block in range(grid):
        for thread in range(256):
            pos, trip = block * 256 + thread, 0
            while pos < n:
                active.setdefault((block, trip), []).append(thread)
                for run, (q_begin, q_end, W) in enumerate(runs):
                    for q0 in range(q_begin, q_end, U * W):
                        clamps = any(q0 + u * W >= q_end for u in range(U))
                        for u in range(U):
                            q = q0 + u * W
                            if q >= q_end:
                                break
                            for c in range(2 * W):
                                if 2 * q + c < nlam:
                                    out[(pos, 2 * q + c)] = (block, thread >> 6, thread & 63, trip, (run, q0, u, c, clamps))
                pos += grid * 256
                trip += 1
    return out, active


def _classes(entries, active, nlam, planes):
    """{class: [entries]} of the entries at a first or last lane: (wave, first/last lane, full or partial workgroup, trip,
    unroll slot, next to the padding wavelength)"""
    out = {}
    for (row, l), (block, wave, lane, trip, slot) in entries.items():
        threads = active[(block, trip)]
        partial = len(threads) < 256
        last_lane = max(t & 63 for t in threads if t >> 6 == wave)
        for which, hit in (("first", lane == 0), ("last", lane == last_lane)):
            if hit:
                pad_nb = planes and nlam & 1 and l == nlam - 1
                if planes:                                      # (which trip of the unroll matters only through tail or not)
                    run, q0, u, c, clamps = slot
                    slot_class = (run, u, c, clamps)
                else:
                    slot_class = 0
                out.setdefault((wave, which, partial, trip, slot_class, bool(pad_nb)), []).append((row, l))
    return out


@pytest.mark.parametrize("kind", R.KINDS)
def test_seam_cases_hit_every_class_of_the_brute_force_thread_map(kind):
    count = 0
    for form in forms(kind):
        for launch in launches(kind, form):
            shapes = [(n, nlam) for n in SITES for nlam in NLAMS[kind]] + ([BIG] if form == "rows" else [])
            for n, nlam in shapes:
                entries, active, classes = _brute(n, nlam, launch)
                assert len(entries) == n * nlam
                # the reference's own map says the same as the loops
                m = R.thread_map(n, nlam, launch)
                for (row, l), (block, wave, lane, trip, slot) in list(entries.items())[:: max(1, len(entries) // 500)]:
                    assert (m["workgroup"][row, l], m["wave"][row, l], m["lane"][row, l], m["trip"][row, l]) == (block, wave, lane, trip)
                    assert m["partial"][row, l] == (len(active[(block, trip)]) < 256)
                    if form == "planes":
                        assert m["slot"][row, l] == slot[2] and m["tail"][row, l] == slot[4]
                cases = {(row, l) for _, row, l in R.seam_cases(n, nlam, launch)}
                assert all(0 <= row < n and 0 <= l < nlam for row, l in cases)
                for cls, members in classes.items():
                    assert cases & set(members), (kind, launch, n, nlam, cls, members[:4])
                    count += 1
                for must in ((0, 0), (n - 1, nlam - 1)):
                    assert must in cases
                if (n, nlam) == BIG:
                    for t in (2 ** 20 - 1, 2 ** 20, n * nlam - 1):
                        assert (t // nlam, t % nlam) in cases
    print(f"{kind}: {count} classes, each hit by a case")


_maps = {}


def _brute(n, nlam, launch):
    """(entries, active threads, classes) of a shape and launch, computed once (the row kernels share one launch)"""
    key = (n, nlam, launch)
    if key not in _maps:
        entries, active = _brute_rows(n, nlam) if launch.form == "rows" else _brute_planes(n, nlam, launch)
        _maps[key] = (entries, active, _classes(entries, active, nlam, launch.form == "planes"))
    return _maps[key]


def test_clamped_slots_are_the_kernels_clamped_loads():
    """the pairs a tail trip loads for its slots past the end, from the load loops' own index expressions"""
    for kind in R.KINDS:
        for launch in launches(kind, "planes"):
            for nlam in NLAMS[kind] + (33, 49, 343):
                npair, U, got = (nlam + 1) // 2, launch.U, []
                if launch.pair_block is None:
                    for q0 in range(0, npair, U):
                        got += [npair - 1 for u in range(U) if not q0 + u < npair]
                else:
                    nquad = npair >> 1 if launch.pair_block >= 2 else 0
                    for q_begin, q_end, W in ((0, 2 * nquad, 2), (2 * nquad, npair, 1)):
                        for q0 in range(q_begin, q_end, U * W):
                            for u in range(U):
                                if not q0 + u * W < q_end:
                                    got += list(range(q_end - W, q_end))
                assert sorted(got) == sorted(R.clamped_slots(npair, launch)), (kind, launch, nlam)


# ---- 4: the entries ------------------------------------------------------------------------------------------------------------
vp, i64, dbl, p_dbl, p_i64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, _lib.p_dbl, _lib.p_i64
ENTRIES = {
    "vrt_lambda_update_dev": [vp, i64, i64, vp, vp, vp, vp, vp, p_dbl, vp],
    "vrt_lambda_ali_update_dev": [vp, i64, i64, vp, vp, vp, vp, vp, vp, p_dbl, p_i64, vp],
    "vrt_lambda_update_native_dev": [vp, i64, vp, vp, vp, vp, vp, vp, p_dbl, vp],
    "vrt_lambda_ali_update_native_dev": [vp, i64, vp, vp, vp, vp, vp, vp, vp, p_dbl, p_i64, vp],
    "vrt_lambda_update_native_dev_f32": [vp, i64, vp, vp, vp, vp, vp, vp, p_dbl, vp],
    "vrt_continuum_update_dev": [vp, i64, i64, vp, vp, vp, dbl, vp, vp, p_dbl, p_i64, vp],
    "vrt_continuum_ali_update_dev": [vp, i64, i64, vp, vp, vp, vp, dbl, vp, vp, p_dbl, p_i64, vp],
    "vrt_continuum_set_operator": [vp, ctypes.c_int],
    "vrt_lambda_use_operator": [vp, ctypes.c_int],
    "vrt_lambda_get_operator": [vp, _lib.p_int, p_i64],
}
WRAPPERS = {
    "lambda_update_dev": ["sites", "nlam", "ld", "dJ", "dB", "deps", "dS_old", "dS_new", "stream"],
    "lambda_ali_update_dev": ["sites", "nlam", "ld", "dJ", "dB", "deps", "d_diag", "dS_old", "dS_new", "stream"],
    "lambda_update_native_dev": ["sites", "nlam", "dJ_up", "dJ_down", "dB_up", "deps", "dS_up", "dS_down", "stream"],
    "lambda_ali_update_native_dev": ["sites", "nlam", "dJ_up", "dJ_down", "dB_up", "deps", "d_diag_up", "dS_up", "dS_down", "stream"],
    "lambda_update_native_dev_f32": ["plan", "nlam", "dJ_up", "dJ_down", "dB_up", "deps", "dS_up", "dS_down", "stream"],
    "continuum_update_dev": ["sites", "J", "B", "eps", "S_old", "S_new", "eps_thick", "nlam"],
    "continuum_ali_update_dev": ["sites", "J", "B", "eps", "diag", "S_old", "S_new", "eps_thick", "nlam"],
}


def test_update_entries_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "voronoirt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, args in ENTRIES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert _lib.PROTOTYPES[name] == (ctypes.c_int, args), name
    for name, params in WRAPPERS.items():
        assert list(inspect.signature(getattr(api, name)).parameters) == params, name
    for name in ("to_native_dev", "from_native_dev", "native_plane_count", "native_pair_block_f32"):
        assert hasattr(vrt.FormalPlan, name)
    assert "operator" in inspect.signature(vrt.Lambda_continuum).parameters
    assert "native" in inspect.signature(vrt.Lambda_continuum).parameters
    # the float model keeps its name where tests/test_f32_lambda.py imports it
    import f32_lambda_model
    assert list(inspect.signature(f32_lambda_model.update_model).parameters) == ["J_up", "J_down", "B", "S_old", "eps", "nlam"]
