#!/usr/bin/env python3
"""diagnostics: what the diagonal operator of the continuum Λ-iteration session costs (vrt_continuum_set_operator), at the
size of BASELINE C2 (246 420 sites x ul7n12 x 1 λ, --a 37 --c 90):

  plain_iterate   wall time of the synchronous vrt_continuum_iterate of a plain session
  ali_iterate     the same after vrt_continuum_set_operator(s, 1): one more plane-set read in the update kernel
  set_operator    wall time of vrt_continuum_set_operator(s, 1) itself: Λ* (k_lambda_diagonal), min den, the up-order
                  plane set; once per session (measured on a fresh session each time)
  plain_update / ali_update
                  vrt_continuum_update_dev / vrt_continuum_ali_update_dev alone (caller layout, the same element count;
                  each reads the scalar back itself)

Median and min..max over the repeats after warm-up; the two iterates are measured in alternating blocks on two sessions
of one process.  `--plain-only` measures the plain iterate alone and needs no new entry: run it with VRT_LIB_PATH pointing
at a build of the parent commit for the A/B.  The probe ends itself after --limit seconds.

`--regular`: the same three figures for the raster session (vrt_regular_continuum_select_operator) at bench_regular.py's
raster size (--shape 215 128 128 interior points, ghosted to 215 x 130 x 130) x ul7n12 x --nlam; the two update kernels
are those of the Voronoi session and are not timed again.

    python tools/ali_probe.py [--a 37 --c 90] [--nlam 1] [--reps 40] [--blocks 3] [--plain-only] [--json out.json]
    python tools/ali_probe.py --regular [--shape 215 128 128] [--nlam 1] [--reps 10] [--blocks 3] [--plain-only]

`--line`: the LINE session (vrt_lambda_use_operator).  Iterate counts and wall times of Lambda_voronoi_host to --tol on
a hard two-level case (the atom of tests/test_physics.py's _lambda_case with ε x 1e-2 and the line strength x 10; 21 line +
2 x 6 continuum wavelengths): plain, operator="diagonal", and that with ng=(4, 4); at most --maxiter iterates each.

    python tools/ali_probe.py --line [--a 59 --c 143] [--tol 1e-3] [--maxiter 400] [--plain-only]

`--regular-line`: the Λ* kernel of the raster LINE session alone (vrt_regular_line_lambda_diagonal_dev: the planes zeroed,
then k_regular_line_lambda_diagonal over all 12 x --nlam solves as one chunk) on random per-angle α planes made on the
device, at --size^3 interior points: wall time of the synchronous call and the bytes per second of what it must move
(α read once, Λ* zeroed, read and written).  The iterate itself, operator off and on: tools/regular_lambda_probe.py.

    python tools/ali_probe.py --regular-line [--size 128] [--nlam 91] [--reps 7]
"""
import argparse
import ctypes
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voronoirt_amd as vrt                     # noqa: E402
from voronoirt_amd import _lib, api, synth      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--a", type=int, default=37)
ap.add_argument("--c", type=int, default=90)
ap.add_argument("--nlam", type=int, default=1)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--blocks", type=int, default=3, help="alternating blocks of --reps iterates per session")
ap.add_argument("--plain-only", action="store_true", help="the plain iterate alone (works with a library of the parent commit)")
ap.add_argument("--limit", type=int, default=240, help="seconds after which the probe ends itself")
ap.add_argument("--json", default="")
ap.add_argument("--regular", action="store_true", help="the raster session instead of the Voronoi one")
ap.add_argument("--shape", type=int, nargs=3, default=[215, 128, 128], help="--regular: nz nx ny interior points")
ap.add_argument("--line", action="store_true", help="the line session: iterate counts plain / diagonal / diagonal + Ng")
ap.add_argument("--tol", type=float, default=1e-3, help="--line: the criterion the runs stop at")
ap.add_argument("--maxiter", type=int, default=400, help="--line: iterates per run at most")
ap.add_argument("--regular-line", action="store_true", help="the Λ* kernel of the raster line session alone")
ap.add_argument("--size", type=int, default=128, help="--regular-line: interior points per axis")
args = ap.parse_args()
signal.alarm(args.limit)


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "reps": len(xs)}


def regular_probe():
    nz, nx, ny = args.shape
    z, x, y, kw = synth.regular_continuum_case(nz, nx, ny, 5, args.nlam)
    case = vrt.ContinuumCase(**kw)
    cc = case.c_struct()
    quad = "ul7n12.dat"
    w, k, dirs = api._regular_directions(quad)
    L = _lib.load()
    solvers = []

    def session():
        solver = api._regular_solver(z, x, y, case.n, 0)         # (a session's chunk workspace lives on its solver)
        solvers.append(solver)
        h = ctypes.c_void_p()
        api.check(L.vrt_regular_continuum_create(solver._h, k.shape[0], k.ctypes.data_as(_lib.p_dbl),
                                                 dirs.ctypes.data_as(_lib.p_int), w.ctypes.data_as(_lib.p_dbl), ctypes.byref(cc), 3,
                                                 ctypes.byref(h)))
        return h

    def iterates(h, reps, out):
        d = ctypes.c_double()
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api.check(L.vrt_regular_continuum_iterate(h, ctypes.byref(d)))
            out.append(1e3 * (time.perf_counter() - t0))
        return d.value

    res = {"grid": "regular", "points": case.n, "shape_ghosted": [int(z.size), int(x.size), int(y.size)], "nlam": args.nlam,
           "quadrature": quad, "lib": os.path.basename(_lib.LIB_PATH), "plain_only": args.plain_only}
    plain = session()
    iterates(plain, 2, [])                                     # warm-up
    t_plain, t_ali, t_set = [], [], []
    if args.plain_only:
        for _ in range(args.blocks):
            iterates(plain, args.reps, t_plain)
    else:
        for _ in range(4):                                     # the one-time cost, on fresh sessions
            h = session()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api.check(L.vrt_regular_continuum_select_operator(h, 1))
            t_set.append(1e3 * (time.perf_counter() - t0))
            L.vrt_regular_continuum_destroy(h)
            solvers.pop().close()
        ali = session()
        api.check(L.vrt_regular_continuum_select_operator(ali, 1))
        iterates(ali, 2, [])
        for _ in range(args.blocks):
            iterates(plain, args.reps, t_plain)
            res["ali_last_scalar"] = iterates(ali, args.reps, t_ali)
        res["ali_iterate_wall"] = stats(t_ali)
        res["set_operator_wall"] = stats(t_set[1:])
        res["set_operator_first_ms"] = t_set[0]
        res["ali_minus_plain_iterate_ms"] = res["ali_iterate_wall"]["median_ms"] - statistics.median(t_plain)
        L.vrt_regular_continuum_destroy(ali)
    res["plain_iterate_wall"] = stats(t_plain)
    L.vrt_regular_continuum_destroy(plain)
    for solver in solvers:
        solver.close()
    return res


def finish(res):
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def line_probe():
    C0, H_PLANCK, K_B = 2.99792458e8, 6.62607015e-34, 1.380649e-23
    pos, nbr, bounds = synth.bcc_grid(args.a, args.c, seed=2022)
    sites = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    n = sites.n
    rng = np.random.default_rng(11)
    nbb, nbf, lambda0 = 21, 6, 121.567e-9
    q = np.concatenate([-np.geomspace(600, 0.05, nbb // 2), [0.0], np.geomspace(0.05, 600, nbb // 2)])
    lam = np.concatenate([lambda0 * (1 + q * 2.5e3 / C0), np.linspace(22.8e-9, 91.17e-9, nbf), np.linspace(91.2e-9, 364.7e-9, nbf)])
    nlam = lam.size
    z = (pos[:, 0] - bounds[0]) / (bounds[1] - bounds[0])
    box = bounds[1] - bounds[0]
    T = 6e3 + 6e3 * z + 200 * rng.random(n)
    doppler = lambda0 / C0 * np.sqrt(2 * K_B * T / 1.6735575e-27)
    n1 = 1e16 * np.exp(-3 * z) * (1 + 0.1 * rng.random(n))
    lte = np.stack([n1, n1 * 1e-3 * (1 + rng.random(n)), n1 * 1e-2 * (1 + rng.random(n))])
    Cm = 10 ** rng.uniform(-1, 1, (n, 3, 3))
    for d in range(3):
        Cm[:, d, d] = 0.0
    case = vrt.LineCase(
        lam=lam, blocks=np.array([0, nbb, nbb, nbb + nbf, nbb + nbf, nbb + 2 * nbf], dtype=np.int64), lambda0=lambda0, c0=C0,
        velocity=rng.normal(0, 3e3, (n, 3)), doppler=doppler, gamma_static=4.702e8 + 10 ** rng.uniform(7, 8.7, n),
        gamma_unsold=10 ** rng.uniform(-8.5, -7.5, n), alpha_cont=0.05 / box * np.exp(-2 * z),
        eps=1e-2 * 10 ** rng.uniform(-2.5, -0.5, n), temperature=T, atom_density=lte.sum(axis=0),
        B0=(1.0 + z)[:, None] * (1 + 0.05 * rng.random((n, nlam))), lte=lte, C=Cm, planck2=2.0 * (lambda0 / lam) ** 5,
        sigma_bf1=1e-21 * (lam[21:27] / lam[26]) ** 3, sigma_bf2=2e-21 * (lam[27:33] / lam[32]) ** 3,
        strength_const=10.0 * 60.0 / box * doppler.mean() / n1.mean(), Bij=1.0, Bji=0.25, sigma_bb_const=2e-32,
        hc_over_kB=H_PLANCK * C0 / K_B, pref_ij=2e36, pref_ji=2e37)
    res = {"n": n, "nlam": nlam, "tol": args.tol, "maxiter": args.maxiter}
    runs = [("plain", {})] if args.plain_only else [("plain", {}), ("diagonal", {"operator": "diagonal"}),
                                                    ("diagonal_ng", {"operator": "diagonal", "ng": (4, 4)})]
    for name, kw in runs:
        t0 = time.perf_counter()
        out = vrt.Lambda_voronoi_host(args.tol, args.maxiter, sites, case, "ul7n12.dat", **kw)
        hist = out[3]
        res[name] = {"iterates": len(hist), "last": hist[-1], "converged": bool(hist[-1] <= args.tol),
                     "wall_s": time.perf_counter() - t0, "history_head": hist[:40], "S_min": float(out[1].min()),
                     "S_max": float(out[1].max()), "populations_min": float(out[2].min())}
        print(f"{name}: {len(hist)} iterates, criterion {hist[-1]:.4g}, {res[name]['wall_s']:.1f} s in all", file=sys.stderr)
    sites.close()
    return res


def regular_line_probe():
    z, x, y, _ = synth.regular_line_case(args.size, args.size, args.size, seed=5, nbb=5, nbf=2)    # (the ghosted axes only)
    n = z.size * x.size * y.size
    quad = "ul7n12.dat"
    w, k, dirs = api._regular_directions(quad)
    A = int((dirs != 0).sum())
    L = _lib.load()
    solver = api._regular_solver(z, x, y, n, 0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    dz = float(np.diff(z).mean())
    d_alpha = torch.empty((A, args.nlam, n), dtype=torch.float64, device=dev)
    for a in range(A):                                         # Δτ = α dz from 1e-3 to 1e3
        d_alpha[a] = 10.0 ** (6.0 * torch.rand((args.nlam, n), dtype=torch.float64, device=dev, generator=gen) - 3.0) / dz
    d_diag = torch.empty((args.nlam, n), dtype=torch.float64, device=dev)
    out = []
    for i in range(1 + args.reps):                             # one warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api.check(L.vrt_regular_line_lambda_diagonal_dev(solver._h, k.shape[0], k.ctypes.data_as(_lib.p_dbl),
                                                         dirs.ctypes.data_as(_lib.p_int), w.ctypes.data_as(_lib.p_dbl), args.nlam,
                                                         d_alpha.data_ptr(), d_diag.data_ptr(), None))
        if i:
            out.append(1e3 * (time.perf_counter() - t0))
    nbytes = 8 * n * args.nlam * (A + 3)
    res = {"grid": "regular line", "points": n, "shape_ghosted": [int(z.size), int(x.size), int(y.size)], "nlam": args.nlam,
           "active_angles": A, "lambda_star_wall": stats(out), "bytes": nbytes,
           "GB_per_s_at_median": nbytes / statistics.median(out) / 1e6, "diag_max": float(d_diag.max()),
           "diag_min_interior_is_positive": bool((d_diag.view(args.nlam, z.size, y.size, x.size)[:, 1:-1, 1:-1, 1:-1] > 0).all())}
    solver.close()
    return res


if args.regular_line:
    finish(regular_line_probe())
    sys.exit(0)
if args.regular:
    finish(regular_probe())
    sys.exit(0)
if args.line:
    finish(line_probe())
    sys.exit(0)

pos, nbr, bounds = synth.bcc_grid(args.a, args.c, seed=2022)
sites = vrt.VoronoiSites(pos, nbr, bounds, device=0)
n, nlam = sites.n, args.nlam
kw = synth.continuum_case(pos, bounds, nlam, seed=5)
quad = "ul7n12.dat"
plan, w = api._quadrature_plan(sites, quad, 3)
L = _lib.load()
case = vrt.ContinuumCase(**kw)
cc = case.c_struct()
wd = np.ascontiguousarray(w, dtype=np.float64)


def session():
    h = ctypes.c_void_p()
    api.check(L.vrt_continuum_create(plan._h, ctypes.byref(cc), wd.ctypes.data_as(_lib.p_dbl), ctypes.byref(h)))
    return h


def iterates(h, reps, out):
    d = ctypes.c_double()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api.check(L.vrt_continuum_iterate(h, ctypes.byref(d)))
        out.append(1e3 * (time.perf_counter() - t0))
    return d.value


res = {"sites": n, "nlam": nlam, "quadrature": quad, "lib": os.path.basename(_lib.LIB_PATH), "plain_only": args.plain_only}
plain = session()
iterates(plain, 5, [])                                         # warm-up
t_plain, t_ali, t_set = [], [], []
if args.plain_only:
    for _ in range(args.blocks):
        iterates(plain, args.reps, t_plain)
else:
    for _ in range(5):                                         # the one-time cost, on fresh sessions
        h = session()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api.check(L.vrt_continuum_set_operator(h, 1))
        t_set.append(1e3 * (time.perf_counter() - t0))
        L.vrt_continuum_destroy(h)
    ali = session()
    api.check(L.vrt_continuum_set_operator(ali, 1))
    iterates(ali, 5, [])
    for _ in range(args.blocks):
        iterates(plain, args.reps, t_plain)
        res["ali_last_scalar"] = iterates(ali, args.reps, t_ali)
    res["ali_iterate_wall"] = stats(t_ali)
    res["set_operator_wall"] = stats(t_set[1:])
    res["set_operator_first_ms"] = t_set[0]
    L.vrt_continuum_destroy(ali)
    # ---- the two update kernels alone, caller layout ---------------------------------------------------------------------
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, J, E, S_old = t(kw["B0"]), t(kw["B0"] * 0.9), t(kw["eps"]), t(kw["B0"])
    S_new = torch.empty_like(B)
    D = t(vrt.lambda_diagonal(sites, kw["alpha"], quad))

    def timed(fn, reps, warm=5):
        out = []
        for i in range(warm + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if i >= warm:
                out.append(1e3 * (time.perf_counter() - t0))
        return out

    res["plain_update_wall"] = stats(timed(lambda: vrt.continuum_update_dev(sites, J, B, E, S_old, S_new, 1e-4), args.reps))
    res["ali_update_wall"] = stats(timed(lambda: vrt.continuum_ali_update_dev(sites, J, B, E, D, S_old, S_new, 1e-4), args.reps))
    res["ali_minus_plain_iterate_ms"] = res["ali_iterate_wall"]["median_ms"] - statistics.median(t_plain)
res["plain_iterate_wall"] = stats(t_plain)
L.vrt_continuum_destroy(plain)

finish(res)
