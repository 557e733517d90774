"""Time Λ_regular's loop on the device (vrt_regular_lambda_*) at a size a user would run, and the oracle-driven CPU loop
at a size it finishes in.

  python tools/regular_lambda_probe.py --size 128 --iters 3
      synth.regular_line_case(128, 128, 128) (128 x 130 x 130 points with the periodic ghost border), 51 + 20 + 20
      wavelengths, ul7n12: ms of each vrt_regular_lambda_iterate (wall clock; the call synchronises)
  rocprofv3 --kernel-trace -d OUT -o run -- python tools/regular_lambda_probe.py --size 128 --iters 2
  python tools/regular_lambda_probe.py --phases OUT/run_results.db --iters 2
      the kernel time of an iteration split into its phases (opacity, solves, J reduction, layout, update, rates)
  python tools/regular_lambda_probe.py --size 128 --iters 8 --operator diagonal
      the same with vrt_regular_lambda_use_operator(1): Λ* of every iterate's α (k_regular_line_lambda_diagonal) and the ALI
      update; --hard for ε × 1e-2 and strength × 10, --ng START PERIOD
      (VRT_LIB_PATH=<an older build> with the operator off times that build: the alternating A/B of profiles/regular_line_ali)
  python tools/regular_lambda_probe.py --oracle --size 32 --iters 1
      the same loop driven by the oracle (orc.line_terms, orc.line_opacity, orc.short_characteristics_up/down,
      orc.calculate_R, orc.revised_populations) on the CPU, one thread
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = (("opacity", ("k_reg_line_opacity",)),
          ("solves", ("k_regular_solve", "k_reg_xy_coefs", "k_reg_xy_march")),
          ("J reduction", ("k_reg_reduce_J",)),
          ("Λ*", ("k_regular_line_lambda_diagonal",)),
          ("layout", ("k_reg_lam_to_planes", "k_reg_lam_from_planes")),
          ("update", ("k_lambda_update",)),
          ("rates", ("k_rates_populations", "k_line_terms")))


def _case(size: int, seed: int, hard: bool = False):
    import voronoirt_amd as vrt
    from voronoirt_amd import synth
    z, x, y, kw = synth.regular_line_case(size, size, size, seed=seed, nbb=51, nbf=20)
    if hard:                                   # the recipe of tests/test_line_ali_host.hard_case
        kw["eps"] = np.asarray(kw["eps"]) * 1e-2
        kw["strength_const"] = kw["strength_const"] * 10.0
    return z, x, y, vrt.LineCase(**kw)


def device_run(size: int, iters: int, seed: int, operator: str = "", hard: bool = False, ng=None) -> dict:
    import voronoirt_amd as vrt
    from voronoirt_amd import _lib, api
    z, x, y, case = _case(size, seed, hard)
    L = _lib.load()
    w, k, dirs = api._regular_directions("ul7n12.dat")
    lc, keep = case.c_struct()
    solver = vrt.RegularSolver(z, x, y)
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    _lib.check(L.vrt_regular_lambda_create(solver._h, k.shape[0], api._d(k), dirs.ctypes.data_as(_lib.p_int), api._d(w),
                                           ctypes.byref(lc), 3, ctypes.byref(h)))
    create_ms = (time.perf_counter() - t0) * 1e3
    if ng:
        _lib.check(L.vrt_regular_lambda_set_acceleration(h, 2, int(ng[0]), int(ng[1])))
    if operator:
        _lib.check(L.vrt_regular_lambda_use_operator(h, 1))
    ms, hist, fallback, applied = [], [], 0, []
    for i in range(iters):
        d = ctypes.c_double()
        t0 = time.perf_counter()
        _lib.check(L.vrt_regular_lambda_iterate(h, ctypes.byref(d)))
        ms.append((time.perf_counter() - t0) * 1e3)
        hist.append(d.value)
        if operator:
            op, cnt = ctypes.c_int(), ctypes.c_int64()
            _lib.check(L.vrt_regular_lambda_get_operator(h, ctypes.byref(op), ctypes.byref(cnt)))
            fallback += cnt.value
        if ng:
            ok = ctypes.c_int()
            _lib.check(L.vrt_regular_lambda_last_acceleration(h, ctypes.byref(ok), None, None))
            if ok.value == 1:
                applied.append(i + 1)
    L.vrt_regular_lambda_destroy(h)
    solver.close()
    n, nlam = case.doppler.size, int(np.asarray(case.lam).size)
    return {"points": n, "shape": [z.size, x.size, y.size], "nlam": nlam, "solves_per_iteration": int((dirs != 0).sum()) * nlam,
            "operator": operator or "plain", "hard": hard, "ng": list(ng) if ng else None, "ng_applied_after": applied,
            "fallback_entries": fallback, "library": os.environ.get("VRT_LIB_PATH", "this tree"),
            "create_ms": round(create_ms, 1), "iterate_ms": [round(v, 2) for v in ms], "history": hist}


def oracle_run(size: int, iters: int, seed: int) -> dict:
    import voronoirt_amd as vrt
    from oracle import oracle as orc
    z, x, y, case = _case(size, seed)
    w, th, ph, nq = vrt.read_quadrature("ul7n12.dat")
    nz, nx, ny = z.size, x.size, y.size
    pops, S_new = case.lte.copy(), case.B0.copy()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        S_old = S_new.copy()
        gamma, strength = orc.line_terms(case.gamma_static, case.gamma_unsold, pops, case.strength_const, case.Bij, case.Bji)
        J = np.zeros_like(S_old)
        for a in range(nq):
            if th[a] == 90:
                continue
            kk = orc.direction(th[a], ph[a])
            alpha = orc.line_opacity(kk, case.lam, case.lambda0, case.c0, case.velocity, case.doppler, gamma, strength,
                                     case.alpha_cont)
            for l in range(S_old.shape[1]):
                S_l, a_l = S_old[:, l].reshape(ny, nx, nz), alpha[:, l].reshape(ny, nx, nz)
                if th[a] > 90:
                    I = orc.short_characteristics_up(kk, S_l, case.B0[:, l].reshape(ny, nx, nz)[:, :, 0], a_l, z, x, y)
                else:
                    I = orc.short_characteristics_down(kk, S_l, np.zeros((ny, nx)), a_l, z, x, y)
                J[:, l] += w[a] * I.ravel()
        S_new = (1 - case.eps)[:, None] * J + case.eps[:, None] * case.B0
        R = orc.calculate_R(case.lam, case.blocks, J, case.planck2, case.lambda0, case.c0, case.doppler, gamma,
                            case.sigma_bb_const, case.sigma_bf1, case.sigma_bf2, case.temperature, case.lte,
                            case.hc_over_kB, case.pref_ij, case.pref_ji)
        pops = orc.revised_populations(R, case.C, case.atom_density)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"oracle_points": case.doppler.size, "shape": [nz, nx, ny], "threads": 1,
            "cpu_cores_visible": len(os.sched_getaffinity(0)), "iterate_ms": [round(v, 1) for v in ms]}


def phases(trace_db: str, iters: int) -> dict:
    """rocprofv3 kernel trace (its rocpd SQLite output) -> ms per iteration of each phase; what the session's creation
    launches (one S transpose, the I_0 planes, fills) is counted with the phase it belongs to, a few tenths of a ms"""
    import sqlite3
    tot = {p: 0.0 for p, _ in PHASES}
    other = 0.0
    con = sqlite3.connect(trace_db)
    for name, ns in con.execute("SELECT name, SUM(end - start) FROM kernels GROUP BY name"):
        for p, keys in PHASES:
            if any(f"::{k}(" in name or f"::{k}<" in name for k in keys):
                tot[p] += ns
                break
        else:
            other += ns
    out = {p: round(v / 1e6 / iters, 3) for p, v in tot.items()}
    out["other kernels (fills, copies), whole run"] = round(other / 1e6, 3)
    s = sum(tot.values())
    out["share"] = {p: round(v / s, 4) for p, v in tot.items()} if s else {}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--phases", default="")
    ap.add_argument("--operator", default="", choices=["", "diagonal"])
    ap.add_argument("--hard", action="store_true")
    ap.add_argument("--ng", type=int, nargs=2, default=None, metavar=("START", "PERIOD"))
    a = ap.parse_args()
    if a.phases:
        res = phases(a.phases, a.iters)
    elif a.oracle:
        res = oracle_run(a.size, a.iters, a.seed)
    else:
        res = device_run(a.size, a.iters, a.seed, a.operator, a.hard, a.ng)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
