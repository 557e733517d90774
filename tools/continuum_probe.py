#!/usr/bin/env python3
"""diagnostics: what one iterate of the continuum Λ-iteration session (vrt_continuum_*) costs beside the bare sweep, at
the size of BASELINE C2 (246 420 sites x ul7n12 x 1 λ, --a 37 --c 90) and at 1 M sites x 1 λ (--a 59 --c 143):

  iterate   wall time of the synchronous vrt_continuum_iterate (sweep + masked update + the read-back of the scalar)
  sweep     vrt_plan_execute_native_dev with VRT_ALPHA_SITE_LAM_NATIVE on plane sets of the same size, wall time of
            launch + stream synchronisation, and the device time between the plan's events (last_sweep_timing)
  update    vrt_continuum_update_dev alone (caller layout, the same element count; it reads the scalar back itself)
  readback  a 24-byte device-to-host copy + stream synchronisation on an idle stream: what a scalar per iterate costs

Median and min..max over the repeats after warm-up.  `--bare` measures the sweep alone and needs no continuum entry: run
it with VRT_LIB_PATH pointing at a build of the parent commit for the A/B (tools/ab_libs.sh does the same for bench.py).
The probe ends itself after --limit seconds.

    python tools/continuum_probe.py [--a 37 --c 90] [--reps 40] [--bare] [--json out.json]
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
ap.add_argument("--bare", action="store_true", help="the sweep alone (works with a library of the parent commit)")
ap.add_argument("--limit", type=int, default=240, help="seconds after which the probe ends itself")
ap.add_argument("--json", default="")
args = ap.parse_args()
signal.alarm(args.limit)

pos, nbr, bounds = synth.bcc_grid(args.a, args.c, seed=2022)
sites = vrt.VoronoiSites(pos, nbr, bounds, device=0)
n, nlam = sites.n, args.nlam
kw = synth.continuum_case(pos, bounds, nlam, seed=5)
quad = "ul7n12.dat"
plan, w = api._quadrature_plan(sites, quad, 3)
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
L = _lib.load()


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "reps": len(xs)}


def timed(fn, reps, warm=5):
    out = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            out.append(1e3 * (time.perf_counter() - t0))
    return out


res = {"sites": n, "nlam": nlam, "quadrature": quad, "lib": os.path.basename(_lib.LIB_PATH), "bare": args.bare}

# ---- the bare sweep on sweep-order planes -----------------------------------------------------------------------------------
B, A = t(kw["B0"]), t(kw["alpha"])
cnt = plan.native_plane_count(nlam)
S_up, S_dn, J_up, J_dn = (torch.zeros(cnt, dtype=torch.float64, device=dev) for _ in range(4))
A_nat = torch.zeros(2 * cnt, dtype=torch.float64, device=dev)
plan.to_native_dev(nlam, nlam, B.data_ptr(), S_up.data_ptr(), S_dn.data_ptr(), stream=st)
plan.to_native_dev(nlam, nlam, A.data_ptr(), A_nat.data_ptr(), A_nat.data_ptr() + 8 * cnt, stream=st)
n1 = int(sites.layers_up[1] - 1)
I0 = B[torch.as_tensor(sites.perm_up[:n1] - 1, device=dev)].contiguous()
dev_ms = []


def sweep():
    plan.execute_native_dev(nlam, S_up.data_ptr(), S_dn.data_ptr(), A_nat.data_ptr(), _lib.ALPHA_SITE_LAM_NATIVE, w,
                            dJ_up=J_up.data_ptr(), dJ_down=J_dn.data_ptr(), dI0_up=I0.data_ptr(), stream=st)
    torch.cuda.synchronize()
    dev_ms.append(plan.last_sweep_timing()[0])


res["sweep_wall"] = stats(timed(sweep, args.reps))
res["sweep_device"] = stats(dev_ms[5:])
res["path"] = plan.last_path
plan.check()

if not args.bare:
    # ---- the session's iterate ------------------------------------------------------------------------------------------------
    case = vrt.ContinuumCase(**kw)
    cc = case.c_struct()
    wd = np.ascontiguousarray(w, dtype=np.float64)
    h = ctypes.c_void_p()
    api.check(L.vrt_continuum_create(plan._h, ctypes.byref(cc), wd.ctypes.data_as(_lib.p_dbl), ctypes.byref(h)))
    d = ctypes.c_double()
    hist = []

    def iterate():
        api.check(L.vrt_continuum_iterate(h, ctypes.byref(d)))
        hist.append(d.value)

    res["iterate_wall"] = stats(timed(iterate, args.reps))
    res["history_head"] = hist[:5]
    L.vrt_continuum_destroy(h)
    # ---- the masked update alone, caller layout ---------------------------------------------------------------------------------
    J, E, S_old, S_new = t(kw["B0"] * 0.9), t(kw["eps"]), B.clone(), torch.empty_like(B)
    res["update_wall"] = stats(timed(lambda: vrt.continuum_update_dev(sites, J, B, E, S_old, S_new, 1e-4), args.reps))
    # ---- a scalar read-back on an idle stream ---------------------------------------------------------------------------------
    words = torch.zeros(3, dtype=torch.int64, device=dev)
    host = torch.zeros(3, dtype=torch.int64).pin_memory()

    def readback():
        host.copy_(words, non_blocking=True)
        torch.cuda.current_stream().synchronize()

    res["readback_wall"] = stats(timed(readback, args.reps))
    res["session_overhead_over_sweep_wall_ms"] = res["iterate_wall"]["median_ms"] - res["sweep_wall"]["median_ms"]

print(json.dumps(res))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
