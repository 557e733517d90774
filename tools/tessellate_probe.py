#!/usr/bin/env python3
"""diagnostics: the Voronoi tessellation on the host (vrt_tessellate) and on the device (vrt_tessellate_gpu, transfers
included; vrt_tessellate_dev by events: grid build, cell kernel, row assembly with any host recomputation) for sites drawn
as synth.voronoi_grid draws them (uniform in x and y, density ~ exp(-(z - z_min)/H) in z).
usage: python tools/tessellate_probe.py [--n 1000000] [--scale-height 0.15 (of the box; 0: uniform)] [--reps 3]
                                        [--plan QUADRATURE  also time vrt_plan_create on the resulting grid, as
                                                            tools/plan_create_probe.py does]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voronoirt_amd as vrt
from voronoirt_amd import _lib, api

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--scale-height", type=float, default=0.15)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--seed", type=int, default=3)
ap.add_argument("--plan", default=None)
a = ap.parse_args()

import torch

L = _lib.load()
D1 = 71
n = a.n
bounds = (-0.5e6, 14.0e6, 0.0, 6.0e6, 0.0, 6.0e6)
rng = np.random.default_rng(a.seed)
Lz = bounds[1] - bounds[0]
x = rng.random(n) * 6.0e6
y = rng.random(n) * 6.0e6
u = rng.random(n)
H = a.scale_height * Lz
z = bounds[0] + u * Lz if H == 0 else bounds[0] - H * np.log(1.0 - u * (1.0 - np.exp(-Lz / H)))
pos = np.ascontiguousarray(np.stack([z, x, y], axis=1))
b = np.array(bounds, dtype=np.float64)
pd, pi = _lib.p_dbl, _lib.p_i64
print(f"sites {n}, scale height {a.scale_height} of the box, host threads {len(os.sched_getaffinity(0))}", flush=True)


def timed(label, call, reps):
    """one warm-up visit, then `reps` timed ones"""
    times = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if r:
            times.append(dt)
    print(f"{label}: " + " ".join(f"{t:.4f}" for t in times) + f" s  (median {np.median(times):.4f} s)", flush=True)
    return float(np.median(times))


Mh = np.zeros((D1, n), dtype=np.int64)
Mg = np.zeros((D1, n), dtype=np.int64)
mxh, mxg, hs = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()


def host():
    vrt.api.check(L.vrt_tessellate(n, pos.ctypes.data_as(pd), b.ctypes.data_as(pd), D1, Mh.ctypes.data_as(pi), ctypes.byref(mxh)))


def gpu():
    vrt.api.check(L.vrt_tessellate_gpu(0, n, pos.ctypes.data_as(pd), b.ctypes.data_as(pd), D1, Mg.ctypes.data_as(pi),
                                       ctypes.byref(mxg), ctypes.byref(hs)))


t_host = timed("host vrt_tessellate     ", host, a.reps)
t_gpu = timed("vrt_tessellate_gpu (h2d, d2h included)", gpu, a.reps)
print(f"host / device wall time: {t_host / t_gpu:.1f}x;  host_sites {hs.value};  max row length host {mxh.value} device {mxg.value};"
      f"  matrices equal: {bool(np.array_equal(Mh, Mg))}", flush=True)
if not np.array_equal(Mh, Mg):
    bad = np.nonzero((Mh != Mg).any(axis=0))[0]
    print(f"  rows that differ: {bad.size}; first: site {bad[0] + 1} host {Mh[:Mh[0, bad[0]] + 1, bad[0]].tolist()} device "
          f"{Mg[:Mg[0, bad[0]] + 1, bad[0]].tolist()}")

dpos = torch.as_tensor(pos, device="cuda")
phases = []
for r in range(a.reps + 1):
    M, _ = vrt.voro_dev(dpos, bounds)
    nn, g, c, w = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    L.vrt_tessellate_last_phases(ctypes.byref(nn), ctypes.byref(g), ctypes.byref(c), ctypes.byref(w))
    if r:
        phases.append((g.value, c.value, w.value))
ph = np.median(np.array(phases), axis=0)
print("vrt_tessellate_dev by events, ms (median of %d): grid build %.3f, cell kernel %.3f, rows + fallback %.3f, sum %.3f"
      % (a.reps, ph[0], ph[1], ph[2], ph.sum()), flush=True)
print(f"device matrix of the _dev form equals the host form's: {bool(np.array_equal(M.cpu().numpy(), Mg))}", flush=True)

if a.plan:
    sites = vrt.VoronoiSites(pos, np.ascontiguousarray(Mg[: mxg.value + 1]), bounds, device=0)
    ts = []
    for rep in range(3):
        t0 = time.perf_counter()
        plan, w = api._quadrature_plan(sites, a.plan, 3)
        ts.append(time.perf_counter() - t0)
        sites._plans.clear()
        del plan
    print(f"plan_create on this grid ({a.plan}): " + " ".join(f"{t:.3f}" for t in ts) + " s", flush=True)
    print(f"mark (vrt_tessellate_gpu <= plan creation): {t_gpu:.3f} s vs {min(ts):.3f} s -> {'met' if t_gpu <= min(ts) else 'missed'}")
