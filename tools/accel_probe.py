#!/usr/bin/env python3
"""diagnostics: what Ng acceleration costs inside the Voronoi Λ-iteration session at the C4 session size of
tools/iteration_breakdown.py (995 566 sites, ul7n12, 51 line + 2 x 20 continuum wavelengths):

  (a) vrt_lambda_iterate with acceleration off,
  (b) an iterate that records S into the history (one device-to-device copy of S),
  (c) an iterate that takes a step (sums, apply, the down-order copy),
  (d) vrt_ng_accelerate_dev alone on four arrays of the session's S size (reduction + apply, HIP events on the caller's
      stream; the bytes it must move: 4 reads + 3 reads + 1 write of 8 n nlam).

(a)-(c) are wall times of the synchronous call (it returns when its stream is idle: only the criterion's scalar comes
back), median and min..max over the repeats after warm-up.  The kernels alone: run this under
`rocprofv3 --kernel-trace --stats -- python tools/accel_probe.py` and read k_ng_sums / k_ng_apply / k_ng_mirror.

    python tools/accel_probe.py [--a 59 --c 143] [--reps 24] [--json out.json]

--multi W: the same three kinds of iterate, (a)-(c), of the MULTI-device session (vrt_multi_lambda_*) with device 0 listed W
times -- W wavelength blocks, W histories, W sets of five sums added on the host, one (a, b), the step on every member or
on none -- and nothing else.  A library selected with VRT_LIB_PATH that has no vrt_multi_lambda_set_acceleration (an older
build, for the A/B of (a)) reports (a) only.

    python tools/accel_probe.py --multi 2 [--reps 7] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voronoirt_amd as vrt                     # noqa: E402
from voronoirt_amd import _lib, api, synth      # noqa: E402

C0, H_PLANCK, K_B = 2.99792458e8, 6.62607015e-34, 1.380649e-23

ap = argparse.ArgumentParser()
ap.add_argument("--a", type=int, default=59)
ap.add_argument("--c", type=int, default=143)
ap.add_argument("--reps", type=int, default=24, help="repeats per kind of iterate (>= 20)")
ap.add_argument("--json", default="")
ap.add_argument("--multi", type=int, default=0, help="time the multi-device session with device 0 listed this many times")
args = ap.parse_args()

pos, nbr, bounds = synth.bcc_grid(args.a, args.c, seed=2022)
sites = None if args.multi else vrt.VoronoiSites(pos, nbr, bounds, device=0)
n = pos.shape[0]
rng = np.random.default_rng(7)
nbb, nbf = 51, 20
lambda0 = 121.567e-9
q = np.concatenate([-np.geomspace(600, 0.05, nbb // 2), [0.0], np.geomspace(0.05, 600, nbb // 2)])
lam = np.concatenate([lambda0 * (1 + q * 2.5e3 / C0), np.linspace(22.8e-9, 91.17e-9, nbf), np.linspace(91.2e-9, 364.7e-9, nbf)])
blocks = np.array([0, nbb, nbb, nbb + nbf, nbb + nbf, nbb + 2 * nbf], dtype=np.int64)
nlam_all = lam.size
z = pos[:, 0]
T = (5e3 + 1.5e4 * (z - bounds[0]) / (bounds[1] - bounds[0])) * (1 + 0.05 * rng.random(n))   # smooth in height, as an atmosphere is
doppler = lambda0 / C0 * np.sqrt(2 * K_B * T / 1.6735575e-27)
gamma = 4.702e8 + 10 ** rng.uniform(6, 10, n)
velocity = rng.normal(0, 8e3, (n, 3))
strat = np.exp(-(z - bounds[0]) / 0.7e6)
strength = 3e-2 * strat * doppler.mean() * (1 + 0.1 * rng.random(n))     # Δτ between neighbours spans the branches
alpha_cont = 1e-4 * strat
lte = np.stack([10 ** rng.uniform(14, 19, n), 10 ** rng.uniform(8, 12, n), 10 ** rng.uniform(10, 16, n)])
Cmat = 10 ** rng.uniform(-2, 4, (n, 3, 3))
for d in range(3):
    Cmat[:, d, d] = 0.0
atom = lte.sum(axis=0)
planck2 = 2 * H_PLANCK * C0 ** 2 / lam ** 5
sig1 = 7.9e-22 * (lam[51:71] / lam[70]) ** 3
sig2 = 1.4e-21 * (lam[71:91] / lam[90]) ** 3
case = vrt.LineCase(lam=lam, blocks=blocks, lambda0=lambda0, c0=C0, velocity=velocity, doppler=doppler,
                    gamma_static=gamma, gamma_unsold=1e-9 * np.ones(n), alpha_cont=alpha_cont,
                    eps=10 ** rng.uniform(-2.5, -0.5, n), temperature=T, atom_density=atom,
                    B0=(1.0 + (z - bounds[0]) / (bounds[1] - bounds[0]))[:, None] * np.ones((1, nlam_all)), lte=lte, C=Cmat,
                    planck2=planck2, sigma_bf1=sig1, sigma_bf2=sig2,
                    strength_const=float(np.median(strength / lte[0])), Bij=1.0, Bji=0.25,
                    sigma_bb_const=H_PLANCK * C0 / (4 * np.pi * lambda0) * 4.5e20, hc_over_kB=H_PLANCK * C0 / K_B,
                    pref_ij=2 * np.pi / (H_PLANCK * C0) / 1000.0, pref_ji=2 * np.pi / (H_PLANCK * C0))

L = _lib.load()
lc, keep = case.c_struct()
h = ctypes.c_void_p()
if args.multi:
    wq, th, ph, _ = vrt.read_quadrature("ul7n12.dat")
    mp = vrt.MultiDevicePlan(pos, nbr, bounds, vrt.quadrature_directions(th, ph), dirs=[1 if t > 90 else -1 for t in th],
                             devices=(0,) * args.multi)
    api.check(L.vrt_multi_lambda_create(mp._h, ctypes.byref(lc), api._d(api._f64(wq)), ctypes.byref(h)))
    prefix = "vrt_multi_lambda"
else:
    plan, wq = api._quadrature_plan(sites, "ul7n12.dat", 3)
    api.check(L.vrt_lambda_create(plan._h, ctypes.byref(lc), api._d(api._f64(wq)), ctypes.byref(h)))
    prefix = "vrt_lambda"
fn = lambda name: getattr(L, f"{prefix}_{name}")
d = ctypes.c_double()


def iterate():
    t0 = time.perf_counter()
    api.check(fn("iterate")(h, ctypes.byref(d)))
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def report(res):
    for k, val in res.items():
        print(k, val)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


for _ in range(3):
    iterate()
off = [iterate() for _ in range(args.reps)]
if not hasattr(L, f"{prefix}_set_acceleration"):         # an older build: (a) is all it has
    fn("destroy")(h)
    report({"library": _lib.LIB_PATH, "members": args.multi, "sites": int(n), "wavelengths": int(nlam_all), "iterate_off": stats(off)})
    (mp if args.multi else sites).close()
    sys.exit(0)
api.check(fn("set_acceleration")(h, 2, 4, 4))
record, step, verdicts = [], [], {1: 0, -1: 0}
applied, coeffs = ctypes.c_int(0), np.zeros(2)
it = 3 + args.reps
while len(step) < args.reps:
    ms = iterate()
    it += 1
    api.check(fn("last_acceleration")(h, ctypes.byref(applied), None, api._d(coeffs)))
    if applied.value:
        if verdicts[1] + verdicts[-1] > 0:          # (the first due iterate: an incomplete history, and the warm-up of the kernels)
            step.append(ms)
        verdicts[applied.value] += 1
    elif it % 4:
        record.append(ms)
api.check(fn("set_acceleration")(h, 0, 0, 0))
off2 = [iterate() for _ in range(args.reps)]
fn("destroy")(h)
if args.multi:
    report({"library": _lib.LIB_PATH, "members": args.multi, "sites": int(n), "wavelengths": int(nlam_all),
            "S_bytes": 8 * n * nlam_all, "iterate_off": stats(off), "iterate_off_after": stats(off2),
            "iterate_recording": stats(record), "iterate_with_step": stats(step), "steps_taken": verdicts[1],
            "steps_rejected": verdicts[-1]})
    mp.close()
    sys.exit(0)

# (d) the standalone entry on arrays of the session's S size
dev = torch.device("cuda", 0)
count = n * nlam_all
gen = torch.Generator(device=dev)
gen.manual_seed(1)
x_star = 1.0 + torch.rand(count, generator=gen, device=dev, dtype=torch.float64)
u = 0.1 * torch.randn(count, generator=gen, device=dev, dtype=torch.float64)
v = 0.1 * torch.randn(count, generator=gen, device=dev, dtype=torch.float64)
xs = [x_star + 0.9 ** k * u + 0.5 ** k * v for k in range(4)]
out = torch.empty_like(x_star)
st = torch.cuda.current_stream().cuda_stream
alone = []
for r in range(args.reps + 2):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ok, sums, co = api.ng_accelerate_dev(count, *(t.data_ptr() for t in xs), out.data_ptr(), st)
    e1.record()
    torch.cuda.synchronize()
    if r >= 2:
        alone.append(e0.elapsed_time(e1))
assert ok and float((out - x_star).abs().max()) < 1e-9
nbytes = 8.0 * count * 8
res = {"sites": int(n), "wavelengths": int(nlam_all), "S_bytes": 8 * count,
       "iterate_off": stats(off), "iterate_off_after": stats(off2), "iterate_recording": stats(record),
       "iterate_with_step": stats(step), "steps_taken": verdicts[1], "steps_rejected": verdicts[-1],
       "ng_accelerate_dev": dict(stats(alone), bytes=nbytes, GBps_at_median=nbytes / statistics.median(alone) / 1e6)}
report(res)
sites.close()
