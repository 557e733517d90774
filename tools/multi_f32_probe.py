#!/usr/bin/env python3
"""diagnostics: what float storage buys the MULTI-device line Λ-iteration session at the C4 session size of
tools/accel_probe.py (995 566 sites, ul7n12, 51 line + 2 x 20 continuum wavelengths), with device 0 listed once and twice:

  for vrt_multi_lambda_create and vrt_multi_lambda_create_f32
    the device memory the create takes (hipMemGetInfo before and after it, the members' plans already made), and
    the wall time of vrt_multi_lambda_iterate (it returns when every stream is idle: only the criterion's scalar comes
    back), median and min..max over the repeats after a warm-up;
  beside them the iterate of the one-device float session (vrt_lambda_create_f32) on the same case.

    python tools/multi_f32_probe.py [--a 59 --c 143] [--reps 5] [--json out.json]

The phases of an iterate (opacity, sweep, update, shares, the adds and copies of the shares between members of one
device): run this under `rocprofv3 --kernel-trace --stats -- python tools/multi_f32_probe.py --reps 2`.
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
ap.add_argument("--reps", type=int, default=5, help="timed iterates per session, after one warm-up")
ap.add_argument("--json", default="")
args = ap.parse_args()

pos, nbr, bounds = synth.bcc_grid(args.a, args.c, seed=2022)
n = pos.shape[0]
rng = np.random.default_rng(7)
nbb, nbf = 51, 20
lambda0 = 121.567e-9
q = np.concatenate([-np.geomspace(600, 0.05, nbb // 2), [0.0], np.geomspace(0.05, 600, nbb // 2)])
lam = np.concatenate([lambda0 * (1 + q * 2.5e3 / C0), np.linspace(22.8e-9, 91.17e-9, nbf), np.linspace(91.2e-9, 364.7e-9, nbf)])
blocks = np.array([0, nbb, nbb, nbb + nbf, nbb + nbf, nbb + 2 * nbf], dtype=np.int64)
nlam = lam.size
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
case = vrt.LineCase(lam=lam, blocks=blocks, lambda0=lambda0, c0=C0, velocity=velocity, doppler=doppler,
                    gamma_static=gamma, gamma_unsold=1e-9 * np.ones(n), alpha_cont=alpha_cont,
                    eps=10 ** rng.uniform(-2.5, -0.5, n), temperature=T, atom_density=lte.sum(axis=0),
                    B0=(1.0 + (z - bounds[0]) / (bounds[1] - bounds[0]))[:, None] * np.ones((1, nlam)), lte=lte, C=Cmat,
                    planck2=2 * H_PLANCK * C0 ** 2 / lam ** 5, sigma_bf1=7.9e-22 * (lam[51:71] / lam[70]) ** 3,
                    sigma_bf2=1.4e-21 * (lam[71:91] / lam[90]) ** 3,
                    strength_const=float(np.median(strength / lte[0])), Bij=1.0, Bji=0.25,
                    sigma_bb_const=H_PLANCK * C0 / (4 * np.pi * lambda0) * 4.5e20, hc_over_kB=H_PLANCK * C0 / K_B,
                    pref_ij=2 * np.pi / (H_PLANCK * C0) / 1000.0, pref_ji=2 * np.pi / (H_PLANCK * C0))

L = _lib.load()
lc, keep = case.c_struct()
wq, th, ph, _ = vrt.read_quadrature("ul7n12.dat")
w_ptr = api._d(api._f64(wq))


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]        # hipMemGetInfo


def timed(prefix, h):
    it, d = getattr(L, prefix + "_iterate"), ctypes.c_double()
    api.check(it(h, ctypes.byref(d)))           # warm-up: first launches, workspaces
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        api.check(it(h, ctypes.byref(d)))
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms), criterion=d.value)


res = dict(sites=int(n), nlam=int(nlam), angles=int(len(wq)), sessions=[])
print(f"{n} sites, {len(wq)} angles, {nlam} wavelengths; {args.reps} timed iterates after one warm-up", flush=True)
for members in ((0,), (0, 0)):
    mp = vrt.MultiDevicePlan(pos, nbr, bounds, vrt.quadrature_directions(th, ph), dirs=[1 if t > 90 else -1 for t in th],
                             devices=members)
    for storage, create in (("f64", L.vrt_multi_lambda_create), ("f32", L.vrt_multi_lambda_create_f32)):
        h = ctypes.c_void_p()
        before = free_bytes()
        api.check(create(mp._h, ctypes.byref(lc), w_ptr, ctypes.byref(h)))
        taken = before - free_bytes()
        r = dict(session="multi", members=len(members), storage=storage, create_MiB=taken / 2 ** 20, **timed("vrt_multi_lambda", h))
        L.vrt_multi_lambda_destroy(h)
        res["sessions"].append(r)
        print(f"multi, device 0 x {len(members)}, {storage}: create takes {r['create_MiB']:9.1f} MiB; iterate {r['median_ms']:8.1f} ms "
              f"({r['min_ms']:.1f} .. {r['max_ms']:.1f})", flush=True)
    mp.close()
sites = vrt.VoronoiSites(pos, nbr, bounds, device=0)
plan, _ = api._quadrature_plan(sites, "ul7n12.dat", 3)
h = ctypes.c_void_p()
before = free_bytes()
api.check(L.vrt_lambda_create_f32(plan._h, ctypes.byref(lc), w_ptr, ctypes.byref(h)))
taken = before - free_bytes()
r = dict(session="one-device", members=1, storage="f32", create_MiB=taken / 2 ** 20, **timed("vrt_lambda", h))
L.vrt_lambda_destroy(h)
res["sessions"].append(r)
print(f"one-device session,        f32: create takes {r['create_MiB']:9.1f} MiB; iterate {r['median_ms']:8.1f} ms "
      f"({r['min_ms']:.1f} .. {r['max_ms']:.1f})", flush=True)
plan.close()
sites.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
