#!/usr/bin/env python3
"""Emergent spectrum on the GPU at a user-sized raster: device-event times of its three stages -- raster opacity and
source function (vrt_synth_opacity_dev), top-plane intensity (vrt_regular_emergent_dev), τ = 1 heights
(vrt_tau_unity_dev) -- with their algorithmic bytes (each input read once, each output written once), Voigt
evaluations, and the share of the MI355X's HBM peak (8 TB/s) the bytes would reach.
usage: timeout -k 10 600 python tools/synth_probe.py [nz nx ny] [nlam] [chunk]     (defaults 200 256 256 70 12)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voronoirt_amd as vrt  # noqa: E402
from voronoirt_amd import synth  # noqa: E402

import torch  # noqa: E402

args = [int(a) for a in sys.argv[1:]]
nz, nx, ny = args[0:3] if len(args) >= 3 else (200, 256, 256)
nlam = args[3] if len(args) > 3 else 70
chunk = args[4] if len(args) > 4 else 12
HBM = 8.0e12

atm = synth.atmosphere_raster(nz, nx, ny, seed=1)
raster, pops, case, src = synth.line_raster(atm, nlam, seed=1)
z, x, y = raster["z"], raster["x"], raster["y"]
vol, volg = nz * nx * ny, nz * (nx + 2) * (ny + 2)
dev = torch.device("cuda", 0)
d_f = {n: torch.from_numpy(np.ascontiguousarray(raster[n], dtype=np.float64)).to(dev) for n in vrt.api.SYNTH_FIELDS}
ptr = {n: t.data_ptr() for n, t in d_f.items()}
d_pops = torch.from_numpy(np.ascontiguousarray(pops)).to(dev)
d_S = torch.empty((chunk, ny + 2, nx + 2, nz), dtype=torch.float64, device=dev)
d_A = torch.empty_like(d_S)
I_top = torch.empty((nlam, ny, nx), dtype=torch.float64, device=dev)
H = torch.empty_like(I_top)
solver = vrt.RegularSolver(z, vrt.periodic_axis(x), vrt.periodic_axis(y))
print(f"raster {nz} x {nx} x {ny} ({volg} points with the ghost border), {nlam} wavelengths in chunks of {chunk}")
for th, ph in ((180.0, 0.0), (130.0, 35.0)):
    k = vrt.direction(th, ph)
    ms = {"opacity": 0.0, "emergent": 0.0, "tau": 0.0}
    for rep in range(2):                       # the first pass grows the solver's workspaces
        for s in ms:
            ms[s] = 0.0
        for l0 in range(0, nlam, chunk):
            nc = min(chunk, nlam - l0)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            vrt.synth_opacity_dev(k, nz, nx, ny, case, src, ptr, d_pops.data_ptr(), d_S.data_ptr(), d_A.data_ptr(),
                                  lam=case.lam[l0:l0 + nc], planck2=case.planck2[l0:l0 + nc])
            ev[1].record()
            vrt.top_intensity_dev(solver, k, nc, d_S.data_ptr(), d_A.data_ptr(), I_top[l0].data_ptr())
            ev[2].record()
            vrt.tau_unity_dev(k, z, x, y, nc, d_A.data_ptr(), H[l0].data_ptr())
            ev[3].record()
            torch.cuda.synchronize()
            ms["opacity"] += ev[0].elapsed_time(ev[1])
            ms["emergent"] += ev[1].elapsed_time(ev[2])
            ms["tau"] += ev[2].elapsed_time(ev[3])
    assert torch.isfinite(I_top).all() and torch.isfinite(H).all()
    nlaunch = sum((min(chunk, nlam - l0) + 31) // 32 for l0 in range(0, nlam, chunk))
    by = {"opacity": 8 * (10 * vol * nlaunch + 2 * volg * nlam),       # 10 input fields per launch, S + alpha out
          "emergent": 8 * (2 * volg * nlam + nx * ny * nlam),          # S + alpha in, the top plane out
          "tau": 8 * (volg * nlam + nx * ny * nlam)}                    # alpha in, the heights out
    print(f"theta {th:5.1f} phi {ph:5.1f}:")
    for s in ms:
        t = ms[s] * 1e-3
        extra = f", {volg * nlam / t:.3g} Voigt evaluations/s" if s == "opacity" else ""
        print(f"  {s:9s} {ms[s]:9.2f} ms  {by[s] / 1e9:7.2f} GB algorithmic  {by[s] / t / 1e12:6.3f} TB/s = "
              f"{100 * by[s] / t / HBM:5.1f} % of HBM peak{extra}")
    print(f"  I_top mean {I_top.mean().item():.4g}, tau=1 heights {H.min().item():.4g} .. {H.max().item():.4g}")
solver.close()
