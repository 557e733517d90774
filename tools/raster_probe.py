#!/usr/bin/env python3
"""Raster resampling on the GPU: walk and gather kernel times of Voronoi_to_Raster / _inv_dist on a tessellated grid,
written bytes and their rate, walk statistics, and scipy cKDTree (build + query, 16 workers) on the same points.
usage: timeout -k 10 900 python tools/raster_probe.py [n_sites] [nz nx ny] [nf]     (defaults 1000000 128 256 256 51)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voronoirt_amd as vrt  # noqa: E402

args = [int(a) for a in sys.argv[1:]]
n = args[0] if len(args) > 0 else 1_000_000
nz, nx, ny = args[1:4] if len(args) > 3 else (128, 256, 256)
nf = args[4] if len(args) > 4 else 51

import torch  # noqa: E402

rng = np.random.default_rng(1)
pos = np.ascontiguousarray(rng.random((n, 3)))
bounds = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
t0 = time.time()
nbr = vrt.voro(pos, bounds)
g = vrt.VoronoiSites(pos, nbr, bounds)
print(f"grid: {n} sites tessellated and uploaded in {time.time() - t0:.1f} s")
z, x, y = np.linspace(0, 1, nz), np.linspace(0, 1, nx), np.linspace(0, 1, ny)
P = nz * nx * ny
dF = torch.rand((n, nf), dtype=torch.float64, device="cuda")
dR = torch.empty((nf, ny, nx, nz), dtype=torch.float64, device="cuda")
written = P * nf * 8
for inv in (False, True):
    for periodic in (False, True):
        rows = []
        for rep in range(4):          # the first call builds the cell list and the workspaces
            vrt.Voronoi_to_Raster_dev(g, z, x, y, nf, nf, dF.data_ptr(), dR.data_ptr(), inv_dist=inv, periodic=periodic)
            rows.append(vrt.raster_stats(g))
        st = rows[-1]
        walk = min(r["nearest_ms"] for r in rows[1:])
        gath = min(r["gather_ms"] for r in rows[1:])
        print(f"{'inv_dist' if inv else 'nearest '} {'periodic ' if periodic else 'euclidean'}: {P} points x {nf} "
              f"fields: walk {walk:.3f} ms ({P / walk / 1e6:.2f} Gq/s), gather {gath:.3f} ms, written "
              f"{written / 1e9:.3f} GB = {written / gath / 1e9:.2f} TB/s (store ceiling 6.0-6.3), "
              f"mean walk steps {st['walk_steps'] / st['queries']:.2f}, Euclidean fallback "
              f"{st['fallbacks'] / st['queries']:.4f}")
try:
    from scipy.spatial import cKDTree
    t0 = time.time()
    tree = cKDTree(pos)
    tb = time.time() - t0
    Y, X, Z = np.meshgrid(y, x, z, indexing="ij")
    q = np.stack([Z.ravel(), X.ravel(), Y.ravel()], 1)
    t0 = time.time()
    tree.query(q, k=1, workers=16)
    tq = time.time() - t0
    print(f"cKDTree (16 workers): build {tb * 1e3:.0f} ms, query of {P} points {tq * 1e3:.0f} ms")
except ImportError:
    print("cKDTree: scipy not available")
g.close()
