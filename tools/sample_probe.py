#!/usr/bin/env python3
"""Site sampling on the GPU: time of sample_from_invNH_invT's rejection sampling (vrt_sample_sites_dev, the quantity
already on the device) for the reference's grid sizes, proposals per second and the acceptance rate, beside the
numpy restatement of the same semantics on the host (bit-compared).
usage: timeout -k 10 900 python tools/sample_probe.py [n_sites nz nx ny] ...   (defaults: 1000000 128 256 256 and
       3522560 430 256 256, the author's production size)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voronoirt_amd as vrt  # noqa: E402
from voronoirt_amd import synth  # noqa: E402

args = [int(a) for a in sys.argv[1:]]
cases = [tuple(args[i:i + 4]) for i in range(0, len(args) - 3, 4)] or [(1_000_000, 128, 256, 256),
                                                                       (3_522_560, 430, 256, 256)]

import torch  # noqa: E402


def sample_numpy(z, x, y, q, n, seed, chunk=1 << 22):
    """include/voronoirt.h's semantics in numpy: proposals in chunks, the first n accepted"""
    q_min, dq = q.min(), q.max() - q.min()
    rows, got, j0, used = [], 0, 0, 0

    def itv(ax, v):
        return np.clip(np.searchsorted(ax, v, side="left") - 1, 0, ax.size - 2)
    while got < n:
        j = np.arange(j0, j0 + chunk, dtype=np.uint64)
        u = [synth.counter_uniform(seed, c, j) for c in range(4)]
        zr, xr, yr = u[0] * (z[-1] - z[0]) + z[0], u[1] * (x[-1] - x[0]) + x[0], u[2] * (y[-1] - y[0]) + y[0]
        iz, ix, iy = itv(z, zr), itv(x, xr), itv(y, yr)
        x_d = (xr - x[ix]) / (x[ix + 1] - x[ix])
        y_d = (yr - y[iy]) / (y[iy + 1] - y[iy])
        z_d = (zr - z[iz]) / (z[iz + 1] - z[iz])
        V = lambda a, b, c: q[iy + c, ix + b, iz + a]      # noqa: E731
        c0 = (V(0, 0, 0) * (1 - x_d) + V(0, 1, 0) * x_d) * (1 - y_d) + (V(0, 0, 1) * (1 - x_d) + V(0, 1, 1) * x_d) * y_d
        c1 = (V(1, 0, 0) * (1 - x_d) + V(1, 1, 0) * x_d) * (1 - y_d) + (V(1, 0, 1) * (1 - x_d) + V(1, 1, 1) * x_d) * y_d
        take = np.nonzero(c0 * (1 - z_d) + c1 * z_d > u[3] * dq + q_min)[0][: n - got]
        rows.append(np.stack([zr[take], xr[take], yr[take]], 1))
        got += take.size
        used = j0 + int(take[-1]) + 1 if got == n else used
        j0 += chunk
    return np.concatenate(rows), used


for n, nz, nx, ny in cases:
    t0 = time.time()
    a = synth.atmosphere_raster(nz, nx, ny, seed=1)
    inv = 1.0 / np.log10(a["N_H"])
    q = (inv * inv) * a["T"] ** (-0.4)
    z, x, y = a["z"], a["x"], a["y"]
    del a, inv
    print(f"raster {nz} x {nx} x {ny} ({q.nbytes / 2**20:.0f} MiB), invNH_invT quantity built in {time.time() - t0:.1f} s")
    dq = torch.as_tensor(q.ravel(), device="cuda")
    dpos = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    used = vrt.rejection_sampling_dev(n, z, x, y, dq.data_ptr(), 8, dpos.data_ptr())      # warm-up (code objects)
    times = []
    for rep in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        used = vrt.rejection_sampling_dev(n, z, x, y, dq.data_ptr(), 8, dpos.data_ptr())  # synchronous
        times.append((time.perf_counter() - t0) * 1e3)
    ms = min(times)
    print(f"  device: {n} sites, {used} proposals, acceptance {n / used:.4f}: best {ms:.2f} ms, median "
          f"{sorted(times)[len(times) // 2]:.2f} ms of 5 ({used / ms / 1e6:.2f} G proposals/s), whole call incl. "
          f"min/max reduction, workspace allocation and one int64 read per batch")
    t0 = time.perf_counter()
    host = vrt.rejection_sampling(n, z, x, y, q, 8)
    th = (time.perf_counter() - t0) * 1e3
    print(f"  host form (quantity uploaded, positions downloaded): {th:.1f} ms")
    t0 = time.perf_counter()
    ref, ref_used = sample_numpy(z, x, y, q, n, 8)
    tn = time.perf_counter() - t0
    same = (np.array_equal(dpos.cpu().numpy().view(np.int64), ref.view(np.int64)) and ref_used == used
            and np.array_equal(host.view(np.int64), ref.view(np.int64)))
    print(f"  numpy restatement on the host (one thread): {tn * 1e3:.0f} ms ({ref_used / tn / 1e6:.2f} M proposals/s); "
          f"bit-equal to the device: {same}")
    del dq, dpos
    torch.cuda.empty_cache()
