#!/usr/bin/env python3
"""diagnostics: how the workgroups of the per-layer patch launches fill and leave the chip (profiles/order/INDEX.md).
Needs the -DVRT_DIAG build of the library (python voronoirt_amd/build.py --diag; select it with VRT_LIB_PATH): with option
VRT_PATCH_TIMELINE=1 every patch and reduction block of a per-layer launch leaves its start stamp, its end stamp
(wall_clock64) and its share in pair steps (vrt_patch.hip: BlockStamp).  This tool runs a workload of bench.py (same grid,
quadrature, fields and entry point: sweep-order S / J, per-angle alpha in the plan's layout) for a few steps and turns the
LAST step into per-launch figures:
  last start   the start of the launch's last-started block, from the launch's first start
  late         blocks that started after the launch's first block had ended (they waited for a slot)
  tail         from the first end of a patch block to the launch's last end
  last-ender   share of the block that ended last, whether it was a late one, and the longest share of the launch
  patch blocks when the patch blocks start (median, 90 %, last), how many of them late, how long a longest / shortest share runs
  fill         slot time used: sum of the blocks' durations over (--slots x the launch's duration)
  riding       with the J reduction riding in the patch blocks (VRT_PATCH_REDUCE_RIDE=1): the blocks that took a slice, their
               elements (chunks x threads), and when they stored J_dir, from their own start
usage: VRT_LIB_PATH=voronoirt_amd/libvrt_hip_diag.so python tools/patch_timeline.py [--workload C4] [--nlam L] [--order 0|1]
       [--split S] [--ride 0|1] [--steps 3] [--slots 512] [--csv per_launch.csv]"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import voronoirt_amd as vrt  # noqa: E402
from bench import WORKLOADS  # noqa: E402
from voronoirt_amd import _lib, synth  # noqa: E402
from voronoirt_amd.api import check  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4", choices=sorted(WORKLOADS))
    ap.add_argument("--nlam", type=int, default=0)
    ap.add_argument("--order", type=int, default=-1, help="VRT_PATCH_ORDER (-1: the library's default)")
    ap.add_argument("--split", type=int, default=0, help="VRT_PATCH_SPLIT (0: the split rule)")
    ap.add_argument("--ride", type=int, default=-1, help="VRT_PATCH_REDUCE_RIDE (-1: the library's default)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=512, help="workgroup slots a launch is measured against (a stream's half of 1024)")
    ap.add_argument("--csv", default="")
    args = ap.parse_args()
    a, c, quad, nlam, per_angle, seed = WORKLOADS[args.workload]
    nlam = args.nlam or nlam
    dev = torch.device("cuda", 0)
    w, theta, phi, nq = vrt.read_quadrature(quad)
    pos, nbr, bounds = synth.bcc_grid(a, c, seed=seed)
    sites = vrt.VoronoiSites(pos, nbr, bounds, device=0)
    n = sites.n
    dirs = np.array([1 if t > 90 else (-1 if t < 90 else 0) for t in theta])
    plan = vrt.FormalPlan(sites, vrt.quadrature_directions(theta, phi), 3, dirs=dirs)
    plan.set_option("VRT_PATCH_CHAIN", 0)
    plan.set_option("VRT_PATCH_TIMELINE", 1)
    if args.order >= 0:
        plan.set_option("VRT_PATCH_ORDER", args.order)
    if args.split > 0:
        plan.set_option("VRT_PATCH_SPLIT", args.split)
    if args.ride >= 0:
        plan.set_option("VRT_PATCH_REDUCE_RIDE", args.ride)
    # the fields of bench.py (synthetic stratified atmosphere, a line profile per angle)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    z = torch.as_tensor(pos[:, 0], device=dev)
    z_min, z_max = bounds[0], bounds[1]
    lam = torch.arange(nlam, device=dev, dtype=torch.float64)
    centre, sigma = 0.5 * (nlam - 1), max(nlam / 6.0, 1.0)
    S = (1.0 + 0.5 * torch.sin(2 * np.pi * (z - z_min) / (z_max - z_min))[:, None]
         + 0.1 * torch.rand((n, nlam), generator=gen, device=dev, dtype=torch.float64)).contiguous()
    strat = 1.0e-2 * torch.exp(-(z - z_min) / 0.7e6)
    st = torch.cuda.current_stream().cuda_stream
    cnt = plan.native_plane_count(nlam)
    if per_angle:
        alpha_native = torch.empty(plan.native_alpha_count(nlam), device=dev, dtype=torch.float64)
        alpha = torch.empty((nq, n, nlam), device=dev, dtype=torch.float64)
        for ai in range(nq):
            psi = 1.0 + 9.0 * torch.exp(-((lam - centre - 0.15 * sigma * np.cos(2 * np.pi * ai / nq)) / sigma) ** 2)
            alpha[ai] = strat[:, None] * (1.0 + 0.1 * torch.rand((n, nlam), generator=gen, device=dev, dtype=torch.float64)) * psi[None, :]
        plan.alpha_to_native_dev(nlam, nlam, alpha.data_ptr(), alpha_native.data_ptr(), stream=st)
        mode = _lib.ALPHA_ANGLE_NATIVE
    else:
        psi = 1.0 + 9.0 * torch.exp(-((lam - centre) / sigma) ** 2)
        alpha = (strat[:, None] * (1.0 + 0.1 * torch.rand((n, nlam), generator=gen, device=dev, dtype=torch.float64)) * psi[None, :]).contiguous()
        alpha_native = torch.empty(2 * cnt, device=dev, dtype=torch.float64)
        plan.to_native_dev(nlam, nlam, alpha.data_ptr(), alpha_native.data_ptr(), alpha_native.data_ptr() + 8 * cnt, stream=st)
        mode = _lib.ALPHA_SITE_LAM_NATIVE
    torch.cuda.synchronize()
    del alpha
    bottom = torch.as_tensor(sites.perm_up[:int(sites.layers_up[1] - 1)] - 1, device=dev)
    I0_up = S[bottom].contiguous()
    S_nat = [torch.empty(cnt, device=dev, dtype=torch.float64) for _ in range(2)]
    J_nat = [torch.zeros(cnt, device=dev, dtype=torch.float64) for _ in range(2)]
    plan.to_native_dev(nlam, nlam, S.data_ptr(), S_nat[0].data_ptr(), S_nat[1].data_ptr(), stream=st)
    torch.cuda.synchronize()
    for _ in range(max(1, args.steps)):
        plan.execute_native_dev(nlam, S_nat[0].data_ptr(), S_nat[1].data_ptr(), alpha_native.data_ptr(), mode, w,
                                dJ_up=J_nat[0].data_ptr(), dJ_down=J_nat[1].data_ptr(), dI0_up=I0_up.data_ptr(), stream=st)
        torch.cuda.synchronize()
    plan.check()
    ms, launches = plan.last_sweep_timing()

    cap_l, cap_b = 4096, 1 << 20
    rec = np.zeros((cap_l, 12), dtype=np.int64)
    stamps = np.zeros((cap_b, 3), dtype=np.uint64)
    counts = (ctypes.c_int64 * 3)()
    check(_lib.load().vrt_plan_patch_timeline(plan._h, cap_l, cap_b, rec.ctypes.data_as(_lib.p_i64),
                                              stamps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), counts))
    nl, nb, khz = (int(v) for v in counts)
    us = 1e3 / khz                                    # microseconds per tick
    print(f"# {args.workload}: {n} sites x {nq} angles x {nlam} wavelengths; last of {args.steps} steps: {ms:.3f} ms by the plan's events "
          f"(diagnostics build, stamps on), {launches} launches, {nl} recorded, {nb} blocks, wall clock {khz} kHz")
    rows = []
    for L in rec[:nl]:
        layer, group, gx, gy, nrow, nsplit, lgs, order, prow, nred, first, steps = (int(v) for v in L)
        s = stamps[first:first + gx * gy]
        t0, t1, sh = s[:, 0].astype(np.int64), s[:, 1].astype(np.int64), s[:, 2]
        is_red = ((sh >> np.uint64(32)) & np.uint64(1)) != 0
        share = (sh & np.uint64(0xFFFFFFFF)).astype(np.int64)
        rode = ((sh >> np.uint64(33)) & np.uint64(0x3FFF)).astype(np.int64)      # elements of a riding slice (BlockStamp::rode)
        rode_at = (sh >> np.uint64(48)).astype(np.int64)                         #   and the ticks from the block's start to its J store
        work = is_red | (share > 0) | (rode > 0)       # blocks that did something (padding returns at once)
        if not work.any():
            continue
        begin = t0.min()
        dur = (t1.max() - begin) * us
        patch = work & ~is_red
        first_end = t1[patch].min() if patch.any() else t1[work].min()
        late = work & (t0 > first_end)
        last = int(np.argmax(np.where(work, t1, -1)))
        rows.append(dict(layer=layer, group=group, order=order, nrow=nrow, nsplit=nsplit, blocks=int(work.sum()),
                         patch_blocks=int(patch.sum()), dur=dur, last_start=(t0[work].max() - begin) * us,
                         late=int(late.sum()), late_long=int((late & patch & (share == share[patch].max())).sum()) if patch.any() else 0,
                         tail=(t1.max() - first_end) * us, last_share=int(share[last]), last_is_red=bool(is_red[last]),
                         last_is_late=bool(late[last]), max_share=int(share[patch].max()) if patch.any() else 0,
                         min_share=int(share[patch].min()) if patch.any() else 0,
                         start_p50=float(np.percentile(t0[patch] - begin, 50) * us) if patch.any() else 0.0,
                         start_p90=float(np.percentile(t0[patch] - begin, 90) * us) if patch.any() else 0.0,
                         start_max=float((t0[patch].max() - begin) * us) if patch.any() else 0.0,
                         late_patch=int((late & patch).sum()),
                         last_ender_start=float((t0[last] - begin) * us), last_ender_run=float((t1[last] - t0[last]) * us),
                         run_long=float(((t1 - t0)[patch & (share == share[patch].max())]).mean() * us) if patch.any() else 0.0,
                         run_short=float(((t1 - t0)[patch & (share == share[patch].min())]).mean() * us) if patch.any() else 0.0,
                         fill=float(((t1 - t0)[work]).sum() * us / (args.slots * dur)) if dur > 0 else 0.0,
                         rode_blocks=int((rode > 0).sum()), rode_elements=int(rode.max()),
                         rode_idle=int(((rode > 0) & (share == 0)).sum()),
                         rode_at_p50=float(np.percentile(rode_at[rode > 0], 50) * us) if (rode > 0).any() else 0.0,
                         rode_at_max=float(rode_at[rode > 0].max() * us) if (rode > 0).any() else 0.0,
                         begin=begin * us, end=t1.max() * us))
    if args.csv:
        import csv
        with open(args.csv, "w", newline="") as f:
            wr = csv.DictWriter(f, fieldnames=list(rows[0]))
            wr.writeheader()
            wr.writerows(rows)
    solve = [r for r in rows if r["patch_blocks"] > 0]
    if not solve:
        sys.exit("no per-layer launch with patch blocks was recorded (chained launch, or VRT_PATCH_TIMELINE ignored: not the diagnostics build?)")
    print(f"step by the stamps: {(max(r['end'] for r in rows) - min(r['begin'] for r in rows)) / 1e3:.3f} ms from the first start to the last end")
    mean = lambda k, rs: float(np.mean([r[k] for r in rs]))
    for g in sorted({r["group"] for r in solve}):
        rs = [r for r in solve if r["group"] == g]
        uneven = [r for r in rs if r["max_share"] > r["min_share"]]
        print(f"stream group {g}: {len(rs)} launches with patch blocks, order {rs[0]['order']}, splits {sorted({r['nsplit'] for r in rs})}, "
              f"blocks {mean('blocks', rs):.0f} ({mean('patch_blocks', rs):.0f} patch)")
        print(f"  duration {mean('dur', rs):.2f} us   last start {mean('last_start', rs):.2f} us   late blocks {mean('late', rs):.1f} "
              f"(of them with the longest share {mean('late_long', rs):.1f})   tail {mean('tail', rs):.2f} us   fill {mean('fill', rs):.3f} of {args.slots} slots")
        print(f"  patch blocks: start at {mean('start_p50', rs):.2f} us (median) / {mean('start_p90', rs):.2f} (90 %) / {mean('start_max', rs):.2f} (last), "
              f"{mean('late_patch', rs):.1f} of them late; a longest share runs {mean('run_long', rs):.2f} us, a shortest {mean('run_short', rs):.2f} us")
        print(f"  the last-ending block started at {mean('last_ender_start', rs):.2f} us and ran {mean('last_ender_run', rs):.2f} us")
        if any(r["rode_blocks"] for r in rs):
            print(f"  riding reduction: {mean('rode_blocks', rs):.0f} blocks took a slice ({mean('rode_idle', rs):.1f} of them with no pair step), at most "
                  f"{max(r['rode_elements'] for r in rs)} elements a block; J stored {mean('rode_at_p50', rs):.2f} us (median) / "
                  f"{max(r['rode_at_max'] for r in rs):.2f} us (latest) after the block's start")
        if uneven:
            print(f"  last-ending block, {len(uneven)} launches with uneven shares: longest share in {np.mean([r['last_share'] == r['max_share'] and not r['last_is_red'] for r in uneven]):.2f}, "
                  f"a late block in {np.mean([r['last_is_late'] for r in uneven]):.2f}, late AND longest in "
                  f"{np.mean([r['last_is_late'] and r['last_share'] == r['max_share'] and not r['last_is_red'] for r in uneven]):.2f}, a reduction block in {np.mean([r['last_is_red'] for r in uneven]):.2f}")
    plan.close()
    sites.close()


if __name__ == "__main__":
    main()
