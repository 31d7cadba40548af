#!/usr/bin/env python3
"""What aic_replace_cube_grid costs beside the path a device-made world took before it, in ONE GPU command (profiles/grid_replace_timing.txt,
DESIGN.md 4.23).

usage: python tools/grid_replace_timing.py [--calls 20]

Grids: bench.py's 256^3 synthetic scene (`s256`: a 32 MB grid) and the atrium of tools/reproject_timing.py. Changes: none, 1 % of the cubes scattered, a
16^3 box, every cube. A change is the step between two grids A and B held as torch tensors on the device; the arms alternate call by call in the same
process, the replace always stepping A -> B and the old path B -> A, so both move the same cubes:

  1. aic_replace_cube_grid(B): info.kernel_ms -- HIP events around its launches -- and the wall time of the blocking call, boxes to the host included.
  2. what there was before: the tensor copied to the host, then aic_upload_space of the space with it (`upload`); and for the partial changes the cheaper
     answer of a host that keeps its own copy and compares: the copy, the comparison, aic_update_cubes of the cubes that differ (`update_cubes`).
  3. a device-to-device copy of the 2 n bytes of the grid, torch events around it: the copy rate the passes are measured against.

The traffic the passes name: the count reads 4 bytes a cube (the grid and the array); the store reads 2 and writes 2 in the workgroups that hold a
change; the boxes' write reads 4 a cube in the workgroups that hold a run's start or end; OPEN (launch_open_cubes over the whole grid, whenever anything
changed) reads a cube and its six neighbours, 2 bytes each from cache lines shared along z, and writes the few tags that move. kernel_ms of "none" is
the count alone, so the other rows' kernel_ms less that one is what store, boxes and OPEN cost together."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)


def quantiles(np, v):
    return [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])]


def changes(np, sp):
    """name -> grid B for the space's grid A"""
    a = np.asarray(sp.block_index)
    n_blocks = len(sp.blocks)
    rng = np.random.default_rng(1)
    out = {"none": a.copy()}
    b = a.copy()
    pick = rng.random(a.shape) < 0.01
    b[pick] = (b[pick] + 1) % n_blocks
    out["1 % scattered"] = b
    b = a.copy()
    lo = [max(0, s // 2 - 8) for s in a.shape]
    box = tuple(slice(l, min(l + 16, s)) for l, s in zip(lo, a.shape))
    b[box] = (b[box] + 1) % n_blocks
    out["a 16^3 box"] = b
    out["everything"] = (a + 1) % n_blocks
    return out


def measure(name, sp, calls):
    import copy

    import numpy as np
    import torch

    from all_is_cubes_amd import abi

    W = abi.LAYER_WORLD
    a = np.ascontiguousarray(sp.block_index, np.uint16)
    n = a.size
    dev = torch.device("cuda", 0)
    ta = torch.from_numpy(a.reshape(-1).view(np.int16)).to(dev)
    spare = torch.empty_like(ta)
    print(f"# {name}: grid {tuple(a.shape)}, {n} entries ({2 * n / 1e6:.1f} MB), {len(sp.blocks)} blocks; {calls} blocking calls per leg, alternating", flush=True)
    with abi.Context(0) as ctx:
        ctx.upload_space(W, sp)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        copies = []
        for k in range(calls + 3):
            e0.record()
            spare.copy_(ta)
            e1.record()
            torch.cuda.synchronize()
            if k >= 3:
                copies.append(e0.elapsed_time(e1))
        copy_ms = quantiles(np, copies)
        rate = 2 * 2 * n / (copy_ms[1] * 1e-3)  # the copy reads 2 n bytes and writes 2 n
        print(f"copy  {name:<10} " + json.dumps({"d2d_ms_p10_p50_p90": copy_ms, "bytes_moved": 4 * n, "copy_rate_TBps": round(rate / 1e12, 3)}), flush=True)
        for what, b in changes(np, sp).items():
            tb = torch.from_numpy(np.ascontiguousarray(b).reshape(-1).view(np.int16)).to(dev)
            torch.cuda.synchronize()
            differ = np.argwhere(a != b)
            partial = 0 < len(differ) < n // 2
            spa, spb = copy.copy(sp), copy.copy(sp)
            spa.block_index, spb.block_index = a.copy(), b.copy()
            host = b.copy()  # the old path's own copy of the grid, for its comparison
            capacity = max(int(ctx.replace_cube_grid(W, tb, capacity=0)[1]["n_runs"]), 1)
            ctx.replace_cube_grid(W, ta, capacity=0)
            k_ms, wall, old_upload, old_cubes = [], [], [], []
            info = None
            for k in range(calls + 2):
                t0 = time.perf_counter()
                _, info = ctx.replace_cube_grid(W, tb, capacity=capacity)  # A -> B
                t1 = time.perf_counter()
                if partial:  # B -> A through the host: the copy, the comparison, the scatter
                    back = ta.cpu().numpy().view(np.uint16).reshape(a.shape)
                    at = np.argwhere(back != host)
                    ctx.update_cubes(W, at + np.asarray(sp.lo), back[tuple(at.T)])
                    t2 = time.perf_counter()
                    ctx.replace_cube_grid(W, tb, capacity=0)  # (B again for the next leg, not timed)
                t3 = time.perf_counter()
                back = ta.cpu().numpy().view(np.uint16).reshape(a.shape)  # B -> A through the host: the copy and a whole upload
                spa.block_index = back
                ctx.upload_space(W, spa)
                t4 = time.perf_counter()
                if k >= 2:
                    k_ms.append(info["kernel_ms"])
                    wall.append((t1 - t0) * 1e3)
                    old_upload.append((t4 - t3) * 1e3)
                    if partial:
                        old_cubes.append((t2 - t1) * 1e3)
            km, wm = quantiles(np, k_ms), quantiles(np, wall)
            row = {"replace_kernel_ms_p10_p50_p90": km, "replace_wall_ms_p10_p50_p90": wm, "n_cubes": info["n_cubes"], "n_runs": info["n_runs"],
                   "n_written": info["n_written"], "d2h_upload_space_wall_ms_p10_p50_p90": quantiles(np, old_upload),
                   "kernel_over_d2d_copy": round(km[1] / copy_ms[1], 2), "upload_over_replace_wall": round(float(np.median(old_upload)) / wm[1], 1)}
            if partial:
                row["d2h_compare_update_cubes_wall_ms_p10_p50_p90"] = quantiles(np, old_cubes)
                row["update_cubes_over_replace_wall"] = round(float(np.median(old_cubes)) / wm[1], 1)
            print(f"{name:<6} {what:<14} " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--grids", default="s256,atrium")
    args = ap.parse_args()
    print(f"# command: python tools/grid_replace_timing.py --calls {args.calls} --grids {args.grids}")
    for name in args.grids.split(","):
        if name == "s256":
            import bench

            sp = bench.build_workload("s256")[0]
        else:
            import reproject_timing as rt

            sp = rt.cameras()[0]
        measure(name, sp, args.calls)
    return 0


if __name__ == "__main__":
    sys.exit(main())
