#!/usr/bin/env python3
"""What aic_find_block_cubes and aic_pick_stale_blocks cost, in ONE GPU command (profiles/stale_blocks_timing.txt).

usage: python tools/measure_stale_blocks.py [--calls 200]

1. The find on bench.py's 256^3 scene (`s256`: a 32 MB grid): info.kernel_ms -- HIP events around the count, and around scan and write -- for a block
   that few cubes hold and for the most common visible block, with capacity for every run; and for the common block with capacity 0 (the count alone:
   merged). Each leg is warmed with 5 calls, then `--calls` blocking calls; 10th percentile, median, 90th. The bytes the rule names,
   2 * 2 * n_cubes(grid) + 24 * n_runs, over the median time, as a share of the 6.3 TB/s a float4 copy reaches on this part.
2. The whole call on the 1920 x 1080 atrium frame of bench.py, resident as an AIC_FRAME_OUT_SPLIT frame, for one redefined block -- the rarest block some
   visible cube holds, a middling one and the most common one in view --: aic_pick_stale_blocks against the only answer there was before,
   aic_pick_stale_cubes with the whole space as one box, alternating call by call in the same process, n = max_stale = 65536, expand = 1. Wall time per
   call, both HIP-event times, and the stale pixels each hands out."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
N = 65536
COPY_RATE = 6.3e12  # bytes/s, a float4 copy on this part


def quantiles(np, v):
    return [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])]


def find_leg(ctx, np, abi, index, capacity, calls):
    for _ in range(5):
        ctx.find_block_cubes(abi.LAYER_WORLD, [index], capacity)
    ks, ws = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        _, info = ctx.find_block_cubes(abi.LAYER_WORLD, [index], capacity)
        ws.append((time.perf_counter() - t0) * 1e3)
        ks.append(info.kernel_ms)
    return info, quantiles(np, ks), quantiles(np, ws)


def measure_find(calls):
    import numpy as np

    import bench
    from all_is_cubes_amd import abi

    sp = bench.build_workload("s256")[0]
    grid = np.asarray(sp.block_index)
    held = np.bincount(grid.reshape(-1), minlength=len(sp.blocks))
    visible = [i for i, b in enumerate(sp.blocks) if not b.is_air and held[i]]
    rare, common = min(visible, key=lambda i: held[i]), max(visible, key=lambda i: held[i])
    print(f"# s256: grid {tuple(grid.shape)}, {grid.size} entries, {len(sp.blocks)} blocks; rarest visible block {rare} ({held[rare]} cubes), most common {common} ({held[common]} cubes)")
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        for name, index, every_run in (("few cubes", rare, True), ("most common visible block", common, True), ("most common, capacity 0 (count alone)", common, False)):
            capacity = int(ctx.find_block_cubes(abi.LAYER_WORLD, [index], 0)[1].n_runs) if every_run else 0  # (the wall time holds the copy of the boxes to the host)
            info, ks, ws = find_leg(ctx, np, abi, index, capacity, calls)
            moved = 2 * 2 * grid.size + 24 * info.n_runs if capacity else 2 * grid.size
            print(f"find, {name:<40} " + json.dumps({"kernel_ms_p10_p50_p90": ks, "wall_ms_p10_p50_p90": ws, "n_cubes": info.n_cubes, "n_runs": info.n_runs, "n_written": info.n_written,
                                                      "merged": info.merged, "bytes": moved, "share_of_copy_rate": round(moved / (ks[1] * 1e-3) / COPY_RATE, 4)}), flush=True)


def measure_pick(calls):
    import numpy as np
    import torch

    import reproject_timing as rt
    from all_is_cubes_amd import abi

    sp, w, h, vd, cams = rt.cameras()
    count = w * h
    projection, view, inv = cams["traced"]
    vp = (view @ projection).reshape(16)
    grid = np.asarray(sp.block_index)
    held = np.bincount(grid.reshape(-1), minlength=len(sp.blocks))
    whole = np.array([[*sp.lo, *sp.hi]], np.int32)
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(bloom_intensity=0.0, view_distance=vd))
        ctx.set_depth_transform(rt.depth_transform(projection, vd))
        frame = ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK)
        src = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(frame, src.data_ptr())
        aux = ctx.render(ctx.make_frame(256, 144, world_inv=inv), want_aux=True)["aux"].reshape(-1)
        hit = np.unique(aux["cube"][aux["hit"] != 0], axis=0).astype(np.int64) - np.asarray(sp.lo, np.int64)
        seen = sorted(set(int(i) for i in grid[hit[:, 0], hit[:, 1], hit[:, 2]]), key=lambda i: held[i])
        # every block some visible cube holds, once: a cube holding it within `expand` of the camera has no rectangle short of the whole frame
        survey = {}
        out1 =torch.zeros(16, dtype=torch.int32, device="cuda")
        for index in seen:
            i = ctx.pick_stale_blocks(vp, w, h, 1, None, None, abi.LAYER_WORLD, [index], 0, 0, out1.data_ptr(), max_stale=1)
            survey[index] = (int(held[index]), int(i.found.n_runs), int(i.pick.n_stale), int(i.pick.whole_frame))
        narrow = [i for i in seen if not survey[i][3]]
        print("# block: (cubes, runs, n_stale, whole_frame) " + json.dumps(survey))
        print(f"# {len(narrow)} of {len(seen)} blocks make fewer than all {count} pixels stale; the others have a cube within one cube of the camera")
        pool = narrow if narrow else seen
        chosen = sorted({pool[0], pool[len(pool) // 2], pool[-1]}, key=lambda i: held[i])
        order, _, _ = abi.pixel_order(w, h)
        order_dev = torch.from_numpy(order.view(np.int32)).cuda()
        out = torch.zeros(N, dtype=torch.int32, device="cuda")
        print(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT; grid {tuple(grid.shape)}, {len(sp.blocks)} blocks, {len(seen)} of them on a visible cube; n = max_stale = {N}; "
              f"{calls} blocking calls per leg, alternating")

        def new(index):
            return ctx.pick_stale_blocks(vp, w, h, N, None, None, abi.LAYER_WORLD, [index], src.data_ptr(), order_dev.data_ptr(), out.data_ptr(), max_stale=N)

        def old():
            return ctx.pick_stale_cubes(vp, w, h, N, whole, None, src.data_ptr(), order_dev.data_ptr(), out.data_ptr(), max_stale=N)

        for index in chosen:
            for _ in range(5):
                new(index), old()
            t = {"new": [], "old": []}
            k = {"find": [], "pick": [], "old": []}
            for _ in range(calls):
                t0 = time.perf_counter()
                a = new(index)
                t1 = time.perf_counter()
                b = old()
                t2 = time.perf_counter()
                t["new"].append((t1 - t0) * 1e3)
                t["old"].append((t2 - t1) * 1e3)
                k["find"].append(a.found.kernel_ms)
                k["pick"].append(a.pick.kernel_ms)
                k["old"].append(b.kernel_ms)
            print(f"block {index} ({held[index]} cubes) " + json.dumps({
                "pick_stale_blocks_wall_ms_p10_p50_p90": quantiles(np, t["new"]), "find_kernel_ms": quantiles(np, k["find"]), "pick_kernel_ms": quantiles(np, k["pick"]),
                "n_runs": a.found.n_runs, "merged": a.found.merged, "n_stale": a.pick.n_stale, "whole_frame": a.pick.whole_frame,
                "whole_space_box_wall_ms_p10_p50_p90": quantiles(np, t["old"]), "whole_space_box_kernel_ms": quantiles(np, k["old"]), "whole_space_box_n_stale": b.n_stale,
                "of_pixels": count, "fewer_stale_pixels": bool(a.pick.n_stale < b.n_stale)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    print(f"# command: python tools/measure_stale_blocks.py --calls {a.calls}")
    measure_find(a.calls)
    measure_pick(a.calls)
    return 0


if __name__ == "__main__":
    sys.exit(main())
