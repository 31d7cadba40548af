#!/usr/bin/env python3
"""What aic_pick_pixels costs beside the host path it replaces, in ONE GPU command (profiles/pick_timing.txt).

usage: python tools/pick_timing.py [--calls 40] [--parent DIR [--bench-steps 30]]
       rocprofv3 --kernel-trace --stats -d DIR -o pick -- python tools/pick_timing.py --profile-leg     (a run of its own: the time per kernel)
       python tools/pick_timing.py --kernel-stats DIR                                                   (prints that run's table)

The 1920 x 1080 atrium frame of bench.py resident in device memory as an AIC_FRAME_OUT_SPLIT frame and reprojected by tools/reproject_timing.py's yaw of
0.02 rad, the picker's order resident beside it. The legs, alternating call by call after 5 calls of warm-up each, every call blocking:
aic_pick_pixels with n = 65536, once with max_unknown = n and once with max_unknown = 0; the host path INTEGRATION.md had before --
PixelPicker.take(65536) and the pageable copy of the list to the device --; and aic_reproject_split itself, for scale. Wall time per call and, where the
call has one, the HIP-event time: 10th percentile, median, 90th.

With --parent (a built checkout of the parent commit): `bench.py --gpus 1 --no-cpu-baseline` of the parent, this tree, the parent, this tree."""
import argparse
import glob
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
N = 65536


def measure(calls, profile_leg):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import reproject_timing as rt
    from all_is_cubes_amd import _host as H
    from all_is_cubes_amd import abi

    sp, w, h, vd, cams = rt.cameras()
    count = w * h
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(bloom_intensity=0.0, view_distance=vd))
        ctx.set_depth_transform(rt.depth_transform(cams["traced"][0], vd))
        flags = abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK
        src = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(ctx.make_frame(w, h, world_inv=cams["traced"][2], flags=flags), src.data_ptr())
        m, zw = rt.reprojection(cams["traced"], cams["yaw 0.02 rad"])
        order, central, cycle = abi.pixel_order(w, h)
        order_dev = torch.from_numpy(order.view(np.int32)).cuda()
        out = torch.zeros(N, dtype=torch.int32, device="cuda")
        picker = H.PixelPicker(w, h)
        rinfo = ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr())

        def host_path():
            pixels = torch.from_numpy(picker.take(N).view(np.int32)).cuda()
            torch.cuda.synchronize()
            return pixels

        legs = {
            f"aic_pick_pixels, n = {N}, max_unknown = n": lambda: ctx.pick_pixels(w, h, N, order_dev.data_ptr(), out.data_ptr(), max_unknown=N),
            f"aic_pick_pixels, n = {N}, max_unknown = 0": lambda: ctx.pick_pixels(w, h, N, order_dev.data_ptr(), out.data_ptr()),
            f"host: PixelPicker.take({N}) and the copy to the device": host_path,
            "aic_reproject_split, yaw 0.02 rad": lambda: ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr()),
        }
        torch.cuda.synchronize()
        if profile_leg:
            for _ in range(10):
                for name, call in legs.items():
                    if name.startswith("aic_pick_pixels"):
                        call()
            return
        for call in legs.values():
            for _ in range(5):
                call()
        wall = {name: [] for name in legs}
        kernel = {name: [] for name in legs}
        last = {}
        for _ in range(calls):
            for name, call in legs.items():
                t0 = time.perf_counter()
                info = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if hasattr(info, "kernel_ms"):
                    kernel[name].append(info.kernel_ms)
                last[name] = info
        q = lambda v: [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])] if v else None
        print(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT, after aic_reproject_split (yaw 0.02 rad): n_gaps {rinfo.n_gaps} of {count} pixels; central {central}, "
              f"cycle_length {cycle}; {calls} blocking calls per leg, alternating")
        for name in legs:
            r = {"wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name])}
            i = last[name]
            if name.startswith("aic_pick_pixels"):
                r.update({"n_unknown": i.n_unknown, "n_from_unknown": i.n_from_unknown, "n_from_order": i.n_from_order})
            print(f"{name:<58} " + json.dumps(r), flush=True)


def kernel_stats(directory):
    """The per-kernel table of one rocprofv3 --kernel-trace --stats run of --profile-leg, from the run's database (its `kernels` view)."""
    import re
    import sqlite3
    import statistics
    from collections import defaultdict

    files = sorted(glob.glob(os.path.join(directory, "**", "*results.db"), recursive=True))
    if not files:
        raise SystemExit(f"no rocprofv3 database under {directory}")
    rows = sqlite3.connect(files[0]).execute("select name, grid_x, start, end, duration, vgpr_count from kernels order by start").fetchall()
    print(f"# rocprofv3 --kernel-trace --stats, 10 calls each of aic_pick_pixels (n = {N}) with max_unknown = n and with max_unknown = 0, alternating; per kernel and grid size")
    groups = defaultdict(list)
    for name, grid, _, _, duration, vgprs in rows:
        m = re.search(r"pick_(count|scan|write)_kernel", name)
        if m:
            groups[(m.group(0), grid, vgprs)].append(duration)
    for (name, grid, vgprs), v in groups.items():
        print(f"{name:<20} threads {grid:>8} vgprs {vgprs:>3} launches {len(v):>3} median_ns {statistics.median(v):>8.0f} min {min(v):>7} max {max(v):>7}")
    first = [r for r in rows if "pick_count_kernel" in r[0]]
    last = [r for r in rows if "pick_write_kernel" in r[0] and r[1] > N]
    spans = [f[3] - s[2] for s, f in zip(first, last)]
    if spans:
        print(f"max_unknown = n: start of the count to end of the write, median of the calls {statistics.median(spans):.0f} ns")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--parent", help="built checkout of the parent commit: also run bench.py of both trees, alternating")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--profile-leg", action="store_true", help="10 calls of each aic_pick_pixels leg and nothing else: the program of a rocprofv3 run")
    ap.add_argument("--kernel-stats", help="print the per-kernel table of a rocprofv3 output directory")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
        return 0
    if a.profile_leg:
        measure(0, True)
        return 0
    print(f"# command: python tools/pick_timing.py --calls {a.calls}" + (f" --parent <parent checkout> --bench-steps {a.bench_steps}" if a.parent else ""))
    if a.parent:
        import reproject_timing as rt

        parent = os.path.abspath(a.parent)
        print("# bench.py --gpus 1 --no-cpu-baseline, alternating")
        for side, tree in (("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT)):
            print(f"bench {side:<6} " + json.dumps(rt.run_bench(tree, a.bench_steps)), flush=True)
    measure(a.calls, False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
