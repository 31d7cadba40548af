#!/usr/bin/env python3
"""What a scattered pixel list costs through aic_trace_pixels, in ONE GPU command (profiles/trace_pixels_timing.txt).

usage: python tools/trace_pixels_timing.py [--calls 40] [--parent DIR [--bench-steps 30]]

The 1920 x 1080 atrium frame of bench.py as an AIC_FRAME_OUT_SPLIT frame resident in device memory, four ways, the legs alternating call by call
after 5 calls of warm-up each:
 (1) aic_trace_pixels, in place, ONE call listing a whole cycle of the pixel picker in pick order (aic_pixel_order: 2 * (count - 60000) picks at 1080p,
     the central 60 000 pixels about 33 times each);
 (2) the same with the picker's sorted order alone, every pixel once (the scattered order without the repeats of the central pixels);
 (3) aic_trace_pixels, in place, one call listing every pixel once in row-major order;
 (4) aic_render of the same frame (AIC_FRAME_NO_FEEDBACK: a pixel list has no cost feedback either).
All four run the recording variants. Wall time per call (the calls return when the device is done) and the launches' HIP-event time; 10th percentile,
median, 90th; nanoseconds per listed pixel from the median. The targets of (1) to (3) are checked against (4)'s bytes once.

With --parent (a built checkout of the parent commit): `bench.py --gpus 1 --no-cpu-baseline` of the parent, this tree, the parent, this tree. bench.py
runs production variants only; the parent's two runs give the spread a difference has to exceed to mean anything."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def measure(calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    import oracle
    from all_is_cubes_amd import abi

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    count = w * h
    order, central, cycle = abi.pixel_order(w, h)
    k = np.arange(cycle, dtype=np.int64)
    picks = order[np.where(k % 2 == 0, (k // 2) % central, central + (k // 2) % (count - central))]
    lists = {"picker order, a whole cycle": picks, "the picker's sorted order, every pixel once": order, "row-major, every pixel once": np.arange(count, dtype=np.uint32)}
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(bloom_intensity=0.0, view_distance=vd))
        frame = ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK)
        whole = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        legs, n_listed, targets = {}, {}, {}
        for name, px in lists.items():
            dev = torch.from_numpy(np.ascontiguousarray(px, np.uint32).view(np.int32)).cuda()
            tgt = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
            legs["aic_trace_pixels in place, " + name] = (lambda dev=dev, tgt=tgt, n=len(px): ctx.trace_pixels_device(frame, n, dev.data_ptr(), tgt.data_ptr(), in_place=True))
            n_listed["aic_trace_pixels in place, " + name] = len(px)
            targets[name] = tgt
        legs["aic_render, the same Split frame"] = lambda: ctx.render_to_device(frame, whole.data_ptr())
        n_listed["aic_render, the same Split frame"] = count
        torch.cuda.synchronize()
        for call in legs.values():
            for _ in range(5):
                call()
        for name, tgt in targets.items():
            if not bool((tgt == whole).all()):
                raise SystemExit(f"{name}: the target differs from aic_render's frame")
        wall = {name: [] for name in legs}
        kernel = {name: [] for name in legs}
        for _ in range(calls):
            for name, call in legs.items():
                t0 = time.perf_counter()
                info = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                kernel[name].append(info.kernel_ms)
        q = lambda v: [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])]
        print(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT; {count} pixels, central {central}, cycle_length {cycle}; {calls} calls per leg, alternating")
        for name in legs:
            r = {"pixels_listed": n_listed[name], "wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name]),
                 "ns_per_listed_pixel": round(float(np.median(wall[name])) * 1e6 / n_listed[name], 3)}
            print(f"{name:<74} " + json.dumps(r), flush=True)


def run_bench(tree, steps):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "3", "--no-cpu-baseline"], cwd=tree, capture_output=True,
                       text=True, timeout=900, env=dict(os.environ, PYTHONPATH=tree))
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-2000:])
        raise SystemExit(f"bench.py in {tree} ended with {p.returncode}")  # (nothing more is started on the device)
    r = json.loads([l for l in p.stdout.split("\n") if l.startswith("{")][-1])
    s = r.get("single_frame", {})
    return {"ms_per_step": r.get("ms_per_step"), "single_frame_warm_ms": s.get("single_frame_warm_ms"), "single_frame_cold_ms": s.get("single_frame_cold_ms"),
            "kernel_ms_warm": s.get("kernel_ms_warm"), "kernel_ms_cold": s.get("kernel_ms_cold"), "streamed_moving_camera_ms": s.get("streamed_moving_camera_ms")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--parent", help="built checkout of the parent commit: also run bench.py of both trees, alternating")
    ap.add_argument("--bench-steps", type=int, default=30)
    a = ap.parse_args()
    print(f"# command: python tools/trace_pixels_timing.py --calls {a.calls}" + (f" --parent <parent checkout> --bench-steps {a.bench_steps}" if a.parent else ""))
    if a.parent:
        parent = os.path.abspath(a.parent)
        print("# bench.py --gpus 1 --no-cpu-baseline, alternating")
        for side, tree in (("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT)):
            print(f"bench {side:<6} " + json.dumps(run_bench(tree, a.bench_steps)), flush=True)
    measure(a.calls)
    return 0


if __name__ == "__main__":
    sys.exit(main())
