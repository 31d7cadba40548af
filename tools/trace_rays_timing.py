#!/usr/bin/env python3
"""Timing of aic_trace_rays against the parent commit, in ONE GPU command with the two sides alternating (profiles/trace_rays_timing.txt).

usage: python tools/trace_rays_timing.py --parent DIR [--calls 300] [--bench-steps 30] [--skip-bench]

DIR is a built checkout of the parent commit (its own libaic_hip.so and host module). Every measurement runs in a fresh child process whose
`all_is_cubes_amd` is that of the tree it measures:
 (a) `bench.py --gpus 1 --no-cpu-baseline` of the parent, this tree, the parent, this tree: ms_per_step and the single_frame figures. The parent's
     two runs give the spread a difference has to exceed to mean anything.
 (b) the 1080p atrium frame. Parent and this tree: aic_render with AIC_FRAME_NO_FEEDBACK into device memory (a cold frame). This tree: the same
     frame's camera rays, made on the host, through aic_trace_rays(AIC_RAYS_DEVICE | AIC_FRAME_OUT_COLORBUF) and in RGBA8. `--calls` timed calls each
     after 20 of warm-up, wall time per call (submit to completion) and the kernel's own HIP-event time; medians and the 10th / 90th percentiles.
     The parent's legs run before and after this tree's.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def child_frame(tree, calls, rays):
    sys.path.insert(0, tree)
    os.chdir(tree)
    import numpy as np
    import torch

    import bench
    import oracle
    from all_is_cubes_amd import abi

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    n = w * h
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(bloom_intensity=0.0, view_distance=vd))
        legs = {}
        if not rays:
            out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            frame = ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_NO_FEEDBACK)
            legs["aic_render cold, RGBA8"] = lambda: ctx.render_to_device(frame, out.data_ptr())
            out_f = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            frame_f = ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_NO_FEEDBACK | abi.FRAME_OUT_COLORBUF)
            legs["aic_render cold, ColorBuf"] = lambda: ctx.render_to_device(frame_f, out_f.data_ptr())
        else:
            m = np.asarray(inv, np.float64).reshape(16)
            ex = np.arange(w + 1, dtype=np.float64) / np.float64(w) * 2.0 - 1.0
            ey = -(np.arange(h + 1, dtype=np.float64) / np.float64(h) * 2.0 - 1.0)
            X, Y = np.meshgrid((ex[:-1] + ex[1:]) / 2.0, (ey[:-1] + ey[1:]) / 2.0)

            def unproject(z):
                o = [X * m[k] + Y * m[4 + k] + z * m[8 + k] + m[12 + k] for k in range(4)]
                return [o[k] / o[3] for k in range(3)]

            near, far = unproject(0.0), unproject(1.0)
            host_rays = np.ascontiguousarray(np.stack(near + [f - a for f, a in zip(far, near)], -1).reshape(-1, 6))
            dev_rays = torch.from_numpy(host_rays).cuda()
            out = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
            out_f = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            legs["aic_trace_rays device, RGBA8"] = lambda: ctx.trace_rays_device(abi.LAYER_WORLD, n, dev_rays.data_ptr(), out.data_ptr())
            legs["aic_trace_rays device, ColorBuf"] = lambda: ctx.trace_rays_device(abi.LAYER_WORLD, n, dev_rays.data_ptr(), out_f.data_ptr(), flags=abi.FRAME_OUT_COLORBUF)
        torch.cuda.synchronize()
        result = {}
        for name, call in legs.items():
            for _ in range(20):
                call()
            wall, kernel = [], []
            for _ in range(calls):
                t0 = time.perf_counter()
                info = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                kernel.append(info.kernel_ms)
            q = lambda v: [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])]
            result[name] = {"wall_ms_p10_p50_p90": q(wall), "kernel_ms_p10_p50_p90": q(kernel), "variant": int(info.variant), "steps": int(info.cubes_traced)}
    print("RESULT " + json.dumps(result))


def run_child(tree, args):
    env = dict(os.environ)
    env["PYTHONPATH"] = tree
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=tree, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-2000:])
        raise SystemExit(f"child {args} in {tree} ended with {p.returncode}")  # (nothing more is started on the device)
    return json.loads([l for l in p.stdout.split("\n") if l.startswith("RESULT ")][-1][7:])


def run_bench(tree, steps):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "3", "--no-cpu-baseline"], cwd=tree, capture_output=True,
                       text=True, timeout=900, env=dict(os.environ, PYTHONPATH=tree))
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-2000:])
        raise SystemExit(f"bench.py in {tree} ended with {p.returncode}")
    line = [l for l in p.stdout.split("\n") if l.startswith("{")][-1]
    r = json.loads(line)
    s = r.get("single_frame", {})
    return {"ms_per_step": r.get("ms_per_step"), "single_frame_warm_ms": s.get("single_frame_warm_ms"), "single_frame_cold_ms": s.get("single_frame_cold_ms"),
            "kernel_ms_warm": s.get("kernel_ms_warm"), "kernel_ms_cold": s.get("kernel_ms_cold"), "streamed_moving_camera_ms": s.get("streamed_moving_camera_ms")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the parent commit")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--child", choices=["frame", "rays"])
    ap.add_argument("--tree")
    a = ap.parse_args()
    if a.child:
        child_frame(a.tree, a.calls, a.child == "rays")
        return 0
    parent = os.path.abspath(a.parent)
    print(f"# command: python tools/trace_rays_timing.py --parent <parent checkout> --calls {a.calls} --bench-steps {a.bench_steps}")
    if not a.skip_bench:
        print("# (a) bench.py --gpus 1 --no-cpu-baseline, alternating")
        for side, tree in (("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT)):
            print(f"bench {side:<6} " + json.dumps(run_bench(tree, a.bench_steps)), flush=True)
    print("# (b) the 1080p atrium frame, cold, into device memory; wall = submit to completion per call")
    child = ["--calls", str(a.calls)]
    for side, tree, kind in (("parent", parent, "frame"), ("this", ROOT, "rays"), ("this", ROOT, "frame"), ("parent", parent, "frame"), ("this", ROOT, "rays")):
        for name, r in run_child(tree, ["--child", kind, "--tree", tree] + child).items():
            print(f"{side:<6} {name:<34} " + json.dumps(r), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
