#!/usr/bin/env python3
"""What aic_reproject_split costs beside the re-trace it stands in for, in ONE GPU command (profiles/reproject_timing.txt).

usage: python tools/reproject_timing.py [--calls 40] [--parent DIR [--bench-steps 30]]
       rocprofv3 --kernel-trace --stats -d DIR -o reproject -- python tools/reproject_timing.py --profile-leg     (a run of its own: the time per kernel)
       python tools/reproject_timing.py --kernel-stats DIR                                                        (prints that run's table)

The 1920 x 1080 atrium frame of bench.py, rendered once as an AIC_FRAME_OUT_SPLIT frame resident in device memory with the depth transform of
raytrace_to_texture, then reprojected into two nearby cameras -- a yaw of 0.02 rad about the eye and a step of one cube forward -- each without and
with AIC_REPROJECT_KEEP_SPLATS; beside them aic_render of the Split frame at each new camera (AIC_FRAME_NO_FEEDBACK), the re-trace a reprojection
stands in for. The legs alternate call by call after 5 calls of warm-up each; every call is blocking. Wall time per call and the HIP-event time;
10th percentile, median, 90th; the four counts; and the share of pixels whose colour is the re-traced frame's.

With --parent (a built checkout of the parent commit): `bench.py --gpus 1 --no-cpu-baseline` of the parent, this tree, the parent, this tree."""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEAR = 1.0 / 32.0


def cameras():
    import numpy as np

    import bench
    import oracle

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    eye, target = np.array(eye, float), np.array(target, float)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    c, s = np.cos(0.02), np.sin(0.02)
    d = target - eye
    yawed = eye + np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]])
    views = {"traced": (eye, target), "yaw 0.02 rad": (eye, yawed), "forward 1 cube": (eye + fwd, target + fwd)}
    out = {}
    for name, (e, t) in views.items():
        p, v, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(tuple(e), tuple(t)), tuple(e))
        out[name] = (p, v, inv)
    return sp, w, h, vd, out


def reprojection(old, new):
    """(matrix [16] f32 as WGSL holds it, inverse_projection_zw [4] f32) from two (projection, view, inverse) triples in euclid's row-vector order"""
    import numpy as np

    m = np.linalg.inv(old[1] @ old[0]) @ new[1] @ new[0]
    ip = np.linalg.inv(new[0])
    return m.reshape(16).astype(np.float32), np.array([ip[2, 2], ip[3, 2], ip[2, 3], ip[3, 3]], np.float32)


def depth_transform(p, vd):
    ds, db = -(vd - NEAR), -NEAR
    return (ds * p[2, 2], db * p[2, 2] + p[3, 2], ds * p[2, 3], db * p[2, 3] + p[3, 3])


def measure(calls, profile_leg):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from all_is_cubes_amd import abi

    sp, w, h, vd, cams = cameras()
    count = w * h
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(bloom_intensity=0.0, view_distance=vd))
        ctx.set_depth_transform(depth_transform(cams["traced"][0], vd))
        flags = abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK
        src = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(ctx.make_frame(w, h, world_inv=cams["traced"][2], flags=flags), src.data_ptr())
        legs, retraced, targets = {}, {}, {}
        for name in ("yaw 0.02 rad", "forward 1 cube"):
            m, zw = reprojection(cams["traced"], cams[name])
            frame = ctx.make_frame(w, h, world_inv=cams[name][2], flags=flags)
            whole = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
            retraced[name] = whole
            for keep in (0, abi.REPROJECT_KEEP_SPLATS):
                dst = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
                leg = f"aic_reproject_split, {name}" + (", KEEP_SPLATS" if keep else "")
                legs[leg] = (lambda m=m, zw=zw, dst=dst, keep=keep: ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr(), keep))
                targets[leg] = (dst, name)
            legs[f"aic_render, the Split frame at {name}"] = (lambda frame=frame, whole=whole: ctx.render_to_device(frame, whole.data_ptr()))
        torch.cuda.synchronize()
        if profile_leg:
            for _ in range(10):
                legs["aic_reproject_split, yaw 0.02 rad"]()
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
                kernel[name].append(info.kernel_ms)
                last[name] = info
        q = lambda v: [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])]
        levels, t0, scratch = abi.reproject_geometry(w, h)
        print(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT; {count} pixels; L = {levels}, T0 = {t0[0]} x {t0[1]}, scratch {scratch} bytes; {calls} blocking calls per leg, alternating")
        for name in legs:
            r = {"wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name])}
            if name in targets:
                i = last[name]
                dst, cam = targets[name]
                same = (dst[:count * 8].view(count, 8) == retraced[cam][:count * 8].view(count, 8)).all(1).float().mean().item()
                r.update({"n_splats": i.n_splats, "n_dropped": i.n_dropped, "n_gaps": i.n_gaps, "n_unfilled": i.n_unfilled,
                          "share_of_pixels_with_the_retraced_colour": round(same, 4)})
            print(f"{name:<58} " + json.dumps(r), flush=True)


def kernel_stats(directory):
    """The per-kernel table of one rocprofv3 --kernel-trace --stats run of --profile-leg (10 calls), from the run's database (its `kernels` view)."""
    import re
    import sqlite3
    import statistics
    from collections import defaultdict

    files = sorted(glob.glob(os.path.join(directory, "**", "*results.db"), recursive=True))
    if not files:
        raise SystemExit(f"no rocprofv3 database under {directory}")
    rows = sqlite3.connect(files[0]).execute("select name, grid_x, start, end, duration, vgpr_count from kernels order by start").fetchall()
    print("# rocprofv3 --kernel-trace --stats, 10 calls of aic_reproject_split (yaw 0.02 rad, no flag) after the source frame's render; per kernel and grid size")
    groups = defaultdict(list)
    for name, grid, _, _, duration, vgprs in rows:
        m = re.search(r"reproject_\w+", name)
        if m:
            groups[(m.group(0), grid, vgprs)].append(duration)
    total = 0.0
    for (name, grid, vgprs), v in groups.items():
        print(f"{name:<28} threads {grid:>8} vgprs {vgprs:>3} launches {len(v):>3} median_ns {statistics.median(v):>8.0f} min {min(v):>7} max {max(v):>7}")
        total += statistics.median(v) * len(v) / 10
    first = [r for r in rows if "reproject_splat" in r[0]]
    last = [r for r in rows if "reproject_final" in r[0]]
    spans = [f[3] - s[2] for s, f in zip(first, last)]
    print(f"sum of the medians per call {total:.0f} ns; start of the splat to end of the final store, median of the calls {statistics.median(spans):.0f} ns")


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
    ap.add_argument("--profile-leg", action="store_true", help="10 calls of one reprojection and nothing else: the program of a rocprofv3 run")
    ap.add_argument("--kernel-stats", help="print the per-kernel table of a rocprofv3 output directory")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
        return 0
    if a.profile_leg:
        measure(0, True)
        return 0
    print(f"# command: python tools/reproject_timing.py --calls {a.calls}" + (f" --parent <parent checkout> --bench-steps {a.bench_steps}" if a.parent else ""))
    if a.parent:
        parent = os.path.abspath(a.parent)
        print("# bench.py --gpus 1 --no-cpu-baseline, alternating")
        for side, tree in (("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT)):
            print(f"bench {side:<6} " + json.dumps(run_bench(tree, a.bench_steps)), flush=True)
    measure(a.calls, False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
