#!/usr/bin/env python3
"""What aic_present_split costs, in ONE GPU command (profiles/present_timing.txt).

usage: python tools/present_timing.py [--calls 40] [--parent DIR [--bench-steps 30]] [--out profiles/present_timing.txt]

The 1920 x 1080 atrium frame of bench.py, rendered once as an AIC_FRAME_OUT_SPLIT frame resident in device memory, and the same view rendered at
960 x 540 (the reference traces at half the nominal size and stretches, raytracer_size_policy). Legs, each a blocking call into device memory:
  * the 1080p frame presented at 1080p with bloom 0.125 and with bloom 0, as RGBA8 (and with bloom 0.125 as f16);
  * the 540p frame presented at 1080p with bloom 0.125 and with bloom 0;
  * beside them one aic_render of the 1080p frame with and without AIC_FRAME_BLOOM at bloom 0.125 (AIC_FRAME_NO_FEEDBACK, RGBA8): their difference is
    what the ColorBuf bloom path adds to a single frame (DESIGN.md 4.7 recorded +0.216 ms).
The legs alternate call by call after 5 calls of warm-up each. Wall time per call and the HIP-event time; 10th percentile, median, 90th.

With --parent (a built checkout of the parent commit): `bench.py --gpus 1 --no-cpu-baseline` of the parent, this tree, the parent, this tree."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BLOOM = 0.125


def measure(calls, say):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    import oracle
    from all_is_cubes_amd import abi

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    hw, hh = w // 2, h // 2
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        opt = abi.make_options(bloom_intensity=BLOOM, view_distance=vd)
        ctx.set_options(abi.LAYER_WORLD, opt)
        tm, mi = opt.tone_mapping, opt.maximum_intensity
        split = abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK
        full = torch.zeros(w * h * 12, dtype=torch.uint8, device="cuda")
        half = torch.zeros(hw * hh * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(ctx.make_frame(w, h, world_inv=inv, flags=split), full.data_ptr())
        ctx.render_to_device(ctx.make_frame(hw, hh, world_inv=inv, flags=split), half.data_ptr())
        out8 = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        out16 = torch.zeros(w * h * 8, dtype=torch.uint8, device="cuda")
        traced = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")

        def present(src, size, bloom, flags=0, out=out8):
            return lambda: ctx.present_split(src.data_ptr(), size, (w, h), bloom, tm, mi, flags=flags, out_device=out.data_ptr())[1]

        def render(flags):
            frame = ctx.make_frame(w, h, world_inv=inv, flags=flags | abi.FRAME_NO_FEEDBACK)
            return lambda: ctx.render_to_device(frame, traced.data_ptr())

        legs = {
            f"aic_present_split {w}x{h} -> {w}x{h}, bloom {BLOOM}": present(full, (w, h), BLOOM),
            f"aic_present_split {w}x{h} -> {w}x{h}, bloom 0": present(full, (w, h), 0.0),
            f"aic_present_split {w}x{h} -> {w}x{h}, bloom {BLOOM}, OUT_F16": present(full, (w, h), BLOOM, abi.PRESENT_OUT_F16, out16),
            f"aic_present_split {hw}x{hh} -> {w}x{h}, bloom {BLOOM}": present(half, (hw, hh), BLOOM),
            f"aic_present_split {hw}x{hh} -> {w}x{h}, bloom 0": present(half, (hw, hh), 0.0),
            f"aic_render {w}x{h}, AIC_FRAME_BLOOM at {BLOOM}": render(abi.FRAME_BLOOM),
            f"aic_render {w}x{h}, no bloom": render(0),
        }
        torch.cuda.synchronize()
        for call in legs.values():
            for _ in range(5):
                call()
        wall = {name: [] for name in legs}
        kernel = {name: [] for name in legs}
        for _ in range(calls):
            for name, call in legs.items():
                t0 = time.perf_counter()
                info = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                kernel[name].append(info.kernel_ms)
        q = lambda v: [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])]
        levels, t0, scratch = abi.present_geometry((w, h), (w, h))
        _, _, scratch_half = abi.present_geometry((hw, hh), (w, h))
        say(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT; L = {levels}, T0 = {t0[0]} x {t0[1]}, scratch {scratch} bytes at equal size, {scratch_half} stretched from "
            f"{hw} x {hh}; {calls} blocking calls per leg, alternating")
        med = {}
        for name in legs:
            r = {"wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name])}
            med[name] = (r["wall_ms_p10_p50_p90"][1], r["kernel_ms_p10_p50_p90"][1])
            say(f"{name:<62} " + json.dumps(r))
        names = list(legs)
        say(f"# AIC_FRAME_BLOOM adds to a single frame (medians): wall {med[names[5]][0] - med[names[6]][0]:+.4f} ms, HIP events {med[names[5]][1] - med[names[6]][1]:+.4f} ms")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_timing.txt"), help="the report is printed and written here")
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("# aic_present_split: one MI355X, one session (tools/present_timing.py; DESIGN.md 4.11)")
    say("#")
    say(f"# command: python tools/present_timing.py --calls {a.calls}" + (f" --parent <parent checkout> --bench-steps {a.bench_steps}" if a.parent else ""))
    if a.parent:
        parent = os.path.abspath(a.parent)
        say("# bench.py --gpus 1 --no-cpu-baseline, alternating")
        for side, tree in (("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT)):
            say(f"bench {side:<6} " + json.dumps(run_bench(tree, a.bench_steps)))
    measure(a.calls, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
