#!/usr/bin/env python3
"""What the info text adds to a presentation, in ONE GPU command (profiles/present_text.txt).

usage: python tools/present_text_timing.py [--calls 40] [--parent DIR [--bench-steps 30]] [--out FILE]

The 1920 x 1080 atrium frame of bench.py, rendered once as an AIC_FRAME_OUT_SPLIT frame resident in device memory and presented at its own size as
RGBA8 into device memory. Legs, each a blocking call, with bloom 0 and with bloom 0.125:
  * with --parent, the parent's aic_present_split: its library, loaded beside this tree's, on a context of its own and the same resident frame;
  * aic_present_split_text with no text (which is aic_present_split_lines, and without lines aic_present_split);
  * the same with a three-line text in the top left corner, as the reference's info text is;
  * the same with a grid of 'M' that fills the window.
The font is the host mirror's info_text_font_atlas, the grid aic_text_geometry's for a nominal size of 1920 x 1080. The legs alternate call by call
after 5 calls of warm-up each. Wall time per call and the HIP-event time; 10th percentile, median, 90th.

With --parent also: `bench.py --gpus 1 --no-cpu-baseline` of the parent, this tree, the parent, this tree."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BLOOM = 0.125
THREE_LINES = "FPS 59.9 (16.69 ms)\nrays 2073600, 41.2 cubes/ray\nlight queue 0"


def measure(calls, parent, say):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    import oracle
    from all_is_cubes_amd import _host as H
    from all_is_cubes_amd import abi

    parent_abi = None
    if parent:
        spec = importlib.util.spec_from_file_location("parent_abi", os.path.join(parent, "all_is_cubes_amd", "abi.py"))
        parent_abi = importlib.util.module_from_spec(spec)
        sys.modules["parent_abi"] = parent_abi
        spec.loader.exec_module(parent_abi)

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        opt = abi.make_options(bloom_intensity=BLOOM, view_distance=vd)
        ctx.set_options(abi.LAYER_WORLD, opt)
        tm, mi = opt.tone_mapping, opt.maximum_intensity
        full = torch.zeros(w * h * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK), full.data_ptr())
        out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        cell = H.INFO_TEXT_CELL
        ctx.set_text_font(H.info_text_font_atlas(), *cell)
        cols, rows, scale, origin = abi.text_geometry((w, h), cell)
        corner, used = abi.text_layout(THREE_LINES, cols, rows)
        filled, _ = abi.text_layout("\n".join("M" * cols for _ in range(rows)), cols, rows)
        parent_ctx = parent_abi.Context(0) if parent_abi else None

        def with_text(bloom, codes):
            text = None if codes is None else (codes, scale, origin)
            return lambda: ctx.present_split_text(full.data_ptr(), (w, h), (w, h), bloom, tm, mi, text=text, out_device=out.data_ptr())[1]

        legs = {}
        for bloom in (0.0, BLOOM):
            if parent_ctx:
                legs[f"parent's aic_present_split, bloom {bloom}"] = (
                    lambda bloom=bloom: parent_ctx.present_split(full.data_ptr(), (w, h), (w, h), bloom, tm, mi, out_device=out.data_ptr())[1])
            legs[f"aic_present_split_text, no text, bloom {bloom}"] = with_text(bloom, None)
            legs[f"aic_present_split_text, three lines, bloom {bloom}"] = with_text(bloom, corner)
            legs[f"aic_present_split_text, {cols} x {rows} of 'M', bloom {bloom}"] = with_text(bloom, filled)
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
        say(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT, presented at {w} x {h} as RGBA8; font cell {cell}, grid {cols} x {rows}, the three lines use {used[0]} x {used[1]} "
            f"cells; {calls} blocking calls per leg, alternating")
        for name in legs:
            say(f"{name:<58} " + json.dumps({"wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name])}))
        if parent_ctx:
            parent_ctx.close()


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
    ap.add_argument("--parent", help="built checkout of the parent commit: its aic_present_split as a leg, and bench.py of both trees, alternating")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_text_timing.txt"), help="the report is printed and written here")
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("# aic_present_split_text: one MI355X, one session (tools/present_text_timing.py; DESIGN.md 4.14)")
    say("#")
    say(f"# command: python tools/present_text_timing.py --calls {a.calls}" + (f" --parent <parent checkout> --bench-steps {a.bench_steps}" if a.parent else ""))
    parent = os.path.abspath(a.parent) if a.parent else None
    if parent:
        say("# bench.py --gpus 1 --no-cpu-baseline, alternating")
        for side, tree in (("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT)):
            say(f"bench {side:<6} " + json.dumps(run_bench(tree, a.bench_steps)))
    measure(a.calls, parent, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
