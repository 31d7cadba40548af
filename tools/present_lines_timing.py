#!/usr/bin/env python3
"""What the line pass of aic_present_split_lines costs, in ONE GPU command (profiles/present_lines_timing.txt).

usage: python tools/present_lines_timing.py [--calls 40] [--parent DIR [--bench-steps 30]] [--out profiles/present_lines_timing.txt]

The 1920 x 1080 atrium frame of bench.py, rendered once as an AIC_FRAME_OUT_SPLIT frame resident in device memory, and the same view at 960 x 540.
Legs, each a blocking call into device memory, for bloom 0 and 0.125, at equal size and stretched from 960 x 540:
  * aic_present_split;
  * aic_present_split_lines with the 28 lines of a cursor's wireframe on the surface the ray through the middle of the view hits (aic_trace_rays' first-hit
    record; host vertices, as the host mirror passes them);
  * aic_present_split_lines with 4096 random lines inside the view (device vertices);
  * the last two again on a second context made with AIC_LINES_CLEAR_KEYS=1, which clears the whole key image at the start of every call instead of
    putting back the keys the call touched.
The legs alternate call by call after 5 calls of warm-up each. Wall time per call and the HIP-event time; 10th percentile, median, 90th.

With --parent (a built checkout of the parent commit): `bench.py --gpus 1 --no-cpu-baseline` of the parent, this tree, the parent, this tree."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from present_timing import run_bench  # noqa: E402

BLOOM = 0.125
N_RANDOM = 4096


def measure(calls, say):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    import oracle
    from all_is_cubes_amd import _host as H
    from all_is_cubes_amd import abi

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    proj, w2e, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    m = (w2e @ proj).reshape(16).astype(np.float32)  # euclid's row-vector order is the ABI's column-major one
    hw, hh = w // 2, h // 2
    rng = np.random.default_rng(1)
    ndc = np.concatenate([rng.uniform(-1, 1, (2 * N_RANDOM, 2)), rng.uniform(0.0, 1.0, (2 * N_RANDOM, 1)), np.ones((2 * N_RANDOM, 1))], axis=1)
    world = ndc @ inv
    random_lines = np.zeros((2 * N_RANDOM, 7), np.float32)
    random_lines[:, :3] = world[:, :3] / world[:, 3:]
    random_lines[:, 3:6] = rng.uniform(0, 2, (2 * N_RANDOM, 3))
    random_lines[:, 6] = 1.0
    ctx = abi.Context(0)
    os.environ["AIC_LINES_CLEAR_KEYS"] = "1"
    ctx_clear = abi.Context(0)
    del os.environ["AIC_LINES_CLEAR_KEYS"]
    try:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        opt = abi.make_options(bloom_intensity=BLOOM, view_distance=vd)
        ctx.set_options(abi.LAYER_WORLD, opt)
        tm, mi = opt.tone_mapping, opt.maximum_intensity
        # the frames' depth planes are the projected depth of this camera (raytrace_to_texture.rs:613-618), as draw_split makes them
        o = H.GraphicsOptions()
        o.view_distance = vd
        ctx.set_depth_transform(tuple(H.Camera(o, H.Viewport.with_scale(1.0, w, h)).depth_transform_zw()))
        # the cursor: where the ray through the middle of the view first hits, as an application's cursor ray would find it
        direction = np.subtract(target, eye) / np.linalg.norm(np.subtract(target, eye))
        hit = ctx.trace_rays(abi.LAYER_WORLD, [[*eye, *direction]], want_aux=True)["aux"][0]
        if not hit["hit"]:
            raise SystemExit("the ray through the middle of the view hits nothing: no cursor to draw")
        distance = float(hit["t_distance"])
        cursor = abi.cursor_wireframe(hit["cube"], int(hit["face"]), int(hit["face"]), np.add(eye, direction * distance), distance)
        say(f"# cursor: cube {hit['cube'].tolist()}, face {int(hit['face'])}, distance {distance:.3f}: {len(cursor) // 2} lines")
        split = abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK
        full = torch.zeros(w * h * 12, dtype=torch.uint8, device="cuda")
        half = torch.zeros(hw * hh * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(ctx.make_frame(w, h, world_inv=inv, flags=split), full.data_ptr())
        ctx.render_to_device(ctx.make_frame(hw, hh, world_inv=inv, flags=split), half.data_ptr())
        out8 = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        on_device = torch.from_numpy(random_lines.view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()

        def plain(src, size, bloom):
            return lambda: (ctx.present_split(src.data_ptr(), size, (w, h), bloom, tm, mi, out_device=out8.data_ptr())[1], None)

        def lines(c, src, size, bloom, vertices, n=None):
            return lambda: c.present_split_lines(src.data_ptr(), size, (w, h), bloom, tm, mi, m, vertices, n, out_device=out8.data_ptr())[1:]

        legs = {}
        for src, size in ((full, (w, h)), (half, (hw, hh))):
            for bloom in (0.0, BLOOM):
                where = f"{size[0]}x{size[1]} -> {w}x{h}, bloom {bloom}"
                legs[f"aic_present_split {where}"] = plain(src, size, bloom)
                legs[f"..._lines, 28 cursor lines {where}"] = lines(ctx, src, size, bloom, cursor)
                legs[f"..._lines, {N_RANDOM} random lines {where}"] = lines(ctx, src, size, bloom, on_device.data_ptr(), N_RANDOM)
                legs[f"..._lines, 28 cursor lines, keys cleared per call {where}"] = lines(ctx_clear, src, size, bloom, cursor)
                legs[f"..._lines, {N_RANDOM} random lines, keys cleared per call {where}"] = lines(ctx_clear, src, size, bloom, on_device.data_ptr(), N_RANDOM)
        for call in legs.values():
            for _ in range(5):
                call()
        wall = {name: [] for name in legs}
        kernel = {name: [] for name in legs}
        counts = {}
        for _ in range(calls):
            for name, call in legs.items():
                t0 = time.perf_counter()
                info, lines_info = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                kernel[name].append(info.kernel_ms)
                if lines_info is not None:
                    counts[name] = {k: getattr(lines_info, k) for k in ("n_clipped_away", "n_fragments", "n_passed", "n_pixels")}
        q = lambda v: [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])]
        say(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT; line scratch {abi.present_lines_scratch((w, h), (w, h), 28)} bytes with 28 host lines; {calls} blocking calls "
            "per leg, alternating")
        for name in legs:
            r = {"wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name]), **counts.get(name, {})}
            say(f"{name:<86} " + json.dumps(r))
    finally:
        ctx.close()
        ctx_clear.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--parent", help="built checkout of the parent commit: also run bench.py of both trees, alternating")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_lines_timing.txt"), help="the report is printed and written here")
    a = ap.parse_args()
    report = []

    def say(line):
        print(line, flush=True)
        report.append(line)

    say("# aic_present_split_lines: one MI355X, one session (tools/present_lines_timing.py; DESIGN.md 4.13)")
    say("#")
    say(f"# command: python tools/present_lines_timing.py --calls {a.calls}" + (f" --parent <parent checkout> --bench-steps {a.bench_steps}" if a.parent else ""))
    if a.parent:
        parent = os.path.abspath(a.parent)
        say("# bench.py --gpus 1 --no-cpu-baseline, alternating")
        for side, tree in (("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT)):
            say(f"bench {side:<6} " + json.dumps(run_bench(tree, a.bench_steps)))
    measure(a.calls, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(report) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
