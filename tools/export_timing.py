#!/usr/bin/env python3
"""What aic_export_split costs, in ONE GPU command (profiles/export_split.txt).

usage: python tools/export_timing.py [--calls 40] [--out profiles/export_split.txt]

The atrium view of bench.py rendered once as AIC_FRAME_OUT_SPLIT frames resident in device memory, at 1920 x 1080 and at 960 x 540, with the mirror
camera's depth transform. Legs, each a blocking call into device memory:
  * the 540p frame exported at logged_image_size_policy of 1080p (740 x 416), both planes, and presented at that size with bloom 0;
  * the 1080p frame exported at 1080p, both planes, the depth plane alone, the statistics alone, and presented at 1080p with bloom 0.
The presentation at bloom 0 is the yardstick: the same stretch and encoder, one 4-byte plane less read and one less written. The legs alternate call by
call after 5 calls of warm-up each. Wall time per call and the HIP-event time; 10th percentile, median, 90th."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def measure(calls, say):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    import oracle
    from all_is_cubes_amd import _host as H
    from all_is_cubes_amd import abi

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    hw, hh = w // 2, h // 2
    lw, lh = abi.export_size((w, h))
    o = H.GraphicsOptions()
    o.view_distance = vd
    camera = H.Camera(o, H.Viewport.with_scale(1.0, w, h))
    ipzw = camera.inverse_projection_zw()
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(bloom_intensity=0.0, view_distance=vd))
        ctx.set_depth_transform(tuple(camera.depth_transform_zw()))
        split = abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK
        full = torch.zeros(w * h * 12, dtype=torch.uint8, device="cuda")
        half = torch.zeros(hw * hh * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(ctx.make_frame(w, h, world_inv=inv, flags=split), full.data_ptr())
        ctx.render_to_device(ctx.make_frame(hw, hh, world_inv=inv, flags=split), half.data_ptr())
        color = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        depth = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")

        def export(src, src_size, out_size, planes=(True, True)):
            outs = (color.data_ptr() if planes[0] else 0, depth.data_ptr() if planes[1] else 0)
            return lambda: ctx.export_split(src.data_ptr(), src_size, out_size, ipzw, device_outs=outs)[2]

        def present(src, src_size, out_size):
            return lambda: ctx.present_split(src.data_ptr(), src_size, out_size, 0.0, 0, float("inf"), out_device=color.data_ptr())[1]

        legs = {
            f"aic_export_split {hw}x{hh} -> {lw}x{lh}, colour and depth": export(half, (hw, hh), (lw, lh)),
            f"aic_present_split {hw}x{hh} -> {lw}x{lh}, bloom 0": present(half, (hw, hh), (lw, lh)),
            f"aic_export_split {w}x{h} -> {w}x{h}, colour and depth": export(full, (w, h), (w, h)),
            f"aic_export_split {w}x{h} -> {w}x{h}, depth alone": export(full, (w, h), (w, h), (False, True)),
            f"aic_export_split {w}x{h} -> {w}x{h}, statistics alone": export(full, (w, h), (w, h), (False, False)),
            f"aic_present_split {w}x{h} -> {w}x{h}, bloom 0": present(full, (w, h), (w, h)),
        }
        torch.cuda.synchronize()
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
        say(f"# {w} x {h} and {hw} x {hh} atrium, AIC_FRAME_OUT_SPLIT; logged size of {w} x {h}: {lw} x {lh}; {calls} blocking calls per leg, alternating")
        for name in legs:
            r = {"wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name])}
            i = last[name]
            if hasattr(i, "n_surface"):
                r["n_surface"], r["depth_min"], r["depth_max"] = int(i.n_surface), round(float(i.depth_min), 4), round(float(i.depth_max), 4)
            say(f"{name:<62} " + json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_split.txt"), help="the report is printed and written here")
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("# aic_export_split: one MI355X, one session (tools/export_timing.py; DESIGN.md 4.15)")
    say("#")
    say(f"# command: python tools/export_timing.py --calls {a.calls}")
    measure(a.calls, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
