#!/usr/bin/env python3
"""What an AIC_FRAME_OUT_SPLIT frame costs: aic_frame_info.kernel_ms (HIP events around the trace) of single 1920 x 1080 frames of the atrium-like
scene, rendered into device memory, for
  * split:      AIC_FRAME_OUT_SPLIT                           (the recording variant, 12 bytes per pixel out)
  * recording:  AIC_FRAME_COUNTERS | AIC_FRAME_OUT_COLORBUF   (the same variant, 16 bytes per pixel out)
  * plain:      no flag                                       (the production variant, RGBA8)
With --baseline DIR the recording and plain frames are ALSO measured on another build of the library, loaded into the same process: DIR is a built copy
of that commit's all_is_cubes_amd package (abi.py, flat.py, __init__.py, libaic_hip.so). The modes are interleaved: every round measures each of them
once, --frames frames each after a warm-up, and keeps the round's median; the report is the median over the rounds and their spread (min .. max).
Usage: python tools/split_timing.py [--baseline DIR] [--rounds R] [--frames N]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import oracle  # noqa: E402
from all_is_cubes_amd import abi  # noqa: E402


def load_baseline(pkg_dir):
    spec = importlib.util.spec_from_file_location("aic_baseline", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["aic_baseline"] = pkg
    spec.loader.exec_module(pkg)
    return importlib.import_module("aic_baseline.abi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=15)
    args = ap.parse_args()
    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    buf = torch.zeros(w * h * 16, dtype=torch.uint8, device="cuda")  # (room for the largest output, 16 bytes per pixel)
    torch.cuda.synchronize()
    builds = [("this", abi)]
    if args.baseline:
        builds.append(("baseline", load_baseline(args.baseline)))
    modes = []  # (label, context, frame)
    contexts = []
    for label, mod in builds:
        ctx = mod.Context(0)
        contexts.append(ctx)
        ctx.upload_space(mod.LAYER_WORLD, sp)
        ctx.set_options(mod.LAYER_WORLD, mod.make_options(fog=3, view_distance=vd))
        flag_sets = {"recording": mod.FRAME_COUNTERS | mod.FRAME_OUT_COLORBUF, "plain": 0}
        if hasattr(mod, "FRAME_OUT_SPLIT"):
            flag_sets["split"] = mod.FRAME_OUT_SPLIT
            ctx.set_depth_transform((1.0, 0.0, 0.0, 1.0))
        for name, flags in flag_sets.items():
            modes.append((f"{label}:{name}", ctx, ctx.make_frame(w, h, world_inv=inv, flags=flags)))
    medians = {label: [] for label, _, _ in modes}
    for _ in range(args.rounds):
        for label, ctx, frame in modes:
            for _ in range(3):  # warm: the mode's allocations, the tile feedback of this view
                ctx.render_to_device(frame, buf.data_ptr())
            ms = [ctx.render_to_device(frame, buf.data_ptr()).kernel_ms for _ in range(args.frames)]
            medians[label].append(statistics.median(ms))
    for label, v in medians.items():
        print(json.dumps({"mode": label, "size": f"{w}x{h}", "kernel_ms_median": round(statistics.median(v), 4), "round_medians_min": round(min(v), 4),
                          "round_medians_max": round(max(v), 4), "rounds": args.rounds, "frames_per_round": args.frames}))
    for ctx in contexts:
        ctx.close()


if __name__ == "__main__":
    main()
