#!/usr/bin/env python3
"""What finding the cursor costs, in ONE GPU command (profiles/cursor_raycast.txt).

usage: python tools/cursor_timing.py [--calls 1000] [--out profiles/cursor_raycast.txt]

bench.py's atrium with its light, uploaded once, seen by the bench's camera. Legs, each a blocking call timed with the host's wall clock around it,
alternating call by call after 20 calls of warm-up each:
  * aic_cursor_raycast with n = 1, the ray through the middle of the view, host pointers, at maximum_distance 6.0 and at infinity;
  * aic_cursor_raycast with n = 4096, a 64 x 64 grid of the camera's rays, AIC_RAYS_DEVICE (rays and records stay on the device), at infinity;
  * project_cursor(0, 0) through the host mirror (one UI-less renderer over the same space: one world raycast at 6.0 and the record's unpacking);
  * for scale, aic_sample_luminance with n = 10, max_steps = 60, host pointers, from the same build.
10th percentile, median, 90th; how many of the rays hit is printed beside them (tests/test_gpu_cursor.py compares the records' bits)."""
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

    import all_is_cubes_amd as A
    import bench
    import oracle
    from all_is_cubes_amd import _host as H
    from all_is_cubes_amd import abi

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    q = oracle.look_at_y_up(eye, target)
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, q, eye)
    ndc = (np.arange(64) + 0.5) / 32.0 - 1.0
    grid = np.array([np.concatenate(oracle.project_ndc_into_world(inv, float(x), float(y))) for y in ndc for x in ndc], np.float64)
    middle = np.concatenate(oracle.project_ndc_into_world(inv, 0.0, 0.0)).astype(np.float64)[None, :]
    inf = float("inf")

    cams = H.StandardCameras()
    cams.graphics_options = H.GraphicsOptions()
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(sp)
    cams.world_view_transform = H.look_at_y_up(tuple(eye), tuple(target))
    renderer = H.HipRtRenderer(cams)
    renderer.update()

    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        d_rays = torch.from_numpy(grid.copy()).to("cuda:0")
        d_out = torch.zeros(len(grid) * abi.CURSOR_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        exposure = abi.exposure_rays(q, eye, 1, 10)
        torch.cuda.synchronize()
        legs = {
            "aic_cursor_raycast n = 1    maximum_distance 6.0, host pointers": lambda: ctx.cursor_raycast(abi.LAYER_WORLD, middle, 6.0),
            "aic_cursor_raycast n = 1    maximum_distance inf, host pointers": lambda: ctx.cursor_raycast(abi.LAYER_WORLD, middle, inf),
            "aic_cursor_raycast n = 4096 maximum_distance inf, AIC_RAYS_DEVICE": lambda: ctx.cursor_raycast_device(abi.LAYER_WORLD, len(grid), d_rays.data_ptr(), inf, d_out.data_ptr()),
            "project_cursor(0, 0) through the host mirror": lambda: renderer.project_cursor(0.0, 0.0),
            "aic_sample_luminance n = 10 max_steps = 60, host pointers": lambda: ctx.sample_luminance(abi.LAYER_WORLD, exposure, 60),
        }
        for call in legs.values():
            for _ in range(20):
                call()
        wall = {name: [] for name in legs}
        for _ in range(calls):
            for name, call in legs.items():
                t0 = time.perf_counter()
                call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        pct = lambda v: [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])]
        n_voxel_blocks = sum(1 for b in sp.blocks if not b.is_one)
        say(f"# atrium {tuple(int(v) for v in sp.size)} cubes, {len(sp.blocks)} blocks ({n_voxel_blocks} with voxels), eye {tuple(eye)}; {calls} blocking calls per leg, alternating")
        records = ctx.cursor_raycast(abi.LAYER_WORLD, grid, inf)
        hits = records[records["hit"] == 1]
        say(f"# the 4096 rays at infinity: {len(hits)} hit, steps of a hit min {int(hits['steps'].min())} mean {float(hits['steps'].mean()):.1f} max {int(hits['steps'].max())}; "
            f"the middle ray at 6.0: {'a hit' if ctx.cursor_raycast(abi.LAYER_WORLD, middle, 6.0)[0]['hit'] else 'nothing'}, at infinity: "
            f"{'a hit' if ctx.cursor_raycast(abi.LAYER_WORLD, middle, inf)[0]['hit'] else 'nothing'}; project_cursor: {'a Cursor' if renderer.project_cursor(0.0, 0.0) else 'None'}")
        for name in legs:
            say(f"{name:<68} " + json.dumps({"wall_ms_p10_p50_p90": pct(wall[name])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cursor_raycast.txt"), help="the report is printed and written here")
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("# aic_cursor_raycast: one MI355X, one session (tools/cursor_timing.py; DESIGN.md 4.18)")
    say("#")
    say(f"# command: python tools/cursor_timing.py --calls {a.calls}")
    measure(a.calls, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
