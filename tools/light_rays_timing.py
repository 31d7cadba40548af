#!/usr/bin/env python3
"""What the light rays at the cursor cost, in ONE GPU command (profiles/light_rays.txt).

usage: python tools/light_rays_timing.py [--calls 300] [--out profiles/light_rays.txt]

bench.py's atrium with its light, uploaded once, seen by the bench's camera. The cursor is cursor_raycast of the ray through the middle of the view (at
6.0, or at infinity if nothing is struck that near); the cube asked about is its preceding cube. Legs, each a blocking call timed with the host's wall
clock around it, alternating call by call after 20 calls of warm-up each:
  * aic_cursor_raycast with n = 1 at that ray, host pointers (the call that finds the cube: for scale, from the same session);
  * aic_light_rays with n = 1 at maximum_distance 30: infos alone; infos, records and lines into host memory; records and lines into device memory;
  * aic_light_rays_cursor_lines: 28 host lines and the cube's behind them in the context's device list (what the mirror's present_split does first);
  * aic_light_rays with n = 4096 at maximum_distance 30, AIC_LIGHT_RAYS_DEVICE: the preceding cubes of a 64 x 64 grid of the camera's rays.
10th percentile, median, 90th; the records the calls produce are printed beside them (tests/test_gpu_light_rays.py compares their bits)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def measure(calls, say):
    sys.path.insert(0, ROOT)
    import ctypes as C

    import numpy as np
    import torch

    import bench
    import oracle
    from all_is_cubes_amd import abi

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    q = oracle.look_at_y_up(eye, target)
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, q, eye)
    ndc = (np.arange(64) + 0.5) / 32.0 - 1.0
    grid = np.array([np.concatenate(oracle.project_ndc_into_world(inv, float(x), float(y))) for y in ndc for x in ndc], np.float64)
    middle = np.concatenate(oracle.project_ndc_into_world(inv, 0.0, 0.0)).astype(np.float64)[None, :]
    inf = float("inf")
    md = 30

    def preceding(rec):
        return tuple(int(v) for v in (rec["preceding_cube"] if rec["has_preceding"] else rec["cube"]))

    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        reach = 6.0 if ctx.cursor_raycast(abi.LAYER_WORLD, middle, 6.0)[0]["hit"] else inf
        cursor = ctx.cursor_raycast(abi.LAYER_WORLD, middle, reach)[0]
        if not cursor["hit"]:
            raise SystemExit("the middle ray strikes nothing")
        cube = np.array([preceding(cursor)], np.int32)
        hits = [r for r in ctx.cursor_raycast(abi.LAYER_WORLD, grid, inf) if r["hit"]]
        many = np.array([preceding(hits[i % len(hits)]) for i in range(4096)], np.int32)
        bound = abi.light_rays_bound(md)
        one_infos, one_rays, one_lines, one_totals = ctx.light_rays(abi.LAYER_WORLD, cube, md)
        many_infos, many_totals = ctx.light_rays_device(abi.LAYER_WORLD, many, md, 0, 0, 0)
        capacity = many_totals[0]
        d_rays = torch.zeros(max(capacity, bound) * 40, dtype=torch.uint8, device="cuda:0")
        d_lines = torch.zeros(56 * (12 * len(many) + 29 * max(capacity, bound)), dtype=torch.uint8, device="cuda:0")
        first = np.zeros(2 * 28, abi.LINE_VERTEX_DTYPE)
        lib = abi.load()
        lib.aic_light_rays_cursor_lines.restype = C.c_int
        lib.aic_light_rays_cursor_lines.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        list_ptr, list_n = C.c_void_p(), C.c_uint32()

        def cursor_lines():
            rc = lib.aic_light_rays_cursor_lines(ctx._h, abi.LAYER_WORLD, cube.ctypes.data, md, first.ctypes.data, 28, None, C.byref(list_ptr), C.byref(list_n))
            assert rc == 0 and list_n.value == 28 + one_totals[1]

        torch.cuda.synchronize()
        legs = {
            f"aic_cursor_raycast n = 1    maximum_distance {reach}, host pointers": lambda: ctx.cursor_raycast(abi.LAYER_WORLD, middle, reach),
            "aic_light_rays n = 1    distance 30, infos alone": lambda: ctx.light_rays_device(abi.LAYER_WORLD, cube, md, 0, 0, 0),
            "aic_light_rays n = 1    distance 30, records and lines to the host": lambda: ctx.light_rays(abi.LAYER_WORLD, cube, md, capacity=bound),
            "aic_light_rays n = 1    distance 30, AIC_LIGHT_RAYS_DEVICE": lambda: ctx.light_rays_device(abi.LAYER_WORLD, cube, md, bound, d_rays.data_ptr(), d_lines.data_ptr()),
            "aic_light_rays_cursor_lines distance 30, 28 lines first": cursor_lines,
            "aic_light_rays n = 4096 distance 30, AIC_LIGHT_RAYS_DEVICE": lambda: ctx.light_rays_device(abi.LAYER_WORLD, many, md, capacity, d_rays.data_ptr(), d_lines.data_ptr()),
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
        say(f"# atrium {tuple(int(v) for v in sp.size)} cubes, {len(sp.blocks)} blocks, eye {tuple(eye)}; {calls} blocking calls per leg, alternating")
        say(f"# the cursor: cube {tuple(int(v) for v in cursor['cube'])} at {float(cursor['distance_to_point']):.3f}, preceding cube {tuple(int(v) for v in cube[0])}: "
            f"{one_totals[0]} records, {one_totals[1]} lines, cost {int(one_infos['cost'][0])}, result {tuple(int(v) for v in one_infos['result'][0])}; the bound at distance 30 is {bound}")
        say(f"# the 4096 cubes ({len(hits)} of the grid's rays hit; their preceding cubes, repeated): {many_totals[0]} records, {many_totals[1]} lines, "
            f"most of one cube {int(many_infos['n_rays'].max())}, cost mean {float(many_infos['cost'].mean()):.0f}")
        for name in legs:
            say(f"{name:<68} " + json.dumps({"wall_ms_p10_p50_p90": pct(wall[name])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_rays.txt"), help="the report is printed and written here")
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("# aic_light_rays: one MI355X, one session (tools/light_rays_timing.py; DESIGN.md 4.21)")
    say("#")
    say(f"# command: python tools/light_rays_timing.py --calls {a.calls}")
    measure(a.calls, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
