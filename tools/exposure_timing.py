#!/usr/bin/env python3
"""What a step of automatic exposure costs, in ONE GPU command (profiles/exposure_sample.txt).

usage: python tools/exposure_timing.py [--calls 1000] [--out profiles/exposure_sample.txt]

bench.py's atrium with its light, uploaded once. Legs, each a blocking call timed with the host's wall clock around it, alternating call by call after 20
calls of warm-up each:
  * aic_sample_luminance with n = 10 (one step of State::step) and n = 100 (the whole grid), max_steps = 60, rays of aic_exposure_rays from the bench's eye
    and view, host pointers;
  * the same with AIC_RAYS_DEVICE (rays and samples stay on the device);
  * the host arithmetic of a step alone: aic_exposure_rays + aic_exposure_advance through ctypes.
Then, 50 times, the first sample after a scene change (aic_update_cubes of one cube with the block it already holds): the call that remakes the visible-block
bitmap. 10th percentile, median, 90th; the outcome counts of the restatement are not repeated here (tests/test_gpu_exposure.py compares the bits)."""
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
    from all_is_cubes_amd import abi

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    q = oracle.look_at_y_up(eye, target)
    state = abi.ExposureState()
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        n_voxel_blocks = sum(1 for b in sp.blocks if not b.is_one)
        rays = {10: abi.exposure_rays(q, eye, 1, 10), 100: abi.exposure_rays(q, eye, 0, 100)}
        d_rays = {n: torch.from_numpy(r.copy()).to("cuda:0") for n, r in rays.items()}
        d_out = torch.zeros(100, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()

        def host_step():
            r = state.rays(q, eye)
            state.advance(np.ones(10, np.float32), 0.1)
            return r

        legs = {}
        for n in (10, 100):
            legs[f"aic_sample_luminance n = {n:<3} max_steps = 60, host pointers"] = lambda n=n: ctx.sample_luminance(abi.LAYER_WORLD, rays[n], 60)
            legs[f"aic_sample_luminance n = {n:<3} max_steps = 60, AIC_RAYS_DEVICE"] = lambda n=n: ctx.sample_luminance_device(abi.LAYER_WORLD, n, d_rays[n].data_ptr(), 60, d_out.data_ptr())
        legs["aic_exposure_rays + aic_exposure_advance (host only)"] = host_step
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
        say(f"# atrium {tuple(int(v) for v in sp.size)} cubes, {len(sp.blocks)} blocks ({n_voxel_blocks} with voxels), eye {tuple(eye)}; {calls} blocking calls per leg, alternating")
        samples = ctx.sample_luminance(abi.LAYER_WORLD, rays[100], 60)
        say(f"# the 100 samples: min {float(samples.min()):.4f} mean {float(samples.mean()):.4f} max {float(samples.max()):.4f}")
        for name in legs:
            say(f"{name:<66} " + json.dumps({"wall_ms_p10_p50_p90": pct(wall[name])}))
        first = []
        cube = [tuple(int(v) for v in sp.lo)]
        block = [int(sp.block_index[0, 0, 0])]
        for _ in range(50):
            ctx.update_cubes(abi.LAYER_WORLD, cube, block)
            t0 = time.perf_counter()
            ctx.sample_luminance(abi.LAYER_WORLD, rays[10], 60)
            first.append((time.perf_counter() - t0) * 1e3)
        say(f"{'first aic_sample_luminance n = 10 after a scene change (bitmap remade)':<66} " + json.dumps({"wall_ms_p10_p50_p90": pct(first)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_sample.txt"), help="the report is printed and written here")
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("# aic_sample_luminance: one MI355X, one session (tools/exposure_timing.py; DESIGN.md 4.16)")
    say("#")
    say(f"# command: python tools/exposure_timing.py --calls {a.calls}")
    measure(a.calls, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
