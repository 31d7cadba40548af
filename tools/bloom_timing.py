#!/usr/bin/env python3
"""What AIC_FRAME_BLOOM adds to a frame, timed with HIP events on the context's streams.

For the atrium-like scene at 1080p and 4K, with and without the flag (GraphicsOptions::default(): bloom 0.125):
  * single: one aic_render into device memory at a time, event to event around it;
  * streamed: N frames submitted on 4 slots in turn (aic_render_submit / aic_render_wait), the whole run event to event.
Prints one JSON line per case and the difference. Usage: python tools/bloom_timing.py [--frames N] [--repeat R]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import oracle  # noqa: E402
from all_is_cubes_amd import abi  # noqa: E402


def timed(fn, repeat):
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=9)
    args = ap.parse_args()
    sp, _, eye, target, vd, _ = bench.build_workload("atrium")
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(fog=3, view_distance=vd))
        for w, h in ((1920, 1080), (3840, 2160)):
            _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
            bufs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(4)]
            res = {}
            for flags in (0, abi.FRAME_BLOOM):
                frame = ctx.make_frame(w, h, world_inv=inv, flags=flags)
                for _ in range(3):  # warm: allocations, tile feedback
                    ctx.render_to_device(frame, bufs[0].data_ptr())

                def single():
                    ctx.render_to_device(frame, bufs[0].data_ptr())

                def streamed():
                    for i in range(args.frames):
                        s = i % 4
                        if i >= 4:
                            ctx.render_wait(s)
                        ctx.render_submit(frame, bufs[s].data_ptr(), s)
                    for s in range(min(4, args.frames)):
                        ctx.render_wait(s)

                res[flags] = (timed(single, args.repeat), timed(streamed, args.repeat) / args.frames)
                print(json.dumps({"size": f"{w}x{h}", "bloom": bool(flags), "single_ms": round(res[flags][0], 4),
                                  "streamed_ms_per_frame": round(res[flags][1], 4)}))
            print(json.dumps({"size": f"{w}x{h}", "bloom_adds_single_ms": round(res[abi.FRAME_BLOOM][0] - res[0][0], 4),
                              "bloom_adds_streamed_ms": round(res[abi.FRAME_BLOOM][1] - res[0][1], 4)}))


if __name__ == "__main__":
    main()
