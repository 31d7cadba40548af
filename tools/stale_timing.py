#!/usr/bin/env python3
"""What aic_pick_stale costs beside aic_pick_pixels, in ONE GPU command (profiles/pick_stale_timing.txt).

usage: python tools/stale_timing.py [--calls 40] [--parent DIR [--bench-steps 30]]

The 1920 x 1080 atrium frame of bench.py resident in device memory as an AIC_FRAME_OUT_SPLIT frame, the picker's order resident beside it. Changed cubes
in view: the cubes a 256 x 144 frame of the same camera hits first and their six neighbours inside the space (where a block is removed, and where one is
placed), 1, 64 and 4096 of them spread evenly over that list, one box of one cube each, turned into rectangles by aic_stale_rects with expand = 1.
The legs, alternating call by call after 5 calls of warm-up each, every call blocking:
aic_pick_stale with n = max_stale = 65536 for each box count, without and with AIC_STALE_DEPTH_TEST; the same session's aic_pick_pixels with
max_unknown = n after tools/reproject_timing.py's yaw of 0.02 rad, the yardstick the project already has; aic_stale_rects itself on the host; and
aic_reproject_split, for scale. Wall time per call and, where the call has one, the HIP-event time: 10th percentile, median, 90th.

With --parent (a built checkout of the parent commit): `bench.py --gpus 1 --no-cpu-baseline` of the parent, this tree, the parent, this tree."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
N = 65536
BOX_COUNTS = (1, 64, 4096)


def measure(calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import reproject_timing as rt
    from all_is_cubes_amd import abi

    sp, w, h, vd, cams = rt.cameras()
    count = w * h
    projection, view, inv = cams["traced"]
    vp = (view @ projection).reshape(16)
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(bloom_intensity=0.0, view_distance=vd))
        ctx.set_depth_transform(rt.depth_transform(projection, vd))
        flags = abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK
        src = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(ctx.make_frame(w, h, world_inv=inv, flags=flags), src.data_ptr())
        aux = ctx.render(ctx.make_frame(256, 144, world_inv=inv), want_aux=True)["aux"].reshape(-1)
        hit = np.unique(aux["cube"][aux["hit"] != 0], axis=0).astype(np.int64)
        steps = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64)
        cubes = np.unique((hit[:, None, :] + steps[None, :, :]).reshape(-1, 3), axis=0)
        lo, size = np.asarray(sp.lo, np.int64), np.asarray(sp.size, np.int64)
        cubes = cubes[((cubes >= lo) & (cubes < lo + size)).all(axis=1)]
        if len(cubes) < BOX_COUNTS[-1]:
            raise SystemExit(f"only {len(cubes)} cubes in view")
        m, zw = rt.reprojection(cams["traced"], cams["yaw 0.02 rad"])
        order, central, cycle = abi.pixel_order(w, h)
        order_dev = torch.from_numpy(order.view(np.int32)).cuda()
        out = torch.zeros(N, dtype=torch.int32, device="cuda")
        rinfo = ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr())
        boxes, rects = {}, {}
        for k in BOX_COUNTS:
            chosen = cubes[np.linspace(0, len(cubes) - 1, k).astype(np.int64)].astype(np.int32)
            boxes[k] = np.concatenate([chosen, chosen + 1], axis=1)
            rects[k] = abi.stale_rects(vp, w, h, boxes[k], 1)

        legs = {}
        for k in BOX_COUNTS:
            for name, fl in (("", 0), (", depth test", abi.STALE_DEPTH_TEST)):
                legs[f"aic_pick_stale, {k} boxes{name}"] = (
                    lambda k=k, fl=fl: ctx.pick_stale(w, h, N, rects[k], src.data_ptr(), order_dev.data_ptr(), out.data_ptr(), max_stale=N, flags=fl))
        legs["aic_pick_pixels, max_unknown = n (after the yaw)"] = lambda: ctx.pick_pixels(w, h, N, order_dev.data_ptr(), out.data_ptr(), max_unknown=N)
        legs["aic_stale_rects, 4096 boxes (host)"] = lambda: abi.stale_rects(vp, w, h, boxes[4096], 1)
        legs["aic_reproject_split, yaw 0.02 rad"] = lambda: ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr())
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
                if hasattr(info, "kernel_ms"):
                    kernel[name].append(info.kernel_ms)
                last[name] = info
        q = lambda v: [round(float(x), 4) for x in np.percentile(v, [10, 50, 90])] if v else None
        print(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT; {len(hit)} cubes hit first at 256 x 144, {len(cubes)} with their neighbours; n = max_stale = {N}; n_gaps of the yaw {rinfo.n_gaps}; "
              f"cycle_length {cycle}; {calls} blocking calls per leg, alternating")
        for name in legs:
            r = {"wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name])}
            i = last[name]
            if name.startswith("aic_pick_stale"):
                r.update({"n_stale": i.n_stale, "n_from_stale": i.n_from_stale, "n_from_order": i.n_from_order})
            elif name.startswith("aic_pick_pixels"):
                r.update({"n_unknown": i.n_unknown, "n_from_unknown": i.n_from_unknown})
            print(f"{name:<52} " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--parent", help="built checkout of the parent commit: also run bench.py of both trees, alternating")
    ap.add_argument("--bench-steps", type=int, default=30)
    a = ap.parse_args()
    print(f"# command: python tools/stale_timing.py --calls {a.calls}" + (f" --parent <parent checkout> --bench-steps {a.bench_steps}" if a.parent else ""))
    if a.parent:
        import reproject_timing as rt

        parent = os.path.abspath(a.parent)
        print("# bench.py --gpus 1 --no-cpu-baseline, alternating")
        for side, tree in (("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT)):
            print(f"bench {side:<6} " + json.dumps(rt.run_bench(tree, a.bench_steps)), flush=True)
    measure(a.calls)
    return 0


if __name__ == "__main__":
    sys.exit(main())
