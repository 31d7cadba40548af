#!/usr/bin/env python3
"""What aic_pick_stale_cubes costs beside aic_pick_stale, and what a relight costs a resident frame, in ONE GPU command
(profiles/pick_stale_cubes_timing.txt).

usage: python tools/stale_cubes_timing.py [--calls 40]

tools/stale_timing.py's session: the 1920 x 1080 atrium frame of bench.py resident as an AIC_FRAME_OUT_SPLIT frame, the picker's order beside it, 1, 64
and 4096 changed cubes in view, one box of one cube each, expand = 1. The legs, alternating call by call after 5 calls of warm-up each, every call
blocking, n = max_stale = 65536: aic_pick_stale over the rectangles aic_stale_rects made on the host, and aic_pick_stale_cubes over the same boxes
(the device projects them), each without and with AIC_STALE_DEPTH_TEST; the lists of a pair are compared once. Then the 4096 cubes as LIGHT cubes,
without and with AIC_STALE_DEPTH_BEHIND. Wall time per call and the HIP-event time: 10th percentile, median, 90th.

Then a relight: a lamp block placed on an air cube in view (aic_update_cubes, aic_light_cubes_changed), aic_evaluate_light to convergence,
aic_light_changed_take, aic_pick_stale_cubes over the lamp's box and the reported cubes without and with AIC_STALE_DEPTH_BEHIND; and the displayed
frames of 65536 picks until the resident frame equals a fresh trace -- with the stale pixels first, and by the picker alone (from the pick at which
the last differing pixel comes up in PixelPicker's sequence)."""
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
    from all_is_cubes_amd import abi, flat

    sp, w, h, vd, cams = rt.cameras()
    lamp = sp.add_block(flat.atom((1.0, 1.0, 0.8, 1.0), emission=(8.0, 8.0, 6.0), name="lamp"))
    air = next(i for i, b in enumerate(sp.blocks) if b.is_air)
    count = w * h
    projection, view, inv = cams["traced"]
    vp = (view @ projection).reshape(16)
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(bloom_intensity=0.0, view_distance=vd))
        ctx.set_depth_transform(rt.depth_transform(projection, vd))
        frame = ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_SPLIT | abi.FRAME_NO_FEEDBACK)
        src = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(frame, src.data_ptr())
        aux = ctx.render(ctx.make_frame(256, 144, world_inv=inv), want_aux=True)["aux"].reshape(-1)
        hit = np.unique(aux["cube"][aux["hit"] != 0], axis=0).astype(np.int64)
        steps = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64)
        cubes = np.unique((hit[:, None, :] + steps[None, :, :]).reshape(-1, 3), axis=0)
        lo, size = np.asarray(sp.lo, np.int64), np.asarray(sp.size, np.int64)
        cubes = cubes[((cubes >= lo) & (cubes < lo + size)).all(axis=1)]
        if len(cubes) < BOX_COUNTS[-1]:
            raise SystemExit(f"only {len(cubes)} cubes in view")
        order, central, cycle = abi.pixel_order(w, h)
        order_dev = torch.from_numpy(order.view(np.int32)).cuda()
        out = torch.zeros(N, dtype=torch.int32, device="cuda")
        out2 = torch.zeros(N, dtype=torch.int32, device="cuda")
        boxes, rects = {}, {}
        for k in BOX_COUNTS:
            chosen = cubes[np.linspace(0, len(cubes) - 1, k).astype(np.int64)].astype(np.int32)
            boxes[k] = np.concatenate([chosen, chosen + 1], axis=1)
            rects[k] = abi.stale_rects(vp, w, h, boxes[k], 1)

        def old(k, fl, dst=out):
            return ctx.pick_stale(w, h, N, rects[k], src.data_ptr(), order_dev.data_ptr(), dst.data_ptr(), max_stale=N, flags=fl)

        def new(k, fl, dst=out, light=False):
            return ctx.pick_stale_cubes(vp, w, h, N, None if light else boxes[k], boxes[k][:, :3] if light else None, src.data_ptr(), order_dev.data_ptr(), dst.data_ptr(),
                                        max_stale=N, flags=fl)

        legs = {}
        for k in BOX_COUNTS:
            for name, fl in (("", 0), (", depth test", abi.STALE_DEPTH_TEST)):
                a, b = old(k, fl, out), new(k, fl, out2)
                same = bool((out == out2).all()) and (a.n_stale, a.n_from_stale, a.next_cursor) == (b.n_stale, b.n_from_stale, b.next_cursor)
                print(f"# {k} boxes{name}: lists identical {same}; n_rects {b.n_rects}, whole_frame {b.whole_frame}")
                legs[f"aic_pick_stale, {k} boxes{name}"] = lambda k=k, fl=fl: old(k, fl)
                legs[f"aic_pick_stale_cubes, {k} boxes{name}"] = lambda k=k, fl=fl: new(k, fl)
        for name, fl in (("", 0), (", behind test", abi.STALE_DEPTH_BEHIND)):
            legs[f"aic_pick_stale_cubes, 4096 light cubes{name}"] = lambda fl=fl: new(4096, fl, light=True)
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
        print(f"# {w} x {h} atrium, AIC_FRAME_OUT_SPLIT; {len(cubes)} cubes in view with their neighbours; n = max_stale = {N}; cycle_length {cycle}; {calls} blocking calls per leg, "
              f"alternating")
        for name in legs:
            i = last[name]
            print(f"{name:<52} " + json.dumps({"wall_ms_p10_p50_p90": q(wall[name]), "kernel_ms_p10_p50_p90": q(kernel[name]), "n_stale": i.n_stale, "n_from_stale": i.n_from_stale}),
                  flush=True)

        # a relight
        bi = np.asarray(sp.block_index)
        airs = [c for c in cubes if int(bi[tuple(c - lo)]) == air]
        site = np.asarray(airs[len(airs) // 2], np.int32)
        ctx.light_changed(abi.LAYER_WORLD)  # (nothing yet; the baseline is the uploaded volume)
        ctx.update_cubes(abi.LAYER_WORLD, [site], [lamp])
        ctx.light_cubes_changed(abi.LAYER_WORLD, [site], queue_order=0)
        t0 = time.perf_counter()
        li = ctx.evaluate_light(abi.LAYER_WORLD, 30, fast=False, epsilon=1, batch=8192, queue_order=0, queue=[])
        t1 = time.perf_counter()
        light_cubes, bounds = ctx.light_changed(abi.LAYER_WORLD)
        t2 = time.perf_counter()
        print(f"# relight: lamp at {site.tolist()}; {li.updates} updates in {li.batches} launches, {(t1 - t0) * 1e3:.2f} ms; {len(light_cubes)} light cubes reported, bounds "
              f"{bounds.tolist()}, count + take {(t2 - t1) * 1e3:.3f} ms")
        lamp_box = np.concatenate([site, site + 1])[None, :]
        for name, fl in (("rectangles alone", 0), ("behind test", abi.STALE_DEPTH_BEHIND)):
            ks, ws = [], []
            for _ in range(5 + calls):
                t0 = time.perf_counter()
                i = ctx.pick_stale_cubes(vp, w, h, N, lamp_box, light_cubes, src.data_ptr(), order_dev.data_ptr(), out.data_ptr(), max_stale=N, flags=fl)
                ws.append((time.perf_counter() - t0) * 1e3)
                ks.append(i.kernel_ms)
            print(f"relight, {name:<18} " + json.dumps({"wall_ms_p10_p50_p90": q(ws[5:]), "kernel_ms_p10_p50_p90": q(ks[5:]), "n_stale": i.n_stale, "of_pixels": count,
                                                         "n_rects": i.n_rects, "whole_frame": i.whole_frame}), flush=True)
        fresh = torch.zeros(count * 12, dtype=torch.uint8, device="cuda")
        ctx.render_to_device(frame, fresh.data_ptr())
        a, b = src.cpu().numpy(), fresh.cpu().numpy()
        differ = (a[:count * 8].view(np.uint64) != b[:count * 8].view(np.uint64)) | (a[count * 8:].view(np.uint32) != b[count * 8:].view(np.uint32))
        rank = np.empty(count, np.int64)
        rank[order] = np.arange(count)
        r = rank[differ]
        first_pick = np.where(r < central, 2 * r, 2 * (r - central) + 1) if central else r
        frames, skip = 0, 0
        while True:
            i = ctx.pick_stale_cubes(vp, w, h, N, lamp_box, light_cubes, src.data_ptr(), order_dev.data_ptr(), out.data_ptr(), max_stale=N, skip_stale=skip,
                                     flags=abi.STALE_DEPTH_BEHIND)
            if i.n_from_stale == 0:
                break
            ctx.trace_pixels_device(frame, i.n_from_stale, out.data_ptr(), src.data_ptr(), in_place=True)
            skip += i.n_from_stale
            frames += 1
        print("relight, frames of 65536 picks  " + json.dumps({"pixels_that_differ": int(differ.sum()), "stale_first_frames": frames,
                                                                "resident_equals_fresh_after": bool((src == fresh).all()),
                                                                "picker_alone_frames": int(-(-(int(first_pick.max()) + 1) // N)) if len(r) else 0}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    print(f"# command: python tools/stale_cubes_timing.py --calls {a.calls}")
    measure(a.calls)
    return 0


if __name__ == "__main__":
    sys.exit(main())
