"""aic_pick_stale_cubes and aic_probe_stale_cube_rects restated in NumPy and Python numbers: DESIGN.md 4.19, written from include/aic_hip.h and not from
the library's code. It builds on tests/stale_ref.py (the rank list) and tests/pick_ref.py (the picker part).

The rule. Changed BLOCKS are boxes, with aic_stale_rects' rectangle. A changed LIGHT texel at cube q, with the blocks as they are, can change only
pixels with a surface inside [q - 1, q + 2): the rectangle of the box [q, q + 1) grown by one, which also carries dmax, the greatest depth of the grown
box. A Split frame's depth texel is the depth of the pixel's NEAREST surface (over a ray's surfaces and over an antialiased pixel's four samples), so
with DEPTH_BEHIND a light rectangle keeps out a world pixel whose depth is beyond dmax: every surface of every sample lies behind the box."""
import math

import numpy as np

from tests import pick_ref, stale_ref

CUBE_RECT_DTYPE = np.dtype([("x0", "<u4"), ("y0", "<u4"), ("x1", "<u4"), ("y1", "<u4"), ("dmin", "<f4"), ("dmax", "<f4")])
DEPTH_TEST = 1
DEPTH_BEHIND = 2
MARGIN = 2.0 ** -24  # both depth bounds move outwards by this much before they are rounded outwards to f32


def _cell(v: float, n: int) -> int:
    """floor(v) clamped to [0, n]; v may be infinite"""
    return 0 if v <= 0.0 else (n if v >= float(n) else int(v))


def _floor(v: float) -> float:
    return v if math.isinf(v) else float(math.floor(v))


def rect(vp, width: int, height: int, box, expand: int):
    """One box -> (x0, y0, x1, y1, dmin, dmax), the depths np.float32. vp: 16 doubles, column-major, clip = M (x, y, z, 1). The bounds are Python
    integers: a light cube at the i32 edge has an upper bound of 2^31."""
    m = [float(v) for v in np.asarray(vp, np.float64).reshape(16)]
    lo, hi = [int(v) for v in box[:3]], [int(v) for v in box[3:]]
    empty = (0, 0, 0, 0, np.float32(0.0), np.float32(0.0))
    if any(h <= l for l, h in zip(lo, hi)):
        return empty
    e = ([float(l - expand) for l in lo], [float(h + expand) for h in hi])
    nxs, nys, nzs = [], [], []
    for k in range(8):
        x, y, z = e[k & 1][0], e[(k >> 1) & 1][1], e[(k >> 2) & 1][2]
        clip = [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] for r in range(4)]
        if not clip[3] > 0.0 or not all(math.isfinite(c) for c in clip):
            return (0, 0, width, height, np.float32(-np.inf), np.float32(np.inf))
        with np.errstate(over="ignore"):
            q = np.array(clip[:3], np.float64) / np.float64(clip[3])
        nxs.append(float(q[0])); nys.append(float(q[1])); nzs.append(float(q[2]))
    ax, bx, ay, by, az, bz = min(nxs), max(nxs), min(nys), max(nys), min(nzs), max(nzs)
    W, H = float(width), float(height)
    x0, x1 = _cell(_floor((ax + 1.0) / 2.0 * W) - 1.0, width), _cell(_floor((bx + 1.0) / 2.0 * W) + 2.0, width)
    y0, y1 = _cell(_floor((1.0 - by) / 2.0 * H) - 1.0, height), _cell(_floor((1.0 - ay) / 2.0 * H) + 2.0, height)
    if x0 >= x1 or y0 >= y1:
        return empty
    lowered, raised = az - MARGIN, bz + MARGIN
    with np.errstate(over="ignore"):
        dmin, dmax = np.float32(lowered), np.float32(raised)
    if float(dmin) > lowered:  # to nearest went up: one step down
        dmin = np.nextafter(dmin, np.float32(-np.inf))
    if float(dmax) < raised:  # to nearest went down: one step up
        dmax = np.nextafter(dmax, np.float32(np.inf))
    if dmin == np.float32(-np.inf):
        dmax = np.float32(np.inf)
    return (x0, y0, x1, y1, dmin, dmax)


def rects(vp, width: int, height: int, boxes=(), light_cubes=(), expand: int = 1) -> np.ndarray:
    """[n_boxes + n_light_cubes] CUBE_RECT_DTYPE records, the boxes' first: what aic_probe_stale_cube_rects copies back."""
    boxes = [[int(v) for v in b] for b in np.asarray(boxes, np.int64).reshape(-1, 6)]
    cubes = [[int(v) for v in q] for q in np.asarray(light_cubes, np.int64).reshape(-1, 3)]
    out = np.zeros(len(boxes) + len(cubes), CUBE_RECT_DTYPE)
    for i, b in enumerate(boxes):
        out[i] = rect(vp, width, height, b, expand)
    for i, q in enumerate(cubes):
        out[len(boxes) + i] = rect(vp, width, height, q + [v + 1 for v in q], 1)
    return out


def _usable(r, is_light: bool, flags: int):
    """(the front bound can keep a pixel out, the behind bound can)"""
    return bool(flags & DEPTH_TEST) and r["dmin"] > -np.inf, bool(flags & DEPTH_BEHIND) and is_light and r["dmax"] < np.inf


def whole_frame(width: int, height: int, rect_list, n_boxes: int, flags: int) -> bool:
    """some rectangle is the whole frame and has no depth bound the flags can use"""
    for i, r in enumerate(rect_list):
        if r["x0"] < r["x1"] and r["y0"] < r["y1"] and (r["x0"], r["y0"], r["x1"], r["y1"]) == (0, 0, width, height) and not any(_usable(r, i >= n_boxes, flags)):
            return True
    return False


def stale_mask(width: int, height: int, rect_list, n_boxes: int, color_bits=None, depth=None, flags: int = 0) -> np.ndarray:
    """S as a [height * width] bool. rect_list: rects()'s records, the first n_boxes of them boxes and the rest light cubes. The frame's planes
    (color_bits [H, W, 4] uint16, depth [H, W] float32) are only looked at with a depth flag."""
    s = np.zeros((height, width), bool)
    if flags & (DEPTH_TEST | DEPTH_BEHIND):
        d = np.asarray(depth, np.float32).reshape(height, width)
        alpha = np.asarray(color_bits, np.uint16).reshape(height, width, 4)[..., 3].view(np.float16).astype(np.float32)
        world = (d.view(np.uint32) >> 31) == 0
        with np.errstate(invalid="ignore"):
            front_able = world & (alpha >= np.float32(1.0))
        with np.errstate(invalid="ignore"):
            behind_able = world & (alpha > np.float32(-0.5))  # the gap fill's validity test: not NaN, not the marker's -1
    for i, r in enumerate(np.asarray(rect_list, CUBE_RECT_DTYPE).reshape(-1)):
        x0, y0, x1, y1 = int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])
        if x0 >= x1 or y0 >= y1:
            continue
        kept_out = np.zeros((y1 - y0, x1 - x0), bool)
        with np.errstate(invalid="ignore"):
            if flags & DEPTH_TEST:
                kept_out |= front_able[y0:y1, x0:x1] & (d[y0:y1, x0:x1] < np.float32(r["dmin"]))
            if (flags & DEPTH_BEHIND) and i >= n_boxes:
                kept_out |= behind_able[y0:y1, x0:x1] & (d[y0:y1, x0:x1] > np.float32(r["dmax"]))
        s[y0:y1, x0:x1] |= ~kept_out
    return s.reshape(-1)


def pick_list(vp, width, height, order, n, boxes=(), light_cubes=(), expand=1, color_bits=None, depth=None, flags=0, max_stale=0, skip_stale=0, cursor=0,
              picker=None, rect_list=None):
    """(pixels_out [n] uint32, dict of the aic_stale_cubes_info fields). rect_list: rects() of the same arguments, if the caller keeps one."""
    count = width * height
    zero = {"n_stale": 0, "next_cursor": 0, "n_from_stale": 0, "n_from_order": 0, "n_rects": 0, "whole_frame": 0}
    if n == 0 or count == 0:
        return np.zeros(0, np.uint32), zero
    n_boxes = len(np.asarray(boxes).reshape(-1, 6))
    n_total = n_boxes + len(np.asarray(light_cubes).reshape(-1, 3))
    look = max_stale > 0 and n_total > 0
    info = dict(zero)
    ranks = np.zeros(0, np.uint32)
    if look:
        rl = rects(vp, width, height, boxes, light_cubes, expand) if rect_list is None else rect_list
        ranks = stale_ref.rank_list(stale_mask(width, height, rl, n_boxes, color_bits, depth, flags), order)
        info["n_rects"] = int(((rl["x0"] < rl["x1"]) & (rl["y0"] < rl["y1"])).sum())
        info["whole_frame"] = int(whole_frame(width, height, rl, n_boxes, flags))
    g = pick_ref.taken(n, max_stale, len(ranks), skip_stale)
    head = ranks[skip_stale:skip_stale + g] if g else np.zeros(0, np.uint32)
    tail = picker(n - g, cursor) if picker is not None else np.array([pick_ref.pick(cursor + j, count, order) for j in range(n - g)], np.uint32)
    info.update(n_stale=len(ranks), next_cursor=(cursor + n - g) % 2**64, n_from_stale=g, n_from_order=n - g)
    return np.concatenate([head, tail]).astype(np.uint32), info
