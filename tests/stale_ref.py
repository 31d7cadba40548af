"""aic_stale_rects and aic_pick_stale restated in NumPy and Python numbers: DESIGN.md 4.17, written from include/aic_hip.h and not from the library's code.

The rule. A resident pixel's value depends only on the cubes its sample rays pass through and, at a lit surface, on the cubes within one cube of the hit
cube (the interpolated light stencil, the light-leak fix, ambient occlusion). Every sample ray of pixel (x, y) passes through an NDC point inside that
pixel's square. Under an unchanged light volume a changed box [lo, hi) can therefore only change a pixel whose square meets the screen-space bounding
rectangle of the projected box grown by one cube. `rects` makes those rectangles, `stale_mask` the stale set S of a frame under them, `pick_list` the
list aic_pick_stale must give entry for entry; the picker part is tests/pick_ref.py's."""
import math

import numpy as np

from tests import pick_ref

RECT_DTYPE = np.dtype([("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2"), ("dmin", "<f4"), ("reserved", "<u4")])
DEPTH_TEST = 1
MAX_RECTS = 4096
DMIN_MARGIN = 2.0 ** -24  # DESIGN.md 4.17 "The margin"


def _cell(v: float, n: int) -> int:
    """floor(v) clamped to [0, n]; v may be infinite"""
    return 0 if v <= 0.0 else (n if v >= float(n) else int(v))


def rect(vp, width: int, height: int, box, expand: int):
    """One box -> (x0, y0, x1, y1, dmin as np.float32). vp: 16 doubles, column-major, clip = M (x, y, z, 1)."""
    m = [float(v) for v in np.asarray(vp, np.float64).reshape(16)]
    lo, hi = [int(v) for v in box[:3]], [int(v) for v in box[3:]]
    empty = (0, 0, 0, 0, np.float32(0.0))
    if any(h <= l for l, h in zip(lo, hi)):
        return empty
    e = ([float(l - expand) for l in lo], [float(h + expand) for h in hi])  # (Python integers: no 32-bit overflow)
    nxs, nys, nzs = [], [], []
    for k in range(8):
        x, y, z = e[k & 1][0], e[(k >> 1) & 1][1], e[(k >> 2) & 1][2]
        clip = [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] for r in range(4)]
        if not clip[3] > 0.0 or not all(math.isfinite(c) for c in clip):
            return (0, 0, width, height, np.float32(-np.inf))
        with np.errstate(over="ignore"):
            q = np.array(clip[:3], np.float64) / np.float64(clip[3])  # (a quotient may overflow to infinity: the clamp takes it)
        nxs.append(float(q[0])); nys.append(float(q[1])); nzs.append(float(q[2]))
    ax, bx, ay, by, az = min(nxs), max(nxs), min(nys), max(nys), min(nzs)
    W, H = float(width), float(height)

    def fl(v):
        return v if math.isinf(v) else float(math.floor(v))

    x0, x1 = _cell(fl((ax + 1.0) / 2.0 * W) - 1.0, width), _cell(fl((bx + 1.0) / 2.0 * W) + 2.0, width)
    y0, y1 = _cell(fl((1.0 - by) / 2.0 * H) - 1.0, height), _cell(fl((1.0 - ay) / 2.0 * H) + 2.0, height)
    if x0 >= x1 or y0 >= y1:
        return empty
    lowered = az - DMIN_MARGIN
    with np.errstate(over="ignore"):
        d = np.float32(lowered)
    if float(d) > lowered:  # to nearest went up: one step down
        d = np.nextafter(d, np.float32(-np.inf))
    return (x0, y0, x1, y1, d)


def rects(vp, width: int, height: int, boxes, expand: int = 1) -> np.ndarray:
    boxes = np.asarray(boxes, np.int64).reshape(-1, 6)
    out = np.zeros(len(boxes), RECT_DTYPE)
    for i, b in enumerate(boxes):
        out[i]["x0"], out[i]["y0"], out[i]["x1"], out[i]["y1"], out[i]["dmin"] = rect(vp, width, height, b, expand)
    return out


def stale_mask(width: int, height: int, rect_list, color_bits=None, depth=None, flags: int = 0) -> np.ndarray:
    """S as a [height * width] bool. color_bits [H, W, 4] uint16 (f16 bit patterns) and depth [H, W] float32 are the frame's planes; only looked at with
    DEPTH_TEST, where rectangle b keeps pixel p out iff p's depth has a clear sign bit, p's alpha half is >= 1 and depth < b.dmin in f32."""
    s = np.zeros((height, width), bool)
    if flags & DEPTH_TEST:
        d = np.asarray(depth, np.float32).reshape(height, width)
        alpha = np.asarray(color_bits, np.uint16).reshape(height, width, 4)[..., 3].view(np.float16).astype(np.float32)
        with np.errstate(invalid="ignore"):
            front_able = ((d.view(np.uint32) >> 31) == 0) & (alpha >= np.float32(1.0))
    for r in np.asarray(rect_list, RECT_DTYPE).reshape(-1):
        x0, y0, x1, y1 = int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])
        if flags & DEPTH_TEST:
            with np.errstate(invalid="ignore"):
                kept_out = front_able[y0:y1, x0:x1] & (d[y0:y1, x0:x1] < np.float32(r["dmin"]))
            s[y0:y1, x0:x1] |= ~kept_out
        else:
            s[y0:y1, x0:x1] = True
    return s.reshape(-1)


def rank_list(mask, order):
    """s_0, s_1, ...: the pixels order[r], r ascending, that are in S (an entry >= count is never stale). order None: row-major."""
    mask = np.asarray(mask, bool).reshape(-1)
    order = np.arange(len(mask), dtype=np.uint32) if order is None else np.asarray(order, np.uint32)
    inside = order < len(mask)
    flags = np.zeros(len(order), bool)
    flags[inside] = mask[order[inside]]
    return order[flags]


def pick_list(width, height, order, n, rect_list=(), color_bits=None, depth=None, flags=0, max_stale=0, skip_stale=0, cursor=0, picker=None):
    """(pixels_out [n] uint32, dict of the aic_stale_info fields). The frame is looked at only with rectangles, max_stale > 0 and DEPTH_TEST.
    picker(n, cursor): a shared copy of the picker part, if the caller keeps one."""
    count = width * height
    if n == 0 or count == 0:
        return np.zeros(0, np.uint32), {"n_stale": 0, "next_cursor": 0, "n_from_stale": 0, "n_from_order": 0}
    look = max_stale > 0 and len(rect_list) > 0
    ranks = rank_list(stale_mask(width, height, rect_list, color_bits, depth, flags), order) if look else np.zeros(0, np.uint32)
    g = pick_ref.taken(n, max_stale, len(ranks), skip_stale)
    head = ranks[skip_stale:skip_stale + g] if g else np.zeros(0, np.uint32)
    if picker is not None:
        tail = picker(n - g, cursor)
    else:
        tail = np.array([pick_ref.pick(cursor + j, count, order) for j in range(n - g)], np.uint32)
    info = {"n_stale": len(ranks), "next_cursor": (cursor + n - g) % 2**64, "n_from_stale": g, "n_from_order": n - g}
    return np.concatenate([head, tail]).astype(np.uint32), info
