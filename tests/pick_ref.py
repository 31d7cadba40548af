"""aic_pick_pixels restated in NumPy and Python integers: DESIGN.md 4.12, written from include/aic_hip.h and not from the kernels. The unknown set comes
from the reprojection's restatement (tests/reproject_ref.py: the splat image R and gf_valid); the picker part is the pick sequence written out under
aic_pixel_order. aic_pick_pixels must give these lists entry for entry."""
import numpy as np

from tests import reproject_ref

CENTRAL_MAX = 60000  # raytrace_to_texture.rs:838-908


def unknown(R):
    """U as a [count] bool: the texels of the splat image R [H, W, 4] u16 that fail the gap fill's validity test, !(alpha > -0.5)"""
    return ~reproject_ref.valid(R).reshape(-1)


def rank_list(R, order):
    """u_0, u_1, ...: the pixels order[r], r ascending, that are in U (an entry >= count is never unknown). order None: row-major."""
    u = unknown(R)
    order = np.arange(len(u), dtype=np.uint32) if order is None else np.asarray(order, np.uint32)
    inside = order < len(u)
    flags = np.zeros(len(order), bool)
    flags[inside] = u[order[inside]]
    return order[flags]


def taken(n, max_unknown, n_unknown, skip_unknown):
    """g = min(n, max_unknown, max(n_unknown - skip_unknown, 0))"""
    return min(int(n), int(max_unknown), max(int(n_unknown) - int(skip_unknown), 0))


def pick(k, count, order=None):
    """pick k of PixelPicker's sequence, in Python integers"""
    central = min(CENTRAL_MAX, count // 4)
    if central == 0:
        r = k % count
    elif k % 2 == 0:
        r = (k // 2) % central
    else:
        r = central + (k // 2) % (count - central)
    return r if order is None else int(order[r])


def pick_list(count, order, n, R=None, max_unknown=0, skip_unknown=0, cursor=0):
    """(pixels_out [n] uint32, dict of the aic_pick_info fields). R is looked at only with max_unknown > 0."""
    if n == 0 or count == 0:
        return np.zeros(0, np.uint32), {"n_unknown": 0, "next_cursor": 0, "n_from_unknown": 0, "n_from_order": 0}
    ranks = rank_list(R, order) if max_unknown > 0 else np.zeros(0, np.uint32)
    g = taken(n, max_unknown, len(ranks), skip_unknown)
    head = [int(v) for v in ranks[skip_unknown:skip_unknown + g]] if g else []
    tail = [pick(cursor + j, count, order) for j in range(n - g)]
    info = {"n_unknown": len(ranks), "next_cursor": (cursor + n - g) % 2**64, "n_from_unknown": g, "n_from_order": n - g}
    return np.array(head + tail, np.uint32), info
