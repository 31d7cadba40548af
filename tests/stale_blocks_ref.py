"""aic_find_block_cubes and aic_pick_stale_blocks restated in NumPy: DESIGN.md 4.20, written from include/aic_hip.h and not from the library's code. It
composes with tests/stale_cubes_ref.py for the pick list.

The rule. A re-evaluated block leaves the cube grid as it is and changes what the cubes holding its index look like. Those cubes are found in the grid
(a flat.FlatSpace's block_index here: plain indices, no tags) as runs along z: maximal stretches of consecutive matching entries inside one (x, y) row,
sorted by the first entry's linear index (x * sy + y) * sz + z, each the box {lo + (x, y, z0), lo + (x + 1, y + 1, z1)}."""
import numpy as np

from tests import stale_cubes_ref

ZERO_INFO = {"n_cubes": 0, "n_runs": 0, "bounds": [0] * 6, "n_written": 0, "merged": 0}


def match(space, indices) -> np.ndarray:
    """[sx, sy, sz] bool: the cube's block index is one of `indices` (duplicates are legal)"""
    return np.isin(np.asarray(space.block_index), np.asarray(list(indices), np.int64).reshape(-1))


def runs(lo, m: np.ndarray) -> np.ndarray:
    """[n_runs, 6] int32 boxes of the match array m [sx, sy, sz], lower corner lo"""
    sx, sy, sz = m.shape
    if m.size == 0:
        return np.zeros((0, 6), np.int32)
    padded = np.zeros((sx, sy, sz + 2), bool)  # a row never continues into the next
    padded[:, :, 1:-1] = m
    starts = np.argwhere(padded[:, :, 1:-1] & ~padded[:, :, :-2])  # argwhere: ascending in (x, y, z), the linear order
    ends = np.argwhere(padded[:, :, 1:-1] & ~padded[:, :, 2:])
    assert len(starts) == len(ends) and (starts[:, :2] == ends[:, :2]).all()
    out = np.zeros((len(starts), 6), np.int64)
    out[:, :3] = starts + np.asarray(lo, np.int64)
    out[:, 3:5] = out[:, :2] + 1
    out[:, 5] = ends[:, 2] + 1 + int(lo[2])
    return out.astype(np.int32)


def find(space, indices, capacity: int):
    """(boxes written [n_written, 6] int32, the aic_block_cubes_info fields but the time)"""
    m = match(space, indices)
    if not m.any():
        return np.zeros((0, 6), np.int32), dict(ZERO_INFO)
    r = runs(space.lo, m)
    at = np.argwhere(m) + np.asarray(space.lo, np.int64)
    bounds = np.concatenate([at.min(0), at.max(0) + 1]).astype(np.int32)
    merged = len(r) > capacity
    written = (bounds[None, :] if capacity >= 1 else np.zeros((0, 6), np.int32)) if merged else r
    return written, {"n_cubes": int(m.sum()), "n_runs": len(r), "bounds": bounds.tolist(), "n_written": len(written), "merged": int(merged)}


def pick_list(space, indices, max_runs, vp, width, height, order, n, boxes=(), light_cubes=(), expand=1, color_bits=None, depth=None, flags=0, max_stale=0,
              skip_stale=0, cursor=0, picker=None):
    """(pixels_out [n] uint32, aic_stale_cubes_info fields, aic_block_cubes_info fields): aic_pick_stale_cubes for `boxes` followed by the found boxes.
    Nothing is found when nothing is looked at (n = 0 or max_stale = 0)."""
    own = np.asarray(boxes if boxes is not None else [], np.int32).reshape(-1, 6)
    light_cubes = light_cubes if light_cubes is not None else ()
    indices = list(indices) if indices is not None else []
    found, info = (find(space, indices, max_runs) if n and max_stale and len(indices) else (np.zeros((0, 6), np.int32), dict(ZERO_INFO)))
    out, pick = stale_cubes_ref.pick_list(vp, width, height, order, n, np.concatenate([own, found]), light_cubes, expand, color_bits, depth, flags, max_stale, skip_stale,
                                          cursor, picker)
    return out, pick, info
