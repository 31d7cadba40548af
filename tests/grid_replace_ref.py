"""aic_replace_cube_grid restated in NumPy: DESIGN.md 4.23, written from include/aic_hip.h and not from the library's code.

The rule. The caller's array replaces the block index of every cube. A cube has changed when its new index differs from the index it held -- plain
indices: tags and OPEN marks are the device's own and never count. The changed cubes are reported as aic_find_block_cubes reports its matches
(tests/stale_blocks_ref.py): runs along z inside one (x, y) row, sorted by the first entry's linear index, boxes with exclusive upper bounds, and the
capacity table of that call. What the grid holds afterwards is tests/cube_tags_ref.tagged_grid of the space with the new indices."""
import numpy as np

from tests import cube_tags_ref, stale_blocks_ref

ZERO_INFO = stale_blocks_ref.ZERO_INFO


def changed(old_index, new_index) -> np.ndarray:
    """[sx, sy, sz] bool"""
    old_index, new_index = np.asarray(old_index), np.asarray(new_index)
    assert old_index.shape == new_index.shape
    return old_index.astype(np.int64) != new_index.astype(np.int64)


def report(lo, old_index, new_index, capacity: int):
    """(boxes written [n_written, 6] int32, the aic_block_cubes_info fields but the time)"""
    m = changed(old_index, new_index)
    if not m.any():
        return np.zeros((0, 6), np.int32), dict(ZERO_INFO)
    r = stale_blocks_ref.runs(lo, m)
    at = np.argwhere(m) + np.asarray(lo, np.int64)
    bounds = np.concatenate([at.min(0), at.max(0) + 1]).astype(np.int32)
    merged = len(r) > capacity
    written = (bounds[None, :] if capacity >= 1 else np.zeros((0, 6), np.int32)) if merged else r
    return written, {"n_cubes": int(m.sum()), "n_runs": len(r), "bounds": bounds.tolist(), "n_written": len(written), "merged": int(merged)}


def replace(space, new_index, capacity: int, light=None):
    """Applies the call to a flat.FlatSpace in place; returns report()'s pair for it."""
    new_index = np.asarray(new_index, np.uint16).reshape(space.block_index.shape)
    if new_index.size and int(new_index.max()) >= len(space.blocks):
        raise ValueError("a block index at or above the layer's block count")
    out = report(space.lo, space.block_index, new_index, capacity)
    space.block_index[...] = new_index
    if light is not None:
        space.light[...] = np.asarray(light, np.uint8).reshape(space.light.shape)
    return out


def grid_after(space) -> np.ndarray:
    """u16 [sx, sy, sz]: what aic_probe_cube_grid must read after the call"""
    return cube_tags_ref.tagged_grid(space)
