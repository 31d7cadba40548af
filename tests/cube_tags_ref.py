"""The cube grid's tags and OPEN marks, restated in NumPy on a flat.FlatSpace (no device, no library code).

What the device keeps per layer (csrc/aic_device.h) and what aic_probe_cube_grid reads back:

* a class per block index, 2 bits each, 16 to a u32 word: 0 an invisible single voxel, 1 any other single voxel, 2 a recursive block;
* the cube grid, Z-major u16. With at most 16384 blocks an entry is `index | tag << 14`, the tag being the block's class plus one, and 0 --
  OPEN -- on every invisible cube that is not on the grid's outermost layer and whose six face neighbours are invisible too. With more
  blocks the entries are the plain indices.

A single-voxel block is one stored as Evoxels::One, or one of resolution 1, whose voxel is the one at [0, 0, 0] of its stored volume and AIR
if the volume does not contain that point (Evoxels::single_voxel, voxel_storage.rs:364-385). It is invisible when its alpha and its three
emission components are all zero (Evoxel::visible); the colour does not count. Every other block is recursive, whatever its voxels show."""
import numpy as np

TAG_SHIFT = 14
INDEX_MASK = (1 << TAG_SHIFT) - 1
MAX_TAGGED_BLOCKS = 1 << TAG_SHIFT
TAG_OPEN, TAG_INVISIBLE, TAG_VISIBLE, TAG_RECURSIVE = 0, 1, 2, 3


def block_class(b) -> int:
    if not b.is_one and b.resolution > 1:
        return 2
    if b.is_one:
        voxel = np.asarray(b.palette[0], np.float32)
    elif all(int(l) <= 0 < int(l) + int(s) for l, s in zip(b.vlo, b.voxels.shape)):
        x, y, z = (-int(l) for l in b.vlo)
        voxel = np.asarray(b.palette[int(b.voxels[x, y, z])], np.float32)
    else:
        voxel = np.zeros(8, np.float32)  # Evoxel::AIR
    return 0 if voxel[3] == 0 and voxel[4] == 0 and voxel[5] == 0 and voxel[6] == 0 else 1


def classes(blocks) -> np.ndarray:
    return np.array([block_class(b) for b in blocks], np.uint32)


def cls_words(blocks) -> np.ndarray:
    """The packed class table: ceil(n / 16) u32 words, block i in bits 2 (i % 16) .. 2 (i % 16) + 1 of word i // 16."""
    c = classes(blocks)
    c = np.concatenate([c, np.zeros(-len(c) % 16, np.uint32)]).reshape(-1, 16)
    return np.bitwise_or.reduce(c << (2 * np.arange(16, dtype=np.uint32)), axis=1).astype(np.uint32)


def is_tagged(sp) -> bool:
    return len(sp.blocks) <= MAX_TAGGED_BLOCKS


def open_cubes(sp) -> np.ndarray:
    """bool [sx, sy, sz]: the invisible cubes inside the outermost layer whose six face neighbours are invisible."""
    inv = classes(sp.blocks)[sp.block_index] == 0 if len(sp.blocks) else np.zeros(sp.block_index.shape, bool)
    p = np.pad(inv, 1, constant_values=False)  # (beyond the grid nothing is invisible: the outermost layer drops out by itself, and is excluded below anyway)
    m = inv & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]
    inner = np.zeros(inv.shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    return m & inner


def tagged_grid(sp) -> np.ndarray:
    """u16 [sx, sy, sz]: the grid as the device holds it."""
    index = sp.block_index.astype(np.uint32)
    if not is_tagged(sp):
        return index.astype(np.uint16)
    tag = classes(sp.blocks)[sp.block_index] + 1 if len(sp.blocks) else np.zeros(index.shape, np.uint32)
    tag = np.where(open_cubes(sp), TAG_OPEN, tag).astype(np.uint32)
    return (index | (tag << TAG_SHIFT)).astype(np.uint16)


def diff(got, want, tagged=True, show=4):
    """For a failure message: {"stale OPEN": (count, first coordinates), "missed OPEN": ..., "other": ...}. A stale OPEN -- the device says OPEN,
    the model INVISIBLE -- is a wrong picture; a missed one -- the device INVISIBLE, the model OPEN -- a lost optimisation; anything else is a
    wrong class or a wrong index. In an untagged grid every difference is of the last kind."""
    got, want = np.asarray(got, np.uint16).astype(np.uint32), np.asarray(want, np.uint16).astype(np.uint32)
    assert got.shape == want.shape, (got.shape, want.shape)
    same_index = ((got & INDEX_MASK) == (want & INDEX_MASK)) & bool(tagged)
    gt, wt = got >> TAG_SHIFT, want >> TAG_SHIFT
    stale = same_index & (gt == TAG_OPEN) & (wt == TAG_INVISIBLE)
    missed = same_index & (gt == TAG_INVISIBLE) & (wt == TAG_OPEN)
    other = (got != want) & ~stale & ~missed

    def some(mask):
        where = np.argwhere(mask)
        return int(len(where)), [tuple(int(v) for v in c) for c in where[:show]]

    return {"stale OPEN": some(stale), "missed OPEN": some(missed), "other": some(other)}


def n_differences(d) -> int:
    return sum(n for n, _ in d.values())
