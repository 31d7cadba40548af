"""The cube grid's tags and OPEN marks against a host model, at every step of sequences of scene calls (run with -m gpu on an MI355X).

aic_probe_cube_grid reads the grid, the 2-bit class table and the tagged flag back from the device; tests/cube_tags_ref.py restates all three
from the flat.FlatSpace a sequence has arrived at. After every call that touches the scene the whole u16 grid must equal the restatement -- a
stale OPEN mark (a wrong picture for the few rays that meet it) and a missed one (only slower, and invisible to every frame) fail alike, and the
failure message says which it is (cube_tags_ref.diff). At marked steps the grid must also equal that of a fresh context that uploads the model's
space, and the frames of tests/test_gpu_open_cubes.py's check() must be the oracle's: the probe makes this file complete, the frames keep it honest.

The sequences are plain data made from the model alone (scripted_updates, scripted_replacements, random_sequence), so that
tests/test_cube_tags_cpu.py can show without a device that they meet the cases they are there for. Every aic_update_cubes batch names distinct
cubes, or the same cube twice with the same value."""
import copy
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest

from all_is_cubes_amd import abi, flat
from tests import cube_tags_ref as ref
from tests.test_gpu_first_lookup import camera, shell_block
from tests.test_gpu_open_cubes import GRID, INVISIBLE_AT, RECURSIVE_AT, SIZE, VD, VISIBLE_AT, air_grid, check

pytestmark = pytest.mark.gpu

LO = (-7, 3, -20)
WORLD = abi.LAYER_WORLD
AIC_ERR_INVALID = 1
SMALL_GRIDS = ((1, 1, 1), (2, 5, 5), (1, 9, 9), (3, 3, 3), (3, 3, 40))
BATCH_LENGTHS = (1, 31, 32, 33, 300)  # open_changed_cubes_kernel runs 8 threads per change: 32 changes fill one 256-thread block exactly
N_SEEDS = int(os.environ.get("AIC_CUBE_TAGS_N", "4"))
SEED_BASE = 4100
N_RANDOM_STEPS = 40
# eye, target, field of view, in cubes from the grid's lower corner: inside the grid, down its long axis
VIEW_Z = ((4.5, 3.5, 9.6), (4.45, 3.45, 0.0), 60.0)
VIEW_X = ((0.6, 3.4, 5.6), (8.0, 3.5, 5.4), 70.0)


# --- scenes -----------------------------------------------------------------------------------------------------------------------------
def ghost_block():
    """A recursive block of invisible voxels only: nothing to see, and recursive all the same."""
    return flat.voxel_block(2, np.zeros((2, 2, 2), np.uint16), flat.evoxel((0, 0, 0, 0))[None, :])


def hollow_block():
    """A resolution-1 block whose stored volume does not contain [0, 0, 0]: its single voxel is AIR."""
    return flat.BlockDef(1, (0, 0, 0), np.zeros((0, 1, 1), np.uint16), np.zeros((0, 8), np.float32))


def scene(size=GRID, lo=LO):
    """air_grid of test_gpu_open_cubes.py at `lo`, with the awkward blocks added to its table: (space, {name: block index})."""
    sp, a, visible, recursive, unseen = air_grid(size)
    sp.lo = tuple(lo)
    ix = dict(air=a, visible=visible, recursive=recursive, unseen=unseen)
    ix["tinted"] = sp.add_block(flat.atom((0.3, 0.9, 0.4, 0.0), name="tinted"))  # alpha 0 and a colour: invisible
    ix["glow"] = sp.add_block(flat.atom((0.0, 0.0, 0.0, 0.0), (0.0, 0.4, 0.1), name="glow"))  # alpha 0 and an emission: visible
    ix["hollow"] = sp.add_block(hollow_block())
    ix["ghost"] = sp.add_block(ghost_block())
    return sp, ix


def world(cube, lo=LO):
    return tuple(int(c) + int(l) for c, l in zip(cube, lo))


def point(p, lo=LO):
    return tuple(float(c) + float(l) for c, l in zip(p, lo))


# --- operations on the scene, as data ---------------------------------------------------------------------------------------------------
def cubes(xyz, block=None, light=None):
    """One aic_update_cubes batch: world coordinates [n, 3], block indices [n] or None, texels [n, 4] or None."""
    return ("cubes", np.asarray(xyz, np.int32).reshape(-1, 3), None if block is None else np.asarray(block, np.uint16).reshape(-1),
            None if light is None else np.asarray(light, np.uint8).reshape(-1, 4))


def blocks(*items):
    """One aic_replace_blocks call: (index, flat.BlockDef) pairs; index == len(table) appends."""
    return ("blocks", list(items))


COMPACT = ("compact",)


@dataclass
class Step:
    what: str
    op: tuple
    unchanged: bool = False  # the grid is bit for bit what it was before the call
    fresh: bool = False  # ... and equals the grid of a fresh context that uploads the model's space
    view: Optional[tuple] = None  # ... and the frames from there are the oracle's


def apply_to_model(sp, op):
    """What the call means, on the FlatSpace (in place): the cubes of a batch that lie in the space get its values, in order."""
    kind = op[0]
    if kind == "cubes":
        _, xyz, bi, lt = op
        for i, c in enumerate(xyz):
            p = tuple(int(v) - int(l) for v, l in zip(c, sp.lo))
            if all(0 <= v < s for v, s in zip(p, sp.size)):
                if bi is not None:
                    sp.block_index[p] = bi[i]
                if lt is not None:
                    sp.light[p] = lt[i]
    elif kind == "blocks":
        for index, block in op[1]:
            if index == len(sp.blocks):
                sp.blocks.append(block)
            else:
                sp.blocks[index] = block
    else:
        assert kind == "compact", kind
    return sp


def apply_to_device(ctx, op):
    kind = op[0]
    if kind == "cubes":
        ctx.update_cubes(WORLD, op[1], op[2], op[3])
    elif kind == "blocks":
        if len(op[1]) == 1:
            ctx.replace_block(WORLD, op[1][0][0], op[1][0][1])
        else:
            ctx.replace_blocks(WORLD, op[1])
    else:
        assert kind == "compact", kind
        ctx.compact(WORLD)


# --- the assertions of a step -----------------------------------------------------------------------------------------------------------
def assert_grid(ctx, sp, what):
    """The three assertions after every call: the grid, the class table and the tagged flag are the restatement's. Returns the grid."""
    grid, cls, tagged = ctx.probe_cube_grid(WORLD, sp.size, len(sp.blocks))
    want = ref.tagged_grid(sp)
    d = ref.diff(grid, want, ref.is_tagged(sp))
    assert not ref.n_differences(d), (what, d)
    assert grid.dtype == want.dtype and (grid == want).all(), what
    want_cls = ref.cls_words(sp.blocks)
    assert (cls == want_cls).all(), (what, "class table", np.flatnonzero(cls != want_cls)[:4])
    assert tagged == ref.is_tagged(sp), (what, "tagged", tagged)
    return grid


def assert_fresh(sp, grid, what):
    """The reference's own invariant: the updated snapshot is the fresh snapshot."""
    with abi.Context(0) as fresh:
        fresh.upload_space(WORLD, sp)
        got, cls, tagged = fresh.probe_cube_grid(WORLD, sp.size, len(sp.blocks))
    d = ref.diff(grid, got, tagged)
    assert not ref.n_differences(d), (what, "against a fresh context's upload", d)
    assert (grid == got).all(), what


def frames(ctx, sp, view, what):
    eye, target, fov = view
    counts = check(ctx, sp, SIZE, camera(SIZE, point(eye, sp.lo), point(target, sp.lo), fov=fov, view_distance=VD), what, upload=False)
    assert counts.max() >= 6, what  # rays long enough to have crossed the grid


def run(ctx, sp0, steps):
    sp = copy.deepcopy(sp0)
    ctx.upload_space(WORLD, sp)
    before = assert_grid(ctx, sp, "the upload")
    for k, s in enumerate(steps):
        what = f"step {k + 1}: {s.what}"
        apply_to_device(ctx, s.op)
        sp = apply_to_model(sp, s.op)
        grid = assert_grid(ctx, sp, what)
        if s.unchanged:
            assert grid.shape == before.shape and (grid == before).all(), (what, "the grid changed", ref.diff(grid, before))
        if s.fresh:
            assert_fresh(sp, grid, what)
        if s.view is not None:
            frames(ctx, sp, s.view, what)
            assert (ctx.probe_cube_grid(WORLD, sp.size, len(sp.blocks))[0] == grid).all(), (what, "frames changed the grid")
        before = grid
    return sp


# --- the scripted sequences -------------------------------------------------------------------------------------------------------------
def scripted_updates():
    """(space, steps): the aic_update_cubes cases, one batch per step."""
    sp, ix = scene()
    a, visible, recursive, unseen = ix["air"], ix["visible"], ix["recursive"], ix["unseen"]
    sp.set(world(RECURSIVE_AT), recursive)
    sp.set(world((2, 4, 3)), visible)
    lo, hi = np.array(sp.lo), np.array(sp.hi)
    spot = (4, 3, 5)
    steps = [Step("a visible block into the middle of an open region", cubes([world(spot)], [visible])),
             Step("... and out again", cubes([world(spot)], [a])),
             Step("a visible block that came with the upload taken out", cubes([world((2, 4, 3))], [a]))]
    cluster = [(x, y, z) for x in (4, 5) for y in (3, 4) for z in (5, 6)]
    steps.append(Step("a 2 x 2 x 2 cluster of visible blocks", cubes([world(c) for c in cluster], [visible, ix["glow"], recursive, visible, ix["ghost"], visible, visible, recursive]),
                      fresh=True, view=VIEW_Z))
    steps.append(Step("four of the cluster removed", cubes([world(c) for c in cluster[::2]], [a, unseen, a, ix["hollow"]])))
    steps.append(Step("a line of 11 along z, through layer 1 and the outermost layer at both ends", cubes([world((6, 2, z)) for z in range(GRID[2])], [visible] * GRID[2]),
                      fresh=True, view=VIEW_Z))
    # cubes outside the space beside cubes inside it: one below, at, far below and far above the bounds on each axis, with the two cubes of the
    # outermost layer next to them -- whose own neighbours, on layer 1, stop being open
    xyz, bi = [], []
    mid = world((4, 3, 8))
    for axis in range(3):
        for v in (lo[axis] - 1, hi[axis], lo[axis] - 1000, hi[axis] + 1000):
            c = list(mid)
            c[axis] = int(v)
            xyz.append(c)
            bi.append(visible)
        for v in (lo[axis], hi[axis] - 1):
            c = list(mid)
            c[axis] = int(v)
            xyz.append(c)
            bi.append(visible)
    steps.append(Step("cubes outside the space beside cubes on its outermost layer", cubes(xyz, bi), fresh=True))
    rng = np.random.default_rng(11)
    some = [world(c) for c in ((1, 1, 1), (4, 3, 5), (7, 5, 9), (6, 2, 4), (0, 0, 0), (8, 6, 10))]
    steps.append(Step("a light-only batch", cubes(some + [world((-1, 3, 5))], None, rng.integers(60, 250, (7, 4))), unchanged=True))
    steps.append(Step("a block-only batch", cubes([world(c) for c in ((1, 1, 1), (1, 2, 1), (7, 5, 9))], [visible, unseen, recursive])))
    steps.append(Step("a block-and-light batch", cubes([world(c) for c in ((1, 1, 1), (2, 1, 1), (7, 5, 8), (3, 5, 2))], [a, ix["glow"], ix["tinted"], visible],
                                                       rng.integers(60, 250, (4, 4)))))
    # (what each cube holds by now: the model is run here to know)
    cur = copy.deepcopy(sp)
    for s in steps:
        cur = apply_to_model(cur, s.op)
    same = [(4, 3, 5), (6, 2, 4), (2, 3, 7), (1, 2, 1), (0, 3, 8), (3, 3, 3), (4, 3, 5)]
    assert ref.open_cubes(cur)[3, 3, 3] and ref.classes(cur.blocks)[cur.block_index[6, 2, 4]] == 1
    steps.append(Step("cubes set to the block they already hold, one of them twice", cubes([world(c) for c in same], [cur.block_index[c] for c in same]), unchanged=True))
    steps.append(Step("visible cubes turned into the invisible atom that is not air", cubes([world((6, 2, z)) for z in (4, 5, 6)] + [world((4, 4, 6))], [unseen] * 4)))
    # batches of 1, 31, 32, 33 and 300 distinct cubes, mostly air with a few blocks of every kind
    every = np.array([(x, y, z) for x in range(GRID[0]) for y in range(GRID[1]) for z in range(GRID[2])])
    kinds = np.array([a] * 16 + [unseen, ix["tinted"], ix["hollow"], visible, recursive, ix["glow"], ix["ghost"]], np.uint16)
    for n in BATCH_LENGTHS:
        pick = every[rng.permutation(len(every))[:n]] + lo
        steps.append(Step(f"a batch of {n} distinct cubes", cubes(pick, rng.choice(kinds, n)), fresh=n in (32, 300)))
    return sp, steps


def scripted_replacements():
    """(space, steps): the aic_replace_block(s) and aic_compact cases."""
    sp, ix = scene()
    a, visible, recursive, unseen = ix["air"], ix["visible"], ix["recursive"], ix["unseen"]
    sp.set(world(VISIBLE_AT), visible)
    sp.set(world(RECURSIVE_AT), recursive)
    sp.set(world(INVISIBLE_AT), unseen)
    sp.set(world((3, 5, 8)), visible)
    sp.set(world((1, 1, 9)), unseen)
    glass = flat.atom((0.2, 0.6, 0.9, 0.02))
    n = len(sp.blocks)
    steps = [
        Step("a block replaced by one of the same class", blocks((visible, flat.atom((0.1, 0.8, 0.3, 0.7)))), unchanged=True),
        Step("invisible -> visible on the block most cubes hold", blocks((a, glass)), fresh=True, view=VIEW_Z),
        Step("... and back", blocks((a, flat.air())), fresh=True, view=VIEW_Z),
        Step("atom -> recursive", blocks((visible, shell_block(4, alpha=0.7))), fresh=True, view=VIEW_X),
        Step("recursive -> invisible atom", blocks((recursive, flat.atom((0.5, 0.5, 0.5, 0.0), name="gone"))), fresh=True, view=VIEW_X),
        Step("two class changes in one call", blocks((recursive, shell_block(2, alpha=0.4)), (unseen, flat.atom((0.9, 0.9, 0.1, 1.0)))), fresh=True, view=VIEW_Z),
        Step("a block appended", blocks((n, flat.atom((0.3, 0.2, 0.9, 0.8)))), unchanged=True),
        Step("... and placed", cubes([world((5, 4, 4)), world((5, 4, 5))], [n, n]), fresh=True),
        Step("a recursive block that outgrows its ranges", blocks((visible, shell_block(8, alpha=0.7))), unchanged=True),
        Step("a second one, its class changing too", blocks((n, shell_block(8, alpha=0.3)))),
        Step("aic_compact over the garbage they left", COMPACT, unchanged=True, fresh=True),
        Step("a cube placed after the compaction", cubes([world((5, 4, 6))], [recursive])),
    ]
    return sp, steps


# --- random sequences -------------------------------------------------------------------------------------------------------------------
def seeds(n=N_SEEDS):
    return [SEED_BASE + i for i in range(n)]


def visible_fill(sp):
    return float((ref.classes(sp.blocks)[sp.block_index] != 0).mean())


def _random_block(rng, kind):
    c = [float(v) for v in rng.uniform(0.05, 0.95, 3)]
    if kind == 0:
        return [flat.atom((c[0], c[1], c[2], 0.0), name="r"), hollow_block(), flat.atom((0.0, 0.0, 0.0, 0.0), name="r")][int(rng.integers(3))]
    if kind == 1:
        return [flat.atom((c[0], c[1], c[2], float(rng.uniform(0.1, 1.0)))), flat.atom((0.0, 0.0, 0.0, 0.0), (c[0], 0.0, c[2]))][int(rng.integers(2))]
    return [shell_block(2, alpha=0.6), shell_block(4, alpha=1.0), ghost_block()][int(rng.integers(3))]


def _random_batch(rng, cur):
    """1 to 60 distinct cubes, half of them around a random centre (so that changed cubes are neighbours of each other, of the rim and of cubes
    outside the space), the others anywhere in the space and the layer of cubes around it."""
    size, lo = np.array(cur.size), np.array(cur.lo)
    m = int(rng.integers(1, 61))
    centre = rng.integers(0, size)
    offsets = np.array([(x, y, z) for x in range(-2, 3) for y in range(-2, 3) for z in range(-2, 3)])
    near = centre + offsets[rng.permutation(len(offsets))[:m // 2]]
    far = np.stack([rng.integers(-1, s + 1, m - m // 2) for s in size], axis=1)
    xyz = np.unique(np.concatenate([near, far]), axis=0)
    xyz = xyz[rng.permutation(len(xyz))]
    cls = ref.classes(cur.blocks)
    seen, unseen = np.flatnonzero(cls != 0), np.flatnonzero(cls == 0)
    fill = visible_fill(cur)
    p = 0.3 if fill < 0.045 else (0.0 if fill > 0.075 else 0.08)
    air = next(i for i, b in enumerate(cur.blocks) if b.is_air)
    bi = np.where(rng.random(len(xyz)) < p, rng.choice(seen, len(xyz)), np.where(rng.random(len(xyz)) < 0.7, air, rng.choice(unseen, len(xyz)))).astype(np.uint16)
    mode = rng.random()
    light = rng.integers(100, 230, (len(xyz), 4)) if mode > 0.6 else None
    if light is not None:
        light[:, 3] = flat.STATUS_VISIBLE
    what = f"a batch of {len(xyz)} cubes" + (", blocks only" if light is None else ", light only" if mode > 0.8 else ", blocks and light")
    return what, cubes(xyz + lo, None if mode > 0.8 else bi, light)


def _random_replacement(rng, cur, toggles):
    """A block that some cubes hold changes class (kept only if the scene stays sparse and keeps something to see), two do in one call, a block
    changes within its class, or a block is appended."""
    for _ in range(8):
        r = rng.random()
        if r < 0.55:
            t = int(rng.choice(toggles))
            items = [(t, _random_block(rng, int(rng.integers(3))))]
        elif r < 0.7:
            items = [(int(t), _random_block(rng, int(rng.integers(3)))) for t in rng.permutation(toggles)[:2]]
        elif r < 0.85:
            t = int(rng.choice(toggles))
            items = [(t, _random_block(rng, int(ref.block_class(cur.blocks[t]))))]
        else:
            toggles.append(len(cur.blocks))
            return "a block appended", blocks((len(cur.blocks), _random_block(rng, int(rng.integers(3)))))
        after = apply_to_model(copy.deepcopy(cur), blocks(*items))
        if 0.035 <= visible_fill(after) <= 0.09:
            names = ", ".join(f"{t}: {ref.block_class(cur.blocks[t])} -> {ref.block_class(b)}" for t, b in items)
            return f"blocks replaced ({names})", blocks(*items)
    return "a compaction", COMPACT


def random_sequence(seed, n_steps=N_RANDOM_STEPS):
    """(space, steps): a sparse scene (visible fill between 3 % and 10 %, so open regions are large and their rims long) and `n_steps` calls drawn
    from the operations above; every tenth step and the last are compared with a fresh context and through frames."""
    rng = np.random.default_rng(seed)
    sp, ix = scene()
    toggles = [sp.add_block(flat.atom((0.0, 0.0, 0.0, 0.0), name="t")), sp.add_block(flat.atom((0.2, 0.6, 0.9, 0.3), name="t")), sp.add_block(shell_block(2, alpha=0.8))]
    n = int(np.prod(sp.size))
    cells = rng.permutation(n)
    grid = sp.block_index.reshape(-1)
    k = int(0.05 * n)
    grid[cells[:k]] = rng.choice([ix["visible"], ix["recursive"], ix["glow"], ix["ghost"]], k)
    grid[cells[k:k + 24]] = rng.choice([ix["unseen"], ix["tinted"], ix["hollow"]], 24)
    for j, t in enumerate(toggles):
        grid[cells[k + 24 + 5 * j:k + 29 + 5 * j]] = t
    cur = copy.deepcopy(sp)
    steps = []
    for k in range(n_steps):
        r = rng.random()
        if r < 0.6:
            what, op = _random_batch(rng, cur)
        elif r < 0.93:
            what, op = _random_replacement(rng, cur, toggles)
        else:
            what, op = "a compaction", COMPACT
        cur = apply_to_model(cur, op)
        marked = (k + 1) % 10 == 0 or k == n_steps - 1
        steps.append(Step(what, op, fresh=marked, view=(VIEW_Z, VIEW_X)[(k // 10) % 2] if marked else None))
    return sp, steps


# --- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def small_space(size, filled):
    sp, ix = scene(size)
    if filled:
        sp.block_index[tuple(s // 2 for s in size)] = ix["visible"]
    return sp


@pytest.mark.parametrize("filled", (False, True), ids=("air", "a visible block in the middle"))
@pytest.mark.parametrize("size", SMALL_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_upload(ctx, size, filled):
    sp = small_space(size, filled)
    n_open = int(ref.open_cubes(sp).sum())
    if size == (3, 3, 3):
        assert n_open == (0 if filled else 1)  # exactly one cube can be open
    if size == (3, 3, 40):
        assert n_open == (35 if filled else 38)
    if min(size) < 3:
        assert n_open == 0
    ctx.upload_space(WORLD, sp)
    grid = assert_grid(ctx, sp, f"upload of {size}")
    assert_fresh(sp, grid, f"upload of {size}")


def boundary_scene():
    """boundary_space of test_gpu_open_cubes.py, at LO and with the awkward blocks about."""
    sp, ix = scene()
    for at, name in ((VISIBLE_AT, "visible"), (RECURSIVE_AT, "recursive"), (INVISIBLE_AT, "unseen"), ((2, 2, 2), "tinted"), ((6, 4, 8), "glow"), ((3, 5, 4), "hollow"),
                     ((6, 2, 8), "ghost")):
        sp.set(world(at), ix[name])
    return sp


def test_upload_of_the_boundary_scene_and_over_a_larger_layer(ctx):
    """An upload over an existing larger layer leaves nothing behind: the n_cubes entries of the smaller grid are the restatement's, and again when
    the larger one comes back."""
    big = boundary_scene()
    m = ref.open_cubes(big)
    assert m[4, 3, 3] and not m[5, 3, 3] and not m[5, 4, 8] and m[2, 2, 2] and m[3, 5, 4] and not m[6, 2, 7] and not m[4, 0, 5]
    ctx.upload_space(WORLD, big)
    grid = assert_grid(ctx, big, "the boundary scene")
    assert_fresh(big, grid, "the boundary scene")
    for size in ((3, 3, 3), (2, 5, 5), (3, 3, 40)):
        for filled in (True, False):
            sp = small_space(size, filled)
            ctx.upload_space(WORLD, sp)
            assert_grid(ctx, sp, f"{size} over a larger layer")
        ctx.upload_space(WORLD, big)
        assert (assert_grid(ctx, big, f"the boundary scene over {size}") == grid).all()


def test_update_cubes_scripted(ctx):
    run(ctx, *scripted_updates())


def test_replace_blocks_scripted(ctx):
    run(ctx, *scripted_replacements())


def test_the_14_bit_limit(ctx):
    """16384 blocks: a tagged grid. One more, appended: the tags are dropped, updates write plain indices and a class change touches the class table
    alone. A small table uploaded: the tags are back."""
    sp, ix = scene()
    for at, name in ((VISIBLE_AT, "visible"), (RECURSIVE_AT, "recursive"), (INVISIBLE_AT, "unseen")):
        sp.set(world(at), ix[name])
    small = copy.deepcopy(sp)
    rng = np.random.default_rng(7)
    while len(sp.blocks) < ref.MAX_TAGGED_BLOCKS:
        c = rng.uniform(0.05, 0.95, 3)
        sp.add_block(flat.atom((float(c[0]), float(c[1]), float(c[2]), 1.0 if len(sp.blocks) % 3 else 0.0)))
    sp.set(world((3, 4, 2)), 9000)
    sp.set(world((5, 2, 6)), 16383)
    assert ref.is_tagged(sp) and ref.open_cubes(sp).any()
    ctx.upload_space(WORLD, sp)
    grid = assert_grid(ctx, sp, "16384 blocks")
    assert (grid >> ref.TAG_SHIFT).max() == ref.TAG_RECURSIVE and int((grid & ref.INDEX_MASK).max()) == 16383
    steps = [Step("index 16384 appended", blocks((16384, flat.atom((0.9, 0.1, 0.1, 1.0))))),
             Step("a batch of cubes", cubes([world(c) for c in ((5, 2, 7), (4, 3, 5), (0, 0, 0), (9, 0, 0), (4, 3, 6))], [16384, 9000, ix["visible"], 16384, ix["air"]])),
             Step("a class change", blocks((ix["air"], flat.atom((0.2, 0.6, 0.9, 0.02)))), unchanged=True),
             Step("... and back", blocks((ix["air"], flat.air())), unchanged=True),
             Step("a light-only batch", cubes([world((4, 3, 5))], None, [(200, 100, 50, 255)]), unchanged=True)]
    for k, s in enumerate(steps):
        apply_to_device(ctx, s.op)
        sp = apply_to_model(sp, s.op)
        assert not ref.is_tagged(sp)
        got = assert_grid(ctx, sp, s.what)  # (the grid: plain indices; the class table: the change)
        assert (got == sp.block_index).all(), s.what
        if s.unchanged:
            assert (got == grid).all(), s.what
        grid = got
    assert int(grid.max()) == 16384 and grid[5, 2, 7] == 16384 and grid[4, 3, 5] == 9000
    assert_fresh(sp, grid, "past the limit")
    ctx.upload_space(WORLD, small)
    grid = assert_grid(ctx, small, "a small table again")
    assert ref.is_tagged(small) and (grid >> ref.TAG_SHIFT == ref.TAG_OPEN).any()


@pytest.mark.parametrize("seed", seeds())
def test_random_sequence(seed):
    with abi.Context(0) as c:
        run(c, *random_sequence(seed))


def test_rejections(ctx):
    import torch

    sp = boundary_scene()
    ctx.upload_space(WORLD, sp)
    ctx.set_options(WORLD, abi.make_options())
    inv = camera(SIZE, point(VIEW_Z[0]), point(VIEW_Z[1]), fov=VIEW_Z[2], view_distance=VD)
    frame = ctx.make_frame(SIZE[0], SIZE[1], world_inv=inv)
    want = ctx.render(frame)["rgba8"].copy()
    lib, h = ctx._lib, ctx._h
    grid = np.full(sp.size, 0xABCD, np.uint16)
    ctx.clear_space(abi.LAYER_UI)
    for what, call in (("a NULL grid", lambda: lib.aic_probe_cube_grid(h, WORLD, None, None, None)),
                       ("a bad layer", lambda: lib.aic_probe_cube_grid(h, 7, grid.ctypes.data, None, None)),
                       ("a negative layer", lambda: lib.aic_probe_cube_grid(h, -1, grid.ctypes.data, None, None)),
                       ("a cleared layer", lambda: lib.aic_probe_cube_grid(h, abi.LAYER_UI, grid.ctypes.data, None, None))):
        with pytest.raises(abi.AicError) as err:
            ctx._check(call())
        assert err.value.code == AIC_ERR_INVALID and "aic_probe_cube_grid" in str(err.value), what
        assert (grid == 0xABCD).all(), what
        assert (ctx.render(frame)["rgba8"] == want).all(), what
    # the optional outputs may be left out
    ctx._check(lib.aic_probe_cube_grid(h, WORLD, grid.ctypes.data, None, None))
    assert (grid == ref.tagged_grid(sp)).all()
    # a probe while a frame is submitted on a slot returns after that frame, which comes back intact
    buf = torch.zeros((SIZE[1], SIZE[0], 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_submit(frame, buf.data_ptr(), 1)
    assert_grid(ctx, sp, "a frame in flight")
    ctx.render_wait(1)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == want).all()
