"""Open cubes and the bonus step (run with -m gpu on an MI355X).

A tagged cube grid marks as OPEN every invisible cube inside the grid's outermost layer whose six face neighbours are invisible too
(csrc/aic_device.h), and a fast step of the plain and the exchanging production kernels that looks such a cube up takes the following
step without a lookup: wherever it lands, the cube is in bounds and invisible. What that may not change is anything a ray computes. So
every frame here is compared with the CPU oracle three times over: the recording variant, which never skips a lookup (RGBA8 bytes,
every pixel's step count, the first-hit records and the lookup totals), and both production variants (RGBA8 bytes, the frame's step
total, and every pixel's step count read from a second frame with debug_pixel_cost, whose linear green is 0.002 n: accum.rs:228-234).
Frames are at most 64 x 48.

The cases are the places where a stale or misplaced OPEN tag, or a bonus step too many, would show: the rim of an open region around
a visible atom, a recursive block and an invisible atom that is not air, met along every axis and along a diagonal; the grid's own
outermost layer, from inside and from outside; cubes changed in the middle of an open region (aic_update_cubes) and a block that
changes class under the cubes that hold it (aic_replace_blocks); the 1000-step cap; and a grid that carries no tags at all."""
import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi, flat
from tests.test_gpu_first_lookup import camera, shell_block
from tests.test_gpu_linear_parity import assert_rgba8_exact
from tests.test_gpu_parity import assert_parity, to_abi_options

pytestmark = pytest.mark.gpu

VARIANTS = (("plain", abi.VARIANT_PLAIN), ("exchanging", abi.VARIANT_EXCHANGING))
SIZE = (64, 48)
VD = 40.0
GRID = (9, 7, 11)
VISIBLE_AT, RECURSIVE_AT, INVISIBLE_AT = (6, 3, 3), (2, 3, 7), (4, 2, 5)


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def options(transparency, view_distance=VD, cost=False):
    return oracle.make_options(fog=0, transparency=transparency, lighting=1, view_distance=view_distance, debug_pixel_cost=cost)


def air_grid(size=GRID):
    """A grid of air and the blocks the cases place in it: (space, air, visible atom, recursive R4 block, invisible atom that is not air)."""
    sp = flat.FlatSpace((0, 0, 0), size)
    sp.set_sky_uniform((0.7, 0.8, 1.0))
    a = sp.add_block(flat.air())
    visible = sp.add_block(flat.atom((0.9, 0.3, 0.2, 0.6)))
    recursive = sp.add_block(shell_block(4, alpha=0.5))
    unseen = sp.add_block(flat.atom((0.0, 0.0, 0.0, 0.0), name="unseen"))
    sp.block_index[...] = a
    sp.light[..., 0:3] = 180
    sp.light[..., 3] = flat.STATUS_VISIBLE
    return sp, a, visible, recursive, unseen


def open_mask(sp):
    """The definition, restated: which cubes of `sp` are open (every block of these scenes that is not invisible is visible or recursive)."""
    inv = np.array([b.is_one and float(b.palette[0][3]) == 0.0 and not b.palette[0][4:7].any() for b in sp.blocks])[sp.block_index]
    m = np.zeros(sp.block_index.shape, bool)
    core = inv[1:-1, 1:-1, 1:-1].copy()
    for axis in range(3):
        for shift in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[axis] = slice(shift, inv.shape[axis] - 2 + shift)
            core &= inv[tuple(sl)]
    m[1:-1, 1:-1, 1:-1] = core
    return m


def check(ctx, sp, size, inv, what, view_distance=VD, upload=True):
    """The frame under Surface and Volumetric transparency: recording, plain and exchanging variants against the oracle (module docstring).
    `upload` False: the scene is on the device already, by whatever route the case took. Returns the oracle's per-pixel step counts."""
    w, h = size
    osp, cam = oracle.Space(sp), oracle.make_camera(inv, w, h)
    if upload:
        ctx.upload_space(abi.LAYER_WORLD, sp)
    ctx.clear_space(abi.LAYER_UI)
    counts = None
    for transparency in (0, 1):
        opt = options(transparency, view_distance)
        ref = oracle.render(osp, opt, cam, want_aux=True)
        counts = ref["aux"]["cubes_traced"]
        ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
        rec = ctx.render(ctx.make_frame(w, h, world_inv=inv), want_aux=True)
        assert rec["info"].variant == abi.VARIANT_RECORDING
        assert_parity(rec, ref, tol=0)
        for name, variant in VARIANTS:
            tag = f"{what}, transparency {transparency}, {name} variant"
            img = ctx.render(ctx.make_frame(w, h, world_inv=inv, tuning=abi.tuning(variant=variant)))
            assert img["info"].variant == variant, tag
            assert img["info"].cubes_traced == int(ref["info"]["cubes_traced"]), (tag, img["info"].cubes_traced, int(ref["info"]["cubes_traced"]))
            assert_rgba8_exact(img["rgba8"], ref["rgba8"], tag)
        ctx.set_options(abi.LAYER_WORLD, to_abi_options(options(transparency, view_distance, cost=True)))
        for name, variant in VARIANTS:
            cost = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_LINEAR, tuning=abi.tuning(variant=variant)))
            got = np.rint(cost["rgba8"][..., 1].astype(np.float64) / float(np.float32(0.002))).astype(np.int64)
            bad = np.argwhere(got != counts)
            assert not len(bad), (what, transparency, name, len(bad), tuple(bad[0]), int(got[tuple(bad[0])]), int(counts[tuple(bad[0])]))
    return counts


# --- the boundaries of open regions -------------------------------------------------------------------------------------------------
def boundary_space():
    sp, _, visible, recursive, unseen = air_grid()
    sp.set(VISIBLE_AT, visible)
    sp.set(RECURSIVE_AT, recursive)
    sp.set(INVISIBLE_AT, unseen)
    return sp


# eye, target, field of view: rays reach each placed block two cubes after an open cube (the cube next to a visible or recursive one is never
# open: the bonus step lands on it), along +-x, +-y, +-z and along diagonals whose steps alternate between two axes; every ray that misses ends by
# leaving the grid through an open cube and then a cube of the outermost layer
VIEWS = {
    "+x at the visible atom": ((1.5, 3.4, 3.6), (6.5, 3.5, 3.5), 60.0),
    "-x at the recursive block": ((7.5, 3.6, 7.4), (2.5, 3.5, 7.5), 60.0),
    "-y through the invisible atom": ((4.5, 5.6, 5.4), (4.5, 0.0, 5.55), 50.0),
    "+y at the visible atom": ((6.4, 1.4, 3.6), (6.5, 6.0, 3.45), 70.0),
    "-z at the recursive block": ((2.6, 3.4, 9.6), (2.5, 3.5, 7.5), 60.0),
    "+z at the visible atom and out": ((6.4, 3.6, 1.5), (6.5, 3.5, 9.0), 80.0),
    "xz diagonal at the visible atom": ((3.3, 3.5, 6.6), (6.5, 3.5, 3.5), 60.0),
    "xyz diagonal through the invisible atom": ((1.4, 5.3, 8.6), (7.5, 1.0, 1.5), 60.0),
    "from outside": ((4.5, 3.5, 16.0), (4.4, 3.4, 0.0), 50.0),
    "from outside, askew": ((14.0, 9.0, 15.0), (3.0, 3.0, 5.0), 40.0),
}


@pytest.mark.parametrize("view", list(VIEWS))
def test_boundaries_of_open_regions(ctx, view):
    sp = boundary_space()
    m = open_mask(sp)
    assert m[4, 3, 3] and not m[5, 3, 3] and m[4, 3, 7] and not m[3, 3, 7]  # two cubes from the visible / recursive block: open; next to it: not
    assert m[4, 3, 5] and m[4, 1, 5] and not m[4, 0, 5]  # beside the invisible atom: open all the same; the outermost layer never is
    assert m[INVISIBLE_AT]  # (an invisible atom is as good as air)
    eye, target, fov = VIEWS[view]
    counts = check(ctx, sp, SIZE, camera(SIZE, eye, target, fov=fov, view_distance=VD), view)
    assert counts.max() >= 8  # rays long enough to have met open cubes


# --- updates ---------------------------------------------------------------------------------------------------------------------
def test_updates_keep_the_open_tags_true(ctx):
    """A visible block placed into the middle of an open region and taken out again (aic_update_cubes), then air itself turned visible
    (aic_replace_blocks): after each step the frame of the updated scene is the oracle's, and so is that of a fresh upload of it."""
    sp, a, visible, recursive, _ = air_grid()
    sp.set(RECURSIVE_AT, recursive)
    eye, target = (4.5, 3.5, 9.6), (4.45, 3.45, 0.0)
    inv = camera(SIZE, eye, target, fov=60.0, view_distance=VD)
    spot = (4, 3, 5)
    assert open_mask(sp)[spot] and all(open_mask(sp)[c] for c in ((3, 3, 5), (5, 3, 5), (4, 2, 5), (4, 4, 5), (4, 3, 4), (4, 3, 6)))
    check(ctx, sp, SIZE, inv, "before any update")

    def both(what):
        check(ctx, sp, SIZE, inv, what + ", updated in place", upload=False)
        snapshot = abi.Context(0)
        try:
            check(snapshot, sp, SIZE, inv, what + ", fresh upload")
        finally:
            snapshot.close()

    # a set OPEN tag left on the six neighbours would carry rays through the new block
    ctx.update_cubes(abi.LAYER_WORLD, np.array([spot], np.int32), np.array([visible], np.uint16))
    sp.set(spot, visible)
    assert not open_mask(sp)[4, 3, 6]
    both("a visible block in an open region")
    # ... and out again, with a cube of the outermost layer and one outside the space in the same batch
    ctx.update_cubes(abi.LAYER_WORLD, np.array([spot, (0, 3, 5), (-1, 3, 5), (8, 6, 10)], np.int32), np.array([a, visible, visible, visible], np.uint16))
    sp.set(spot, a)
    sp.set((0, 3, 5), visible)
    sp.set((8, 6, 10), visible)
    assert open_mask(sp)[spot] and not open_mask(sp)[1, 3, 5]
    both("the block removed, two rim cubes filled")
    # air becomes a translucent visible block: every cube that held it changes class under its tag
    glass = flat.atom((0.2, 0.6, 0.9, 0.02))
    ctx.replace_blocks(abi.LAYER_WORLD, [(a, glass)])
    sp.blocks[a] = glass
    assert not open_mask(sp).any()
    both("air replaced by a visible block")
    # ... and back: the open regions return
    ctx.replace_blocks(abi.LAYER_WORLD, [(a, flat.air())])
    sp.blocks[a] = flat.air()
    assert open_mask(sp)[spot]
    both("the visible block replaced by air")


# --- the step cap ------------------------------------------------------------------------------------------------------------------
def test_a_bonus_step_stops_at_the_step_cap(ctx):
    """A 3 x 3 x 1100 corridor of air seen end to end: its middle column is open from end to end, and the rays that stay in it are cut
    at the cap (count_step_should_stop, sr.rs:639-651) -- at the oracle's count, wherever in a fast step's pair of steps the cap falls."""
    sp, *_ = air_grid((3, 3, 1100))
    m = open_mask(sp)
    assert m[1, 1, 1:1099].all() and m.sum() == 1098
    size = (48, 32)
    for z0 in (1099.5, 1098.2, 1097.7):  # (the cap falls on the first or the second step of a pair, depending on where the ray starts)
        inv = camera(size, (1.5, 1.5, z0), (1.5, 1.5, 0.0), fov=0.6, view_distance=3000.0)
        counts = check(ctx, sp, size, inv, f"corridor from z = {z0}", view_distance=3000.0)
        assert counts.max() >= 1000 and (counts == counts.max()).sum() > 64  # whole waves of rays run into the cap
    inv = camera(size, (1.5, 1.5, 1099.5), (1.5, 1.5, 0.0), fov=2.0, view_distance=3000.0)
    counts = check(ctx, sp, size, inv, "corridor, wide", view_distance=3000.0)
    assert counts.max() >= 1000 and counts.min() < 100  # rays that leave through the walls early beside rays that are cut


# --- an untagged grid ------------------------------------------------------------------------------------------------------------------
def test_a_layer_past_16384_blocks_renders_as_before(ctx):
    sp = boundary_space()
    rng = np.random.default_rng(7)
    while len(sp.blocks) < 16385:  # one past the 14-bit limit: plain indices in the grid, no tags, no open cubes
        c = rng.uniform(0.05, 0.95, 3)
        sp.add_block(flat.atom((float(c[0]), float(c[1]), float(c[2]), 1.0)))
    sp.set((5, 2, 6), 16384)
    sp.set((3, 4, 2), 9000)
    eye, target, fov = VIEWS["from outside, askew"]
    check(ctx, sp, SIZE, camera(SIZE, eye, target, fov=fov, view_distance=VD), "untagged grid, from outside")
    eye, target, fov = VIEWS["xyz diagonal through the invisible atom"]
    check(ctx, sp, SIZE, camera(SIZE, eye, target, fov=fov, view_distance=VD), "untagged grid, from inside")
