"""aic_replace_cube_grid, aic_copy_cube_grid and aic_update_light_volume_device on the device (run with -m gpu on an MI355X). DESIGN.md 4.23.

The device arrays are torch tensors. After every replace the whole grid and the class table read back by aic_probe_cube_grid must equal
tests/cube_tags_ref.py's restatement of the model, and the boxes and the info tests/grid_replace_ref.py's, entry for entry. The shapes are chosen for
the kernel's seams: a workgroup owns 2048 entries, a lane 8, and the last partial group of 8 is handled entry by entry."""

import numpy as np
import pytest
import torch

import oracle
from all_is_cubes_amd import abi, flat
from tests import cube_tags_ref, stale_scenes as S
from tests import grid_replace_ref as ref
from tests import test_gpu_pick as pk
from tests import test_gpu_reproject as rp
from tests import test_gpu_stale as gs
from tests.test_gpu_cube_tags import LO, assert_fresh, assert_grid, scene
from tests.test_gpu_first_lookup import camera
from tests.test_gpu_parity import to_abi_options

pytestmark = pytest.mark.gpu

WORLD = abi.LAYER_WORLD
AIC_ERR_INVALID = 1
SHAPES = ((1, 1, 1), (3, 3, 3), (2, 5, 5), (3, 3, 40), (2, 3, 1027), (17, 16, 16))
INFO_KEYS = ("n_cubes", "n_runs", "bounds", "n_written", "merged")


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def on_device(index):
    """uint16 indices as a tensor on the device (int16: the bits as they are), complete before it is handed over"""
    t = torch.from_numpy(np.array(index, np.uint16).reshape(-1).view(np.int16)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def light_on_device(light):
    t = torch.from_numpy(np.array(light, np.uint8).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def replace_and_check(ctx, sp, new, what, capacity=None, light=None):
    """One call on the device and on the model `sp` (in place); the report and the grid must be the restatements'."""
    capacity = sp.block_index.size + 1 if capacity is None else capacity
    boxes, info = ctx.replace_cube_grid(WORLD, on_device(new), None if light is None else light_on_device(light), capacity=capacity)
    want_boxes, want_info = ref.replace(sp, new, capacity, light)
    assert {k: info[k] for k in INFO_KEYS} == want_info, what
    assert boxes.dtype == np.int32 and boxes.shape == want_boxes.shape and (boxes == want_boxes).all(), what
    return assert_grid(ctx, sp, what)


def changes(sp, ix, rng):
    """(what, new index array) for every kind of change, each made from the grid the one before leaves."""
    size = sp.size
    n = int(np.prod(size))
    kinds = np.array([ix["air"]] * 6 + [ix["visible"], ix["recursive"], ix["unseen"], ix["tinted"], ix["glow"], ix["hollow"], ix["ghost"]], np.uint16)
    cur = sp.block_index.copy()
    mid = tuple(s // 2 for s in size)

    def step(what, new):
        nonlocal cur
        cur = np.asarray(new, np.uint16).copy()
        return what, cur.copy()

    new = cur.copy(); new[mid] = ix["visible"]
    yield step("one cube: a visible block into an open region", new)
    new = cur.copy(); new[mid] = ix["air"]
    yield step("... and out again", new)
    new = cur.copy(); new[size[0] - 1, size[1] // 2, :] = ix["recursive"]
    yield step("a whole row", new)
    yield step("everything", (cur + 1) % len(sp.blocks))
    yield step("nothing", cur)
    new = cur.copy(); new[-1, -1, -1] = (int(new[-1, -1, -1]) + 1) % 4
    yield step("the last entry alone", new)
    new = cur.copy(); new[0, 0, 0] = (int(new[0, 0, 0]) + 1) % 4
    yield step("the first entry alone", new)
    new = cur.copy(); new[0, :, :] = ix["unseen"]; new[:, 0, :] = ix["glow"]
    yield step("the outermost layer", new)
    yield step("all air", np.full(size, ix["air"], np.uint16))
    for share in (0.01, 0.5, 0.99):
        pick = rng.random(size) < share
        if not pick.any():
            pick.reshape(-1)[int(rng.integers(n))] = True
        new = cur.copy()
        new[pick] = rng.choice(kinds, int(pick.sum()))
        yield step(f"random, {share:.0%} of the cubes drawn", new)


# --- 1. whole grids, exactly --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_whole_grids(ctx, size):
    sp, ix = scene(size)
    ctx.upload_space(WORLD, sp)
    rng = np.random.default_rng(sum(size))
    for k, (what, new) in enumerate(changes(sp, ix, rng)):
        replace_and_check(ctx, sp, new, f"{size}: {what}")
        if what in ("everything", "the outermost layer") or k == 11:
            assert_fresh(sp, ctx.probe_cube_grid(WORLD, sp.size, len(sp.blocks))[0], what)


@pytest.mark.parametrize("size", ((3, 3, 40), (2, 3, 1027)), ids=lambda s: "x".join(map(str, s)))
def test_the_capacity_table(ctx, size):
    sp, ix = scene(size)
    ctx.upload_space(WORLD, sp)
    rng = np.random.default_rng(5)
    for capacity in (0, 1, 7, None):
        new = sp.block_index.copy()
        pick = rng.random(size) < 0.3
        new[pick] = (new[pick] + 1) % 4
        n_runs = ref.report(sp.lo, sp.block_index, new, 1 << 30)[1]["n_runs"]
        assert n_runs > 7
        for cap in ([capacity] if capacity is not None else [n_runs - 1, n_runs]):
            replace_and_check(ctx, sp, new, f"{size}: capacity {cap} of {n_runs} runs", capacity=cap)
            new = new.copy()
            new[pick] = (new[pick] + 1) % 4


@pytest.mark.parametrize("seed", (7100, 7101))
def test_sequences_of_replaces(seed):
    rng = np.random.default_rng(seed)
    size = (5, 4, 419)  # 8380 entries: five workgroups, rows that straddle their seams, a last group of 4
    sp, ix = scene(size)
    kinds = np.array([ix["air"]] * 10 + [ix["visible"], ix["recursive"], ix["unseen"], ix["ghost"]], np.uint16)
    with abi.Context(0) as c:
        c.upload_space(WORLD, sp)
        for k in range(20):
            new = sp.block_index.copy()
            pick = rng.random(size) < rng.choice([0.002, 0.05, 0.6])
            new[pick] = rng.choice(kinds, int(pick.sum()))
            grid = replace_and_check(c, sp, new, f"seed {seed} step {k + 1}", capacity=int(rng.choice([0, 3, 100000])))
            if (k + 1) % 5 == 0:
                assert_fresh(sp, grid, f"seed {seed} step {k + 1}")


# --- 2. the pool beyond the grid ----------------------------------------------------------------------------------------------------------
def frame_of(c, sp, size=(64, 48)):
    eye = tuple(float(l) + v for l, v in zip(sp.lo, (4.5, 3.5, 9.0)))
    target = tuple(float(l) + v for l, v in zip(sp.lo, (1.0, 2.5, 2.0)))
    c.set_options(WORLD, abi.make_options())
    c.clear_space(abi.LAYER_UI)
    got = c.render(c.make_frame(size[0], size[1], world_inv=camera(size, eye, target, fov=80.0, view_distance=40.0)))
    return got["rgba8"].copy(), int(got["info"].cubes_traced)


def test_the_pool_behind_the_grid_stays(ctx):
    size = (2, 5, 5)  # 50 entries: the last lane's group of 8 has two; the recursive block's voxels start at entry 50
    sp, ix = scene(size)
    assert sp.block_index.size % 8 == 2 and cube_tags_ref.block_class(sp.blocks[ix["recursive"]]) == 2
    sp.block_index[1, 2, 2] = ix["recursive"]
    ctx.upload_space(WORLD, sp)
    new = sp.block_index.copy()
    new[-1, -1, -1] = ix["recursive"]
    new[0, 0, 0] = ix["visible"]
    new[1, 4, 3] = ix["ghost"]
    replace_and_check(ctx, sp, new, "recursive blocks at the grid's end")
    got = frame_of(ctx, sp)
    with abi.Context(0) as fresh:
        fresh.upload_space(WORLD, sp)
        want = frame_of(fresh, sp)
    assert got[1] == want[1] and (got[0] == want[0]).all()
    assert len(np.unique(want[0].reshape(-1, 4), axis=0)) > 3, "the blocks show"


# --- 3. untagged grids --------------------------------------------------------------------------------------------------------------------
def test_untagged_grids(ctx):
    sp, ix = scene((2, 3, 5))
    rng = np.random.default_rng(9)
    while len(sp.blocks) < cube_tags_ref.MAX_TAGGED_BLOCKS + 1:
        c = rng.uniform(0.05, 0.95, 3)
        sp.add_block(flat.atom((float(c[0]), float(c[1]), float(c[2]), 1.0)))
    assert len(sp.blocks) == 16385 and not cube_tags_ref.is_tagged(sp)
    ctx.upload_space(WORLD, sp)
    new = sp.block_index.copy()
    assert ix["air"] == 0
    new[0, 0, 0] = 16384  # differs from the air it replaces, index 0, only above bit 13: a masked comparison would miss it
    new[1, 2, 4] = 16383
    grid = replace_and_check(ctx, sp, new, "plain indices")
    assert (grid == new).all()
    new = new.copy()
    new[0, 0, 0] = 0
    boxes, info = ctx.replace_cube_grid(WORLD, on_device(new))
    assert info["n_cubes"] == 1 and boxes.tolist() == [[LO[0], LO[1], LO[2], LO[0] + 1, LO[1] + 1, LO[2] + 1]]
    sp.block_index[...] = new
    assert (assert_grid(ctx, sp, "a change above bit 13") == new).all()
    bad = new.copy()
    bad[0, 1, 0] = 16385
    with pytest.raises(abi.AicError):
        ctx.replace_cube_grid(WORLD, on_device(bad))
    assert_grid(ctx, sp, "after the refusal")


# --- 4. rejection -------------------------------------------------------------------------------------------------------------------------
def test_rejections(ctx):
    size = (3, 4, 400)  # 4800 entries: three workgroups
    sp, ix = scene(size)
    sp.block_index[1, 2, 200] = ix["visible"]
    sp.block_index[1, 1, 199] = ix["recursive"]
    sp.block_index[1, 2, 3] = ix["visible"]  # (in front of frame_of's camera)
    sp.block_index[0, 1, 2] = ix["recursive"]
    ctx.upload_space(WORLD, sp)
    before = assert_grid(ctx, sp, "the upload")
    light_before = ctx.read_light_volume(WORLD, sp.size)
    frame_before = frame_of(ctx, sp)
    n = sp.block_index.size
    n_blocks = len(sp.blocks)

    def unchanged(what):
        assert (ctx.probe_cube_grid(WORLD, sp.size, n_blocks)[0] == before).all(), what
        assert (ctx.read_light_volume(WORLD, sp.size) == light_before).all(), what
        got = frame_of(ctx, sp)
        assert got[1] == frame_before[1] and (got[0] == frame_before[0]).all(), what

    for at in (0, n - 1, 2048 + 1000, 2047, 2048):
        bad = sp.block_index.copy()
        bad[...] = ix["visible"]  # everything else changes too: nothing of it may land
        bad.reshape(-1)[at] = n_blocks
        with pytest.raises(abi.AicError) as err:
            ctx.replace_cube_grid(WORLD, on_device(bad), light_on_device(np.full((n, 4), 7, np.uint8)))
        assert err.value.code == AIC_ERR_INVALID and "aic_replace_cube_grid" in str(err.value), at
        unchanged(f"an index of n_blocks at entry {at}")
        bad.reshape(-1)[at] = 0xFFFF
        with pytest.raises(abi.AicError):
            ctx.replace_cube_grid(WORLD, on_device(bad))
        unchanged(f"an index of 65535 at entry {at}")
    lib, h = ctx._lib, ctx._h
    good = on_device(sp.block_index)
    wide = torch.zeros(n + 8, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    info = abi.BlockCubesInfo()
    out = np.zeros((4, 6), np.int32)
    import ctypes as C
    ip, op = C.byref(info), C.c_void_p(out.ctypes.data)
    ctx.clear_space(abi.LAYER_UI)
    for what, call in (("a misaligned array", lambda: lib.aic_replace_cube_grid(h, WORLD, C.c_void_p(wide.data_ptr() + 2), None, 4, op, ip)),
                       ("a NULL array", lambda: lib.aic_replace_cube_grid(h, WORLD, None, None, 4, op, ip)),
                       ("a NULL info", lambda: lib.aic_replace_cube_grid(h, WORLD, C.c_void_p(good.data_ptr()), None, 4, op, None)),
                       ("NULL boxes with a capacity", lambda: lib.aic_replace_cube_grid(h, WORLD, C.c_void_p(good.data_ptr()), None, 4, None, ip)),
                       ("a bad layer", lambda: lib.aic_replace_cube_grid(h, 5, C.c_void_p(good.data_ptr()), None, 4, op, ip)),
                       ("a layer without a space", lambda: lib.aic_replace_cube_grid(h, abi.LAYER_UI, C.c_void_p(good.data_ptr()), None, 4, op, ip)),
                       ("an array in host memory", lambda: lib.aic_replace_cube_grid(h, WORLD, C.c_void_p(np.zeros(n + 8, np.uint16).ctypes.data & ~15), None, 4, op, ip)),
                       ("copy: a misaligned array", lambda: lib.aic_copy_cube_grid(h, WORLD, C.c_void_p(wide.data_ptr() + 2), None)),
                       ("copy: a layer without a space", lambda: lib.aic_copy_cube_grid(h, abi.LAYER_UI, C.c_void_p(wide.data_ptr()), None)),
                       ("light: a NULL array", lambda: lib.aic_update_light_volume_device(h, WORLD, None)),
                       ("light: a layer without a space", lambda: lib.aic_update_light_volume_device(h, abi.LAYER_UI, C.c_void_p(wide.data_ptr())))):
        assert call() == AIC_ERR_INVALID, what
        unchanged(what)
    # the binding's own checks, on device tensors
    with pytest.raises(ValueError):
        ctx.replace_cube_grid(WORLD, wide)
    with pytest.raises(ValueError):
        ctx.replace_cube_grid(WORLD, good.to(torch.int32))
    with pytest.raises(ValueError):
        ctx.replace_cube_grid(WORLD, good.cpu())
    # ... and the next valid call succeeds
    new = sp.block_index.copy()
    new[2, 3, 399] = ix["glow"]
    replace_and_check(ctx, sp, new, "a valid call after the refusals")
    # an empty grid: AIC_OK and a zero info, whatever the array
    empty, _ = scene((0, 3, 3))
    ctx.upload_space(WORLD, empty)
    boxes, info = ctx.replace_cube_grid(WORLD, None)
    assert boxes.shape == (0, 6) and {k: info[k] for k in INFO_KEYS} == ref.ZERO_INFO


# --- 5. round trip ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ((2, 3, 1027), (9, 7, 11)), ids=lambda s: "x".join(map(str, s)))
def test_round_trip(ctx, size):
    sp, ix = scene(size)
    rng = np.random.default_rng(21)
    pick = rng.random(size) < 0.2
    sp.block_index[pick] = rng.choice([ix["visible"], ix["recursive"], ix["unseen"], ix["ghost"]], int(pick.sum()))
    sp.light[...] = rng.integers(0, 255, sp.light.shape)
    ctx.upload_space(WORLD, sp)
    before = assert_grid(ctx, sp, "the upload")
    n = sp.block_index.size
    index = torch.full((n,), -1, dtype=torch.int16, device="cuda:0")
    light = torch.full((4 * n,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.copy_cube_grid(WORLD, index, light)
    assert (index.cpu().numpy().view(np.uint16).reshape(size) == sp.block_index).all()
    assert (light.cpu().numpy().reshape(size + (4,)) == ctx.read_light_volume(WORLD, sp.size)).all() and (light.cpu().numpy().reshape(sp.light.shape) == sp.light).all()
    only = torch.full((n,), -1, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    ctx.copy_cube_grid(WORLD, only)
    assert (only == index).all()
    boxes, info = ctx.replace_cube_grid(WORLD, index, light)
    assert boxes.shape == (0, 6) and {k: info[k] for k in INFO_KEYS} == ref.ZERO_INFO
    assert (assert_grid(ctx, sp, "replaced with its own copy") == before).all()
    assert (ctx.read_light_volume(WORLD, sp.size) == sp.light).all()


# --- 6. light -----------------------------------------------------------------------------------------------------------------------------
def lamp_scene():
    """plaza of tests/stale_scenes.py, lit, with a lamp in its block table: (space A, [(cube, block index)])"""
    a, edits, _, _ = S.case("plaza")
    sp = flat.FlatSpace(a.lo, a.size, blocks=list(a.blocks), sky_kind=a.sky_kind, sky=a.sky.copy(), block_index=a.block_index.copy(), light=a.light.copy())
    lamp = sp.add_block(flat.atom((1.0, 1.0, 1.0, 1.0), (4.0, 3.0, 1.0), name="lamp"))
    return sp, list(edits) + [((5, 2, 2), lamp)]


def test_the_light_updater_sees_the_new_grid():
    sp, edits = lamp_scene()
    cubes = np.array([cube for cube, _ in edits], np.int32)
    new = sp.block_index.copy()
    for cube, index in edits:
        new[cube] = index
    results = []
    for route in ("replace", "update_cubes"):
        with abi.Context(0) as c:
            c.upload_space(WORLD, sp)
            # (an update first: the updater's host mirrors are current before the change, and the replace must make them stale)
            first = c.evaluate_light(WORLD, 8, fast=False, queue=[], queue_order=0)
            if route == "replace":
                boxes, info = c.replace_cube_grid(WORLD, on_device(new))
                assert info["n_cubes"] == len(edits)
                changed = np.concatenate([np.stack(np.meshgrid(*[np.arange(b[a], b[a + 3]) for a in range(3)], indexing="ij"), -1).reshape(-1, 3) for b in boxes])
                assert sorted(map(tuple, changed.tolist())) == sorted(map(tuple, cubes.tolist()))
                assert c.light_changed(WORLD, take=False)[0] == 0
            else:
                c.update_cubes(WORLD, cubes, [index for _, index in edits])
            c.light_cubes_changed(WORLD, cubes, 0)
            got = c.evaluate_light(WORLD, 8, fast=False, queue=[], queue_order=0)
            results.append((int(first.updates), int(got.updates), c.read_light_volume(WORLD, sp.size), c.light_changed(WORLD)[0]))
    a, b = results
    assert a[0] == b[0] and a[1] == b[1] and a[1] > 0
    assert (a[2] == b[2]).all() and (a[2] != np.asarray(sp.light)).any()
    assert (a[3] == b[3]).all() and len(a[3]) > 0


def test_light_volume_from_device_memory(ctx):
    sp, _ = lamp_scene()
    rng = np.random.default_rng(4)
    light = rng.integers(0, 255, sp.light.shape).astype(np.uint8)
    light[..., 3] = flat.STATUS_VISIBLE
    frames = []
    for route in ("host", "device"):
        ctx.upload_space(WORLD, sp)
        if route == "host":
            ctx.update_light_volume(WORLD, light)
        else:
            ctx.update_light_volume_device(WORLD, light_on_device(light))
        assert (ctx.read_light_volume(WORLD, sp.size) == light).all(), route
        assert ctx.light_changed(WORLD, take=False)[0] == 0, route
        ctx.set_options(WORLD, to_abi_options(S.options(0)))
        ctx.clear_space(abi.LAYER_UI)
        frames.append(ctx.render(ctx.make_frame(64, 48, world_inv=S.camera("plaza")[0]))["rgba8"].copy())
    assert (frames[0] == frames[1]).all() and len(np.unique(frames[0].reshape(-1, 4), axis=0)) > 8
    # the light of a replace: the caller's own texels, never reported
    ctx.upload_space(WORLD, sp)
    ctx.replace_cube_grid(WORLD, on_device(sp.block_index), light_on_device(light))
    assert (ctx.read_light_volume(WORLD, sp.size) == light).all() and ctx.light_changed(WORLD, take=False)[0] == 0


# --- 7. the interactive loop --------------------------------------------------------------------------------------------------------------
W, HT = 64, 48


def loop_camera(name):
    from all_is_cubes_amd import _host as H

    _, _, eye, target = S.case(name)
    projection, world_to_eye, inv = oracle.camera_matrices(90.0, S.VIEW_DISTANCE, W / HT, oracle.look_at_y_up(eye, target), eye)
    o = H.GraphicsOptions()
    o.view_distance = S.VIEW_DISTANCE
    return inv, (world_to_eye @ projection).reshape(16).copy(), tuple(H.Camera(o, H.Viewport.with_scale(1.0, W, HT)).depth_transform_zw())


def split_frame(c, name, antialiasing):
    inv, vp, zw = loop_camera(name)
    c.set_options(WORLD, to_abi_options(S.options(antialiasing)))
    c.clear_space(abi.LAYER_UI)
    c.set_depth_transform(zw)
    return c.make_frame(W, HT, world_inv=inv, flags=abi.FRAME_OUT_SPLIT), vp


@pytest.mark.parametrize("antialiasing", S.ANTIALIASING)
@pytest.mark.parametrize("name", S.CASES)
def test_the_interactive_loop(name, antialiasing):
    count = W * HT
    a, edits, _, _ = S.case(name)
    b = S.edited(name)
    with abi.Context(0) as c, abi.Context(0) as fresh:
        c.upload_space(WORLD, a)
        f, vp = split_frame(c, name, antialiasing)
        resident = rp.device_bytes(count * 12)
        c.render_submit(f, resident.data_ptr(), 0)
        c.render_wait(0)
        c.synchronize()
        before = resident.cpu().numpy().copy()
        boxes, info = c.replace_cube_grid(WORLD, on_device(b.block_index))
        assert info["n_cubes"] == len(edits) and sorted(map(tuple, boxes.tolist())) == sorted(map(tuple, S.boxes(name).tolist()))
        order = gs.picker_order(W, HT)
        picks = pk.out_words(count)
        got = c.pick_stale_cubes(vp, W, HT, count, boxes, None, resident.data_ptr(), pk.to_device_words(order).data_ptr(), picks.data_ptr(), max_stale=count)
        assert 0 < got.n_stale < count and got.n_from_stale == got.n_stale
        tinfo = c.trace_pixels_device(f, int(got.n_stale), picks.data_ptr(), resident.data_ptr(), in_place=True)
        assert tinfo.rows_rendered == got.n_stale
        after = resident.cpu().numpy()
        fresh.upload_space(WORLD, b)
        f2, _ = split_frame(fresh, name, antialiasing)
        res = fresh.render(f2)
        want = rp.frame_bytes(res["color_f16"].view(np.uint16), res["depth"])
        assert (before != want).any(), "the edit shows"
        assert (after == want).all()


def test_the_interactive_loop_through_the_host_mirror():
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H

    name = "plaza"
    n = W * HT
    a, edits, eye, target = S.case(name)

    def renderer(sp):
        cams = H.StandardCameras()
        cams.graphics_options = H.GraphicsOptions()
        cams.viewport = H.Viewport.with_scale(1.0, W, HT)
        cams.world_space = A.space_from_flat(sp)
        cams.world_view_transform = H.look_at_y_up(eye, target)
        r = H.HipRtRenderer(cams)
        r.update()
        return r, cams

    r, keep = renderer(a)
    resident = rp.to_device(rp.split_bytes(r.draw_split()))
    before = resident.cpu().numpy().copy()
    r.update()
    assert r.changed_boxes() == []
    info = r.replace_cube_grid_device(WORLD, on_device(S.edited(name).block_index).data_ptr())
    assert info["n_cubes"] == len(edits) and info["merged"] == 0
    assert sorted(map(tuple, r.changed_boxes())) == sorted(map(tuple, S.boxes(name).tolist())) and r.pick_skip_stale == 0
    order_dev = pk.to_device_words(abi.pixel_order(W, HT)[0])
    picks = pk.out_words(n)
    got = r.pick_stale_cubes(resident.data_ptr(), order_dev.data_ptr(), picks.data_ptr(), n, n, 0)
    assert 0 < got["n_stale"] < n and got["n_from_stale"] == got["n_stale"]
    r.trace_pixels_into(resident.data_ptr(), picks.data_ptr(), got["n_from_stale"])
    after = resident.cpu().numpy()
    r2, keep2 = renderer(S.edited(name))
    want = rp.split_bytes(r2.draw_split())
    assert (before != want).any() and (after == want).all()


# --- 8. frames in flight ------------------------------------------------------------------------------------------------------------------
def test_a_frame_in_flight_is_the_old_scenes(ctx):
    name = "terrace"
    a, b = S.case(name)[0], S.edited(name)
    ctx.upload_space(WORLD, a)
    ctx.set_options(WORLD, to_abi_options(S.options(0)))
    ctx.clear_space(abi.LAYER_UI)
    frame = ctx.make_frame(W, HT, world_inv=loop_camera(name)[0])
    old = ctx.render(frame)["rgba8"].copy()
    buf = torch.zeros((HT, W, 4), dtype=torch.uint8, device="cuda:0")
    new = on_device(b.block_index)
    ctx.render_submit(frame, buf.data_ptr(), 1)
    boxes, info = ctx.replace_cube_grid(WORLD, new)
    assert info["n_cubes"] == len(S.case(name)[1])
    ctx.render_wait(1)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == old).all()
    with abi.Context(0) as fresh:
        fresh.upload_space(WORLD, b)
        fresh.set_options(WORLD, to_abi_options(S.options(0)))
        want = fresh.render(frame)["rgba8"].copy()
    got = ctx.render(frame)["rgba8"]
    assert (got == want).all() and (want != old).any()
    # a copy is legal with a frame in flight on another slot
    ctx.render_submit(frame, buf.data_ptr(), 1)
    back = torch.zeros(b.block_index.size, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    ctx.copy_cube_grid(WORLD, back)
    ctx.render_wait(1)
    assert (back.cpu().numpy().view(np.uint16).reshape(b.size) == b.block_index).all()


# --- the call recorder ----------------------------------------------------------------------------------------------------------------------
RECORDING = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from all_is_cubes_amd import abi
from tests import test_gpu_grid_replace as t
a, b, light, frame = t.recorded_scene()
live = []
with abi.Context(0) as c:  # (AIC_DUMP is in this process's environment: the recorder is armed when the context is created)
    c.upload_space(t.WORLD, a)
    c.set_options(t.WORLD, t.to_abi_options(t.S.options(0)))
    c.replace_cube_grid(t.WORLD, t.on_device(b.block_index), capacity=5)
    live.append(c.render(frame)["rgba8"].copy())
    c.replace_cube_grid(t.WORLD, t.on_device(a.block_index), t.light_on_device(light), capacity=0)
    live.append(c.render(frame)["rgba8"].copy())
    c.update_light_volume_device(t.WORLD, t.light_on_device(a.light))
    live.append(c.render(frame)["rgba8"].copy())
np.save(sys.argv[2], np.stack(live))
"""


def recorded_scene():
    name = "plaza"
    a, b = S.case(name)[0], S.edited(name)
    light = np.random.default_rng(8).integers(40, 250, a.light.shape).astype(np.uint8)
    light[..., 3] = flat.STATUS_VISIBLE
    return a, b, light, abi.Context.make_frame(W, HT, world_inv=loop_camera(name)[0])


def test_the_library_records_the_call_and_the_record_replays(tmp_path):
    """The recording runs in a process of its own: the library numbers the dump files of a process's contexts, and this file's must not move the
    number another test's file gets."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    from all_is_cubes_amd import replay

    a, b, light, _ = recorded_scene()
    path, frames = tmp_path / "grid.aic", tmp_path / "live.npy"
    root = str(Path(__file__).resolve().parents[1])
    out = subprocess.run([sys.executable, "-c", RECORDING, root, str(frames)], env=dict(os.environ, AIC_DUMP=str(path)), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    live = np.load(frames)
    records = list(replay.read_dump(path))
    tags = [r.tag for r in records]
    grids = [r.data for r in records if r.tag == replay.GRID]
    assert tags.count(replay.GRID) == 2 and tags.count(replay.LIGHT) == 1
    assert (grids[0]["block_index"].reshape(b.size) == b.block_index).all() and grids[0]["light"] is None and grids[0]["capacity"] == 5
    assert (grids[1]["block_index"].reshape(a.size) == a.block_index).all() and (grids[1]["light"].reshape(light.shape) == light).all() and grids[1]["capacity"] == 0
    again = replay.replay(path)
    assert len(again) == 3 and all((x == y).all() for x, y in zip(again, live))
    assert (live[0] != live[1]).any() and (live[1] != live[2]).any()
