"""GPU tests (-m gpu) of aic_cursor_raycast and of project_cursor through the host mirror: cursor_raycast (all-is-cubes/src/character/cursor.rs:26-107)
and StandardCameras::project_cursor (all-is-cubes-render/src/camera/stdcam.rs:357-389) on the device.

Yardstick: tests/cursor_ref.py, the function restated over the CPU oracle's Raycaster. Every field of every record is compared, integers exactly and f64
by bit pattern -- that is, the bytes of the records' fields. Scenes are at most 8^3 cubes with blocks of resolution 2 to 16; tests/test_cursor_cpu.py checks that the
case list reaches every outcome."""
import copy
import ctypes

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi, flat
from tests import cursor_ref as ref

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
CASES = ref.cases()
W, HGT = 64, 48
INF = float("inf")


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def raycast_on_device(ctx, rays, maximum_distance, layer=abi.LAYER_WORLD) -> np.ndarray:
    """The AIC_RAYS_DEVICE form: rays and records in tensors on the device, a guard record behind the output"""
    import torch

    r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    size = abi.CURSOR_HIT_DTYPE.itemsize
    d_rays = torch.from_numpy(r.copy()).to("cuda:0")
    d_out = torch.full(((len(r) + 1) * size,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.cursor_raycast_device(layer, len(r), d_rays.data_ptr(), maximum_distance, d_out.data_ptr())
    out = d_out.cpu().numpy()
    assert (out[len(r) * size:] == 0xA5).all(), "wrote past the records"
    return out[:len(r) * size].view(abi.CURSOR_HIT_DTYPE)


def check(ctx, scene: ref.Scene, rays, maximum_distance, what="", want=None):
    want = scene.raycast_all(rays, maximum_distance) if want is None else want
    got = ctx.cursor_raycast(abi.LAYER_WORLD, rays, maximum_distance)
    bad = ref.same_records(got, want)
    assert len(bad) == 0, (what, bad[:8], got[bad[:1]], want[bad[:1]])
    bad = ref.same_records(raycast_on_device(ctx, rays, maximum_distance), want)
    assert len(bad) == 0, (what, "device pointers", bad[:8])
    return want


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_device_equals_the_restatement(ctx, case):
    name, key, rays, maximum_distance = CASES[case]
    scene = ref.scene(key)
    ctx.upload_space(abi.LAYER_WORLD, scene.sp)
    want = check(ctx, scene, rays, maximum_distance, name)
    assert not np.isnan(want["distance_to_point"]).any()


def test_batch_sizes(ctx):
    scene = ref.scene("garden")
    ctx.upload_space(abi.LAYER_WORLD, scene.sp)
    rays = ref.garden_rays()
    assert len(rays) == 130
    whole = scene.raycast_all(rays, INF)
    assert 0 < whole["hit"].sum() < len(rays)
    for n in (1, 10, 64, 65, 130):  # (65: a second wave with one live lane)
        check(ctx, scene, rays[:n], INF, f"n = {n}", want=whole[:n])
    check(ctx, scene, rays[64:65], INF, "one ray", want=whole[64:65])
    assert ctx.cursor_raycast(abi.LAYER_WORLD, np.zeros((0, 6)), INF).shape == (0,)


@pytest.mark.parametrize("case", range(7), ids=[t[0] for t in ref.reference_tests()])
def test_the_references_own_tests(ctx, case):
    name, make_space, ray, maximum_distance, expected = ref.reference_tests()[case]
    sp = make_space()
    ctx.upload_space(abi.LAYER_WORLD, sp)
    got = check(ctx, ref.Scene(sp), ray[None, :], maximum_distance, name)[0]
    if expected is None:
        assert got["hit"] == 0
    else:
        assert got["hit"] == 1
        for field, value in expected.items():
            assert np.array_equal(got[field], value), (name, field, got[field])


def test_scene_changes_are_seen(ctx):
    sp = copy.deepcopy(ref.scene("garden").sp)
    rays = ref.garden_rays()
    ctx.upload_space(abi.LAYER_WORLD, sp)
    before = check(ctx, ref.Scene(sp), rays, INF, "as uploaded")
    # aic_update_cubes: a selectable block placed in front of the corridor's rays
    sp.set((0, 0, 3), ref.ATOM)
    ctx.update_cubes(abi.LAYER_WORLD, [(0, 0, 3)], [ref.ATOM])
    placed = check(ctx, ref.Scene(sp), rays, INF, "an atom placed in front")
    assert placed[0]["hit"] and tuple(placed[0]["cube"]) == (0, 0, 3) and len(ref.same_records(placed, before)) > 0
    # aic_replace_blocks in place: the atom becomes unselectable (the same ranges hold it)
    dull = flat.atom((0.5, 0.5, 0.5, 1.0))
    dull.selectable = False
    sp.blocks[ref.ATOM] = dull
    ctx.replace_blocks(abi.LAYER_WORLD, [(ref.ATOM, dull)])
    passed = check(ctx, ref.Scene(sp), rays, INF, "the atom made unselectable in place")
    assert tuple(passed[0]["cube"]) != (0, 0, 3)
    # ... appended: the checkered block outgrows its ranges (resolution 4 -> 8) and none of its voxels is selectable any more; a new block at the table's end
    bigger = flat.voxel_block(8, np.indices((8, 8, 8)).sum(0).astype(np.uint16) % 2,
                              np.stack([flat.evoxel((0, 0, 0, 0)), flat.evoxel((0.9, 0.1, 0.1, 0.5))]), name="c")
    bigger.voxel_selectable = [True, False]
    sp.blocks[ref.CHECKER] = bigger
    extra = flat.voxel_block(2, np.array([[[0, 1], [1, 0]], [[1, 0], [0, 1]]], np.uint16), np.stack([flat.evoxel((0, 0, 0, 0)), flat.evoxel((0.2, 0.3, 0.9, 1.0))]), name="x")
    new_index = sp.add_block(extra)
    ctx.replace_blocks(abi.LAYER_WORLD, [(ref.CHECKER, bigger), (new_index, extra)])
    sp.set((0, 0, 3), new_index)
    ctx.update_cubes(abi.LAYER_WORLD, [(0, 0, 3)], [new_index])
    appended = check(ctx, ref.Scene(sp), rays, INF, "a block grown past its ranges, a block appended")
    assert appended[0]["block_index"] == new_index
    ctx.compact(abi.LAYER_WORLD)
    check(ctx, ref.Scene(sp), rays, INF, "after aic_compact", want=appended)


def test_frames_do_not_move_and_are_not_disturbed(ctx):
    import torch

    scene = ref.scene("garden")
    rays = ref.garden_rays()
    want = scene.raycast_all(rays, INF)
    frames = []
    for eye in ((1.5, 2.5, 9.0), (8.0, -3.0, 6.0)):
        q = oracle.look_at_y_up(eye, (1.0, 1.5, 0.5))
        _, _, inv = oracle.camera_matrices(45.0, 200.0, W / HGT, q, eye)
        frames.append(inv)
    with abi.Context(0) as c:  # (a context of its own: its first raycast is this test's)
        c.upload_space(abi.LAYER_WORLD, scene.sp)
        c.set_options(abi.LAYER_WORLD, abi.make_options())
        frames = [c.make_frame(W, HGT, world_inv=inv) for inv in frames]
        before = [c.render(f)["rgba8"] for f in frames]
        assert len(ref.same_records(c.cursor_raycast(abi.LAYER_WORLD, rays, INF), want)) == 0
        after = [c.render(f)["rgba8"] for f in frames]
        for a, b in zip(before, after):
            assert (a == b).all()
        outs = [torch.zeros((HGT, W, 4), dtype=torch.uint8, device="cuda:0") for _ in frames]
        torch.cuda.synchronize()
        for slot, (f, o) in enumerate(zip(frames, outs)):
            c.render_submit(f, o.data_ptr(), slot)
        busy = c.cursor_raycast(abi.LAYER_WORLD, rays, INF)
        busy_d = raycast_on_device(c, rays, INF)
        for slot in range(len(frames)):
            c.render_wait(slot)
        assert len(ref.same_records(busy, want)) == 0 and len(ref.same_records(busy_d, want)) == 0
        for o, alone in zip(outs, before):
            assert (o.cpu().numpy() == alone).all()


def test_light_evaluated_on_the_device_is_reported(ctx):
    sp = copy.deepcopy(ref.scene("garden").sp)
    sp.light[...] = (0, 0, 0, flat.STATUS_UNINITIALIZED)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    rays = ref.garden_rays()
    dark = check(ctx, ref.Scene(sp), rays, INF, "unlit")
    ctx.evaluate_light(abi.LAYER_WORLD, 30)
    volume = ctx.read_light_volume(abi.LAYER_WORLD, sp.size)
    sp.light = volume
    lit = check(ctx, ref.Scene(sp), rays, INF, "lit on the device")
    hits = np.flatnonzero(lit["hit"])
    assert len(hits) > 20 and (lit["light_hit"] != dark["light_hit"]).any()
    lo = np.asarray(sp.lo)
    for i in hits:
        assert (lit["light_hit"][i] == volume[tuple(lit["cube"][i] - lo)]).all()
        p = lit["preceding_cube"][i] - lo
        if lit["has_preceding"][i] and (p >= 0).all() and (p < np.asarray(sp.size)).all():
            assert (lit["light_preceding"][i] == volume[tuple(p)]).all()
    # a submitted update is finished and published by the raycast itself
    sp2 = copy.deepcopy(ref.scene("garden").sp)
    sp2.light[...] = (0, 0, 0, flat.STATUS_UNINITIALIZED)
    ctx.upload_space(abi.LAYER_WORLD, sp2)
    ctx.evaluate_light_submit(abi.LAYER_WORLD, 30)
    got = ctx.cursor_raycast(abi.LAYER_WORLD, rays, INF)
    ctx.evaluate_light_wait(abi.LAYER_WORLD)
    assert len(ref.same_records(got, lit)) == 0


def test_errors_leave_the_context_usable():
    import torch

    lib = abi.load()
    scene = ref.scene("garden")
    rays = np.ascontiguousarray(ref.garden_rays()[:10])
    out = np.zeros(10, abi.CURSOR_HIT_DTYPE)
    with abi.Context(0) as c:
        call = lambda layer, n, r, md, flags, o: lib.aic_cursor_raycast(c._h, layer, n, r, md, flags, o)
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, INF, 0, out.ctypes.data) == ERR_INVALID  # no space yet
        c.upload_space(abi.LAYER_WORLD, scene.sp)
        assert call(abi.LAYER_UI, 10, rays.ctypes.data, INF, 0, out.ctypes.data) == ERR_INVALID      # a layer without a space
        assert call(2, 10, rays.ctypes.data, INF, 0, out.ctypes.data) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, INF, 1, out.ctypes.data) == ERR_INVALID   # unknown flag bits
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, INF, abi.RAYS_DEVICE | 128, out.ctypes.data) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 10, None, INF, 0, out.ctypes.data) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, INF, 0, None) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, float("nan"), 0, out.ctypes.data) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, -1.0, 0, out.ctypes.data) == ERR_INVALID
        d_rays = torch.zeros(10 * 6 + 1, dtype=torch.float64, device="cuda:0")
        d_out = torch.zeros(11 * 144, dtype=torch.uint8, device="cuda:0")
        assert call(abi.LAYER_WORLD, 10, d_rays.data_ptr() + 4, INF, abi.RAYS_DEVICE, d_out.data_ptr()) == ERR_INVALID  # misaligned device pointers
        assert call(abi.LAYER_WORLD, 10, d_rays.data_ptr(), INF, abi.RAYS_DEVICE, d_out.data_ptr() + 4) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 0, None, INF, 0, None) == abi.AIC_OK
        assert (out.view(np.uint8) == 0).all() and (d_out.cpu().numpy() == 0).all()
        with pytest.raises(abi.AicError):
            c.cursor_raycast(abi.LAYER_UI, rays, INF)
        # a palette whose eighth float is neither 1.0 nor 0.0 under AIC_BLOCK_VOXEL_SELECTABLE is refused, and the scene stays
        bad = flat.atom((0.5, 0.5, 0.5, 1.0))
        d, vox, pal = flat.pack_block(bad)
        d["flags"] |= flat.FLAG_VOXEL_SELECTABLE
        pal[0, 7] = 0.5
        desc = abi.BlockDesc.from_buffer_copy(d.tobytes())
        assert lib.aic_replace_block(c._h, abi.LAYER_WORLD, ref.ATOM, ctypes.byref(desc), vox.ctypes.data, pal.ctypes.data) == ERR_INVALID
        # the context still raycasts at 0 and at +inf
        for md in (0.0, INF):
            got = c.cursor_raycast(abi.LAYER_WORLD, rays, md)
            assert len(ref.same_records(got, scene.raycast_all(rays, md))) == 0


# ---- the host mirror ---------------------------------------------------------------------------------------------------

def column_space(block: flat.BlockDef) -> flat.FlatSpace:
    """1 x 1 x 10 cubes of air along Z with `block` at the origin end, every cube's light its own"""
    sp = flat.FlatSpace((0, 0, 0), (1, 1, 10))
    sp.set_sky_uniform((0.5, 0.6, 0.7))
    sp.add_block(flat.air())
    sp.set((0, 0, 0), sp.add_block(block))
    sp.light[0, 0, :, 0] = np.arange(10) + 60
    return sp


def mirror(world, world_eye_z, ui=None):
    """A renderer over `world` seen along -Z from (0.5, 0.5, world_eye_z), and over `ui` (if any) seen from 20 cubes up the same axis"""
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H

    cams = H.StandardCameras()
    o = H.GraphicsOptions()
    o.bloom_intensity = 0.0
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, 40, 24)
    cams.world_space = A.space_from_flat(world)
    cams.world_view_transform = H.look_at_y_up((0.5, 0.5, world_eye_z), (0.5, 0.5, 0.0))
    if ui is not None:
        state = H.UiViewState()
        state.space = A.space_from_flat(ui)
        state.view_transform = H.look_at_y_up((0.5, 0.5, 20.5), (0.5, 0.5, 0.0))
        state.graphics_options = o
        cams.ui = state
    r = H.HipRtRenderer(cams)
    r.update()
    return cams, r


def ray_of(camera, x, y) -> np.ndarray:
    origin, direction = camera.project_ndc_into_world(x, y)
    return np.concatenate([origin, direction]).astype(np.float64)


def assert_cursor_is(cursor, rec):
    assert cursor is not None and rec["hit"] == 1
    assert tuple(cursor.cube) == tuple(rec["cube"]) and (cursor.face_entered, cursor.face_selected) == (rec["face_entered"], rec["face_selected"])
    assert np.asarray(cursor.point_entered, np.float64).tobytes() == rec["point_entered"].tobytes()
    assert np.float64(cursor.distance_to_point).tobytes() == rec["distance_to_point"].tobytes()
    assert (tuple(cursor.voxel_lo), tuple(cursor.voxel_size), cursor.resolution) == (tuple(rec["voxel_lo"]), tuple(rec["voxel_size"]), rec["resolution"])
    assert cursor.block_index == rec["block_index"] and tuple(cursor.voxel) == tuple(rec["voxel"]) and tuple(cursor.light) == tuple(rec["light_hit"])
    if rec["has_preceding"]:
        assert tuple(cursor.preceding_cube) == tuple(rec["preceding_cube"]) and tuple(cursor.preceding_light) == tuple(rec["light_preceding"])
    else:
        assert cursor.preceding_cube is None and cursor.preceding_light is None


def test_project_cursor_through_the_mirror():
    from all_is_cubes_amd import _host as H
    from tests.test_gpu_reproject import split_bytes, to_device

    world = column_space(ref.slab(3, 4))
    ui_hit, ui_miss = column_space(flat.atom((0.9, 0.9, 0.2, 1.0))), column_space(ref.white_unselectable())
    # a selectable block of the UI space under the point: the UI's hit, at any distance
    _, r = mirror(world, 4.5, ui_hit)
    want = ref.Scene(ui_hit).raycast(ray_of(r.ui_camera(), 0.0, 0.0), INF)
    assert want["hit"] and want["distance_to_point"] > 6.0
    assert_cursor_is(r.project_cursor(0.0, 0.0), want)
    # nothing selectable there: the world at 6.0
    cams, r = mirror(world, 4.5, ui_miss)
    ray = ray_of(r.world_camera(), 0.0, 0.0)
    want = ref.Scene(world).raycast(ray, 6.0)
    assert want["hit"] and tuple(want["cube"]) == (0, 0, 0) and want["face_entered"] == ref.PZ and want["resolution"] == 4
    found = r.project_cursor(0.0, 0.0)
    assert_cursor_is(found, want)
    assert_cursor_is(r.cursor_raycast(abi.LAYER_WORLD, ray, 6.0), want)
    many = r.cursor_raycast(abi.LAYER_WORLD, np.stack([ray, ray * [1, 1, 1, -1, -1, -1]]), 6.0)
    assert_cursor_is(many[0], want)
    assert many[1] is None
    # no UI space at all: the same; a block 7 cubes away: nothing
    _, r_plain = mirror(world, 4.5)
    assert_cursor_is(r_plain.project_cursor(0.0, 0.0), want)
    _, r_far = mirror(world, 8.0, ui_miss)
    far = ref.Scene(world).raycast(ray_of(r_far.world_camera(), 0.0, 0.0), INF)  # (7 from the eye; the camera's ray starts on the near plane)
    assert far["hit"] and 6.0 < far["distance_to_point"] <= 7.0
    assert r_far.project_cursor(0.0, 0.0) is None
    # the result goes straight into update(): the presentation draws what it draws for the hand-made Cursor of the same fields
    by_hand = H.Cursor()
    by_hand.cube, by_hand.face_entered, by_hand.face_selected = tuple(found.cube), found.face_entered, found.face_selected
    by_hand.point_entered, by_hand.distance_to_point = tuple(found.point_entered), found.distance_to_point
    by_hand.voxel_lo, by_hand.voxel_size, by_hand.resolution = tuple(found.voxel_lo), tuple(found.voxel_size), found.resolution
    assert (found.wireframe() == by_hand.wireframe()).all() and found.wireframe().shape == (56, 7)
    r.update(found)
    resident = to_device(split_bytes(r.draw_split()))
    shown, counts = r.present_split_lines(resident.data_ptr(), 40, 24)
    r.update(by_hand)
    shown_by_hand, counts_by_hand = r.present_split_lines(resident.data_ptr(), 40, 24)
    assert counts == counts_by_hand and counts["n_pixels"] > 0 and (shown.data == shown_by_hand.data).all()
    r.update()
    assert (r.present_split_lines(resident.data_ptr(), 40, 24)[0].data != shown.data).any()
