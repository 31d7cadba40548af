"""GPU tests (-m gpu) of aic_light_rays: the records, infos and device-made lines of compute_light::<LightUpdateCubeInfo> against the
restatement (tests/light_rays_ref.py: pinned to the oracle by `cost`) entry for entry and f32 by bit pattern, `result` and `cost` against
oracle.compute_light itself; batch shapes, capacities, host against device lists, frames in flight, a light update in flight, errors."""
import copy

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi, flat
from tests import light_rays_ref as ref

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
W, HGT = 64, 48


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def on_device(ctx, cubes, maximum_distance, capacity, want_rays=True, want_lines=True, layer=abi.LAYER_WORLD):
    """The AIC_LIGHT_RAYS_DEVICE form: records and lines in tensors on the device, a guard behind each; returns (infos, rays, lines, totals) with the
    lists cut to what the infos say was stored"""
    import torch

    n = len(cubes)
    ray_bytes, line_bytes = 40 * capacity, 56 * (12 * n + 29 * capacity)
    d_rays = torch.full((ray_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_lines = torch.full((line_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    infos, totals = ctx.light_rays_device(layer, cubes, maximum_distance, capacity, d_rays.data_ptr() if want_rays else 0, d_lines.data_ptr() if want_lines else 0)
    stored = infos[(infos["flags"] & abi.LIGHT_CUBE_STORED) != 0]
    n_rays = int(stored["n_rays"].sum())
    n_lines = 12 * len(stored) + 29 * n_rays
    rays, lines = d_rays.cpu().numpy(), d_lines.cpu().numpy()
    assert (rays[40 * n_rays if want_rays else 0:] == 0xA5).all(), "wrote past the stored records"
    assert (lines[56 * n_lines if want_lines else 0:] == 0xA5).all(), "wrote past the stored lines"
    return infos, rays[:40 * n_rays].view(abi.LIGHT_RAY_DTYPE), lines[:56 * n_lines].view(abi.LINE_VERTEX_DTYPE), totals


def rows(a):
    return a.view(np.uint8).reshape(len(a), a.dtype.itemsize)


def same(got, want, what):
    gi, gr, gl, gt = got
    wi, wr, wl, wt = want
    assert gt == wt, (what, gt, wt)
    assert len(gi) == len(wi), (what, "infos", len(gi), len(wi))
    bad = np.flatnonzero((rows(gi) != rows(wi)).any(axis=1))
    assert len(bad) == 0, (what, "infos", bad[:8], gi[bad[:2]], wi[bad[:2]])
    assert len(gr) == len(wr), (what, "records", len(gr), len(wr))
    bad = np.flatnonzero((rows(gr) != rows(wr)).any(axis=1))
    assert len(bad) == 0, (what, "records", bad[:8], gr[bad[:2]], wr[bad[:2]])
    if gl is not None:
        assert len(gl) == len(wl), (what, "lines", len(gl), len(wl))
        bad = np.flatnonzero((rows(gl) != rows(wl)).any(axis=1))
        assert len(bad) == 0, (what, "lines", bad[:8], gl[bad[:2]], wl[bad[:2]])


def upload(ctx, name):
    sp, t = ref.scene(name)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    return sp, t


@pytest.mark.parametrize("case", ["closed_cell", "spread_6", "spread_30", "slab_6", "slab_30", "edges"])
def test_device_equals_the_restatement(ctx, case):
    """Records, infos and device-made lines equal the restatement's; result and cost are the oracle's (ref.answer puts oracle.compute_light's texel into
    the infos and has checked its cost); host lists and device lists are identical."""
    name, cubes, md = ref.cases()[case]
    upload(ctx, name)
    want = ref.answer(case)
    print(case, "cubes", len(cubes), "records", want[3][0], "most of one cube", int(want[0]["n_rays"].max()))
    same(ctx.light_rays(abi.LAYER_WORLD, cubes, md), want, case)
    same(on_device(ctx, cubes, md, want[3][0]), want, case + ", device lists")


def test_closed_cell_has_its_six_records(ctx):
    sp, t = upload(ctx, "closed_cell")
    infos, rays, lines, totals = ctx.light_rays(abi.LAYER_WORLD, [(1, 1, 1)], 30)
    assert totals == (6, 12 + 29 * 6) and infos["n_rays"][0] == 6 and len(lines) == 2 * totals[1]
    centre = np.asarray(sp.light).reshape(3, 3, 3, 4)[1, 1, 1]
    for f, r in enumerate(rays):
        assert tuple(r["trigger_cube"]) == tuple(1 + v for v in ref.NORMALS[f]) and tuple(r["value_cube"]) == (1, 1, 1) and np.array_equal(r["value"], centre)
        colour, emission = (ref.LAMP_COLOR, ref.LAMP_EMISSION) if f == 0 else ((0.5, 0.25, 0.75, 1.0), (0.0, 0.0, 0.0))
        want = (np.array(emission, np.float32) + np.array(colour[:3], np.float32) * t.lut[centre[:3]]).astype(np.float32)
        assert r["light_from_struck_face"].tobytes() == want.tobytes()
    # distance 0: the walk stops at the origin cube, no record
    infos, rays, _, totals = ctx.light_rays(abi.LAYER_WORLD, [(1, 1, 1)], 0)
    assert totals == (0, 12) and len(rays) == 0


def test_edge_cases_carry_their_flags(ctx):
    upload(ctx, "light_spread")
    name, cubes, md = ref.cases()["edges"]
    infos, rays, lines, totals = ctx.light_rays(abi.LAYER_WORLD, cubes, md)
    outside = (infos["flags"] & abi.LIGHT_CUBE_OUTSIDE) != 0
    assert outside.tolist() == [False, False, False, False, True, True, True, False]
    assert (infos["n_rays"][outside] == 0).all() and (infos["cost"][outside] == 0).all() and (infos["result"][outside] == 0).all()
    assert infos["n_rays"][0] == 0 and infos["cost"][0] == 0 and tuple(infos["result"][0]) == (0, 0, 0, 128)  # an opaque origin: PackedLight::OPAQUE
    assert infos["n_rays"][1] == 0 and infos["cost"][1] == 0 and infos["result"][1][3] == 1                   # every direction weight 0: NO_RAYS
    assert infos["n_rays"][7] > 0
    # the box of a cube outside the space is still drawn
    k = 4
    start = 2 * (12 * k + 29 * int(infos["first_ray"][k]))
    assert lines[start:start + 24].tobytes() == ref.wireframe(cubes[k], np.zeros(0, abi.LIGHT_RAY_DTYPE)).tobytes()


def test_batch_shapes_and_positions(ctx):
    """n = 0, 1, 63, 64, 65 and 300: the same cubes give the same records at every n and at every position in the batch"""
    _, t = upload(ctx, "light_spread")
    pool = ref.cases()["spread_6"][1]
    want_i, want_r, _, _ = ref.answer("spread_6")
    per_cube = {tuple(i["cube"]): (i, want_r[i["first_ray"]:i["first_ray"] + i["n_rays"]]) for i in want_i}
    infos, rays, lines, totals = ctx.light_rays(abi.LAYER_WORLD, np.zeros((0, 3), np.int32), 6)
    assert len(infos) == 0 and len(rays) == 0 and totals == (0, 0)
    for n, start in ((1, 417), (63, 5), (64, 100), (65, 333), (300, 650), (300, 0)):
        cubes = [pool[(start + 7 * j) % len(pool)] for j in range(n)]  # (another order than the case's: positions move)
        infos, rays, lines, totals = ctx.light_rays(abi.LAYER_WORLD, cubes, 6)
        first = 0
        for k, cube in enumerate(cubes):
            wi, wr = per_cube[tuple(cube)]
            assert tuple(infos[k]["cube"]) == tuple(cube) and infos[k]["first_ray"] == first and infos[k]["n_rays"] == len(wr), (n, k)
            assert infos[k]["cost"] == wi["cost"] and np.array_equal(infos[k]["result"], wi["result"]) and infos[k]["flags"] == abi.LIGHT_CUBE_STORED
            assert rays[first:first + len(wr)].tobytes() == wr.tobytes(), (n, k, cube)
            got_lines = lines[2 * (12 * k + 29 * first):2 * (12 * (k + 1) + 29 * (first + len(wr)))]
            assert got_lines.tobytes() == ref.wireframe(cube, wr).tobytes(), (n, k, cube)
            first += len(wr)
        assert totals == (first, 12 * n + 29 * first)


def test_capacity(ctx):
    """The total: everything stored. One less: the last cube with records loses STORED, and so does every cube behind it (first_ray + n_rays <= capacity
    fails for them too); the cubes before keep what they had. 0: only the leading cubes without records are stored."""
    _, t = upload(ctx, "light_spread")
    cubes = ref.cases()["spread_6"][1][400:440]
    full = ctx.light_rays(abi.LAYER_WORLD, cubes, 6)
    total = full[3][0]
    assert total > 0 and (full[0]["flags"] == abi.LIGHT_CUBE_STORED).all()
    with_rays = np.flatnonzero(full[0]["n_rays"] > 0)
    assert len(with_rays) > 3 and with_rays[0] > 0  # (the batch begins with a cube that has no record)
    for capacity in (total, total - 1, 0):
        want = ref.batch(t, cubes, 6, capacity)
        want[0]["result"] = full[0]["result"]
        for got, what in ((ctx.light_rays(abi.LAYER_WORLD, cubes, 6, capacity=capacity), "host"), (on_device(ctx, cubes, 6, capacity), "device")):
            same(got, want, f"capacity {capacity}, {what} lists")
            infos = got[0]
            stored = (infos["flags"] & abi.LIGHT_CUBE_STORED) != 0
            last = with_rays[-1] if capacity == total - 1 else (with_rays[0] if capacity == 0 else len(cubes))
            assert stored.tolist() == [k < last for k in range(len(cubes))]
            assert got[3] == (total, 12 * len(cubes) + 29 * total)  # the totals are always the whole batch's
            kept = int(infos["n_rays"][stored].sum())
            assert got[1].tobytes() == full[1][:kept].tobytes()
    # each output alone, and none: the infos are the same
    for want_rays, want_lines in ((True, False), (False, True), (False, False)):
        got = on_device(ctx, cubes, 6, total, want_rays, want_lines)
        assert got[0].tobytes() == full[0].tobytes() and got[3] == full[3]
        if want_rays:
            assert got[1].tobytes() == full[1].tobytes()
        if want_lines:
            assert got[2].tobytes() == full[2].tobytes()
    infos, rays, lines, totals = ctx.light_rays(abi.LAYER_WORLD, cubes, 6, want_lines=False)
    assert lines is None and infos.tobytes() == full[0].tobytes() and rays.tobytes() == full[1].tobytes()


def test_frames_in_flight_keep_their_image():
    """A frame submitted before the call and collected after it is the frame rendered alone, and the call's answer is the answer of an idle context."""
    import torch

    sp, _ = ref.scene("light_spread")
    name, cubes, md = ref.cases()["spread_30"]
    want = ref.answer("spread_30")
    q = oracle.look_at_y_up((0.0, 0.0, 8.0), (0.0, 0.0, 0.0))
    _, _, inv = oracle.camera_matrices(45.0, 200.0, W / HGT, q, (0.0, 0.0, 8.0))
    with abi.Context(0) as c:
        c.upload_space(abi.LAYER_WORLD, sp)
        c.set_options(abi.LAYER_WORLD, abi.make_options())
        frame = c.make_frame(W, HGT, world_inv=inv)
        alone = c.render(frame)["rgba8"]
        outs = [torch.zeros((HGT, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        for slot, o in enumerate(outs):
            c.render_submit(frame, o.data_ptr(), slot)
        busy = c.light_rays(abi.LAYER_WORLD, cubes, md)
        busy_d = on_device(c, cubes, md, want[3][0])
        for slot in range(2):
            c.render_wait(slot)
        same(busy, want, "frames in flight")
        same(busy_d, want, "frames in flight, device lists")
        for o in outs:
            assert (o.cpu().numpy() == alone).all()
        assert (c.render(frame)["rgba8"] == alone).all()


def test_a_submitted_light_update_is_published_first(ctx):
    """An update submitted and not waited for: the call finishes and publishes it, and the records read the new texels."""
    lit, t_lit = ref.scene("light_spread")
    dark = copy.deepcopy(lit)
    dark.light[...] = (0, 0, 0, flat.STATUS_UNINITIALIZED)
    name, cubes, md = ref.cases()["spread_30"]
    want = ref.answer("spread_30")
    ctx.upload_space(abi.LAYER_WORLD, dark)
    before = ctx.light_rays(abi.LAYER_WORLD, cubes, md)
    assert before[3] == want[3] and (before[1]["value"] == (0, 0, 0, 0)).all() and (want[1]["value"][:, 3] != 0).all()
    ctx.evaluate_light_submit(abi.LAYER_WORLD, 30)
    got = ctx.light_rays(abi.LAYER_WORLD, cubes, md)
    ctx.evaluate_light_wait(abi.LAYER_WORLD)
    assert (ctx.read_light_volume(abi.LAYER_WORLD, lit.size) == np.asarray(lit.light).reshape(*lit.size, 4)).all()
    same(got, want, "behind a submitted update")


def test_scene_and_light_writes_are_seen(ctx):
    """The tables follow the scene: a block placed, a texel written, another maximum_distance -- each answer is the restatement's for the space as it is"""
    sp = copy.deepcopy(ref.scene("light_spread")[0])
    ctx.upload_space(abi.LAYER_WORLD, sp)
    cubes = [(1, 1, 1), (2, 3, 0), (-3, 0, 1)]
    same(ctx.light_rays(abi.LAYER_WORLD, cubes, 6), with_results(sp, cubes, 6), "as uploaded")
    sp.set((1, 1, 2), 1)  # a wall cube over the first cube
    ctx.update_cubes(abi.LAYER_WORLD, [(1, 1, 2)], [1])
    same(ctx.light_rays(abi.LAYER_WORLD, cubes, 6), with_results(sp, cubes, 6), "a block placed")
    light = np.asarray(sp.light).reshape(*sp.size, 4).copy()
    light[11, 11, 2] = (200, 10, 99, 255)  # the light of (1, 1, 1)
    sp.light = light
    ctx.update_light_volume(abi.LAYER_WORLD, light)
    same(ctx.light_rays(abi.LAYER_WORLD, cubes, 6), with_results(sp, cubes, 6), "a texel written")
    same(ctx.light_rays(abi.LAYER_WORLD, cubes, 9), with_results(sp, cubes, 9), "another distance")
    same(ctx.light_rays(abi.LAYER_WORLD, cubes, 6), with_results(sp, cubes, 6), "and back")


def with_results(sp, cubes, md):
    want = ref.batch(ref.Tables(sp), cubes, md)
    osp = oracle.Space(sp)
    for k, cube in enumerate(cubes):
        texel, cost = oracle.compute_light(osp, cube, md)
        assert cost == want[0][k]["cost"]
        want[0][k]["result"] = texel
    return want


def test_errors_leave_the_context_usable():
    import torch

    lib = abi.load()
    sp, _ = ref.scene("closed_cell")
    cubes = np.ascontiguousarray([(1, 1, 1)] * 4, np.int32)
    infos = np.zeros(4, abi.LIGHT_CUBE_INFO_DTYPE)
    rays = np.zeros(24, abi.LIGHT_RAY_DTYPE)
    totals = np.full(2, 7, np.uint64)
    with abi.Context(0) as c:
        call = lambda layer, n, cu, md, flags, r, l: lib.aic_light_rays(c._h, layer, n, cu, md, flags, 24, infos.ctypes.data, r, l, totals.ctypes.data)
        assert call(abi.LAYER_WORLD, 4, cubes.ctypes.data, 6, 0, rays.ctypes.data, None) == ERR_INVALID  # no space yet
        c.upload_space(abi.LAYER_WORLD, sp)
        assert call(abi.LAYER_UI, 4, cubes.ctypes.data, 6, 0, rays.ctypes.data, None) == ERR_INVALID
        assert call(2, 4, cubes.ctypes.data, 6, 0, rays.ctypes.data, None) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 4, None, 6, 0, rays.ctypes.data, None) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 4, cubes.ctypes.data, 6, 2, rays.ctypes.data, None) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 4, cubes.ctypes.data, -1, 0, rays.ctypes.data, None) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 4, cubes.ctypes.data, 256, 0, rays.ctypes.data, None) == ERR_INVALID
        assert call(abi.LAYER_WORLD, (1 << 16) + 1, cubes.ctypes.data, 6, 0, rays.ctypes.data, None) == ERR_INVALID
        d_rays = torch.zeros(24 * 40 + 8, dtype=torch.uint8, device="cuda:0")
        d_lines = torch.zeros(56 * (48 + 29 * 24) + 8, dtype=torch.uint8, device="cuda:0")
        assert call(abi.LAYER_WORLD, 4, cubes.ctypes.data, 6, abi.LIGHT_RAYS_DEVICE, d_rays.data_ptr() + 2, d_lines.data_ptr()) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 4, cubes.ctypes.data, 6, abi.LIGHT_RAYS_DEVICE, d_rays.data_ptr(), d_lines.data_ptr() + 1) == ERR_INVALID
        assert (infos.view(np.uint8) == 0).all() and (rays.view(np.uint8) == 0).all() and (totals == 7).all() and (d_rays.cpu().numpy() == 0).all()
        with pytest.raises(abi.AicError):
            c.light_rays(abi.LAYER_UI, cubes, 6)
        want = ref.answer("closed_cell")
        got = c.light_rays(abi.LAYER_WORLD, cubes, 6)
        assert got[3] == (24, 48 + 29 * 24) and (got[0]["n_rays"] == 6).all() and got[1][18:].tobytes() == want[1].tobytes()
        assert call(abi.LAYER_WORLD, 0, None, 6, 0, None, None) == abi.AIC_OK and (totals == 0).all()


# ---- the host mirror ---------------------------------------------------------------------------------------------------

def test_light_rays_at_cursor_through_the_mirror():
    """GraphicsOptions::debug_light_rays_at_cursor: project_cursor hits the closed cell's +X wall from inside the cell, so cursor.preceding_cube() is the
    centre and compute_light there has its six records. The presentation draws the cursor's lines and then the records' lines from one list made on the
    device: the image is the line reference's (tests/present_lines_ref.py) fed the restatement's lines behind the cursor's. Option off: today's image."""
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H
    from tests import present_lines_ref
    from tests.test_gpu_present_lines import view_projection_of
    from tests.test_gpu_reproject import split_bytes, to_device

    w, h = 40, 24
    n = w * h
    sp, _ = ref.scene("closed_cell")
    cams = H.StandardCameras()
    o = H.GraphicsOptions()
    o.bloom_intensity = 0.0
    o.debug_light_rays_at_cursor = True
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(sp)
    cams.world_view_transform = H.look_at_y_up((1.3, 1.6, 1.7), (3.0, 1.4, 1.5))
    r = H.HipRtRenderer(cams)
    r.light_rays_maximum_distance = 6
    r.update()
    cursor = r.project_cursor(0.0, 0.0)
    assert cursor is not None and tuple(cursor.cube) == (2, 1, 1) and cursor.layer == abi.LAYER_WORLD and tuple(cursor.preceding_cube_or_cube()) == (1, 1, 1)
    # light_rays through the mirror: the restatement's records and the host's lines
    want_infos, want_rays, want_lines, _ = ref.answer("closed_cell")
    (info, rays, lines), = r.light_rays(abi.LAYER_WORLD, [(1, 1, 1)], 6)
    assert info.tobytes() == want_infos.tobytes() and rays.tobytes() == want_rays.tobytes() and lines.tobytes() == want_lines.tobytes()
    r.update(cursor)
    src = to_device(split_bytes(r.draw_split()))
    raw = src.cpu().numpy()
    color, depth = raw[:n * 8].view(np.uint16).reshape(h, w, 4), raw[n * 8:n * 12].view(np.uint32).reshape(h, w)
    m = view_projection_of(r.world_camera())
    own = np.asarray(cursor.wireframe(), np.float32).reshape(-1, 7)
    both = np.concatenate([own, want_lines.view(np.float32).reshape(-1, 7)])
    want, counts = present_lines_ref.present(color, depth, (w, h), both, m, 0.0, int(o.tone_mapping), o.maximum_intensity)
    shown, got_counts = r.present_split_lines(src.data_ptr(), w, h, None)
    print("cursor and light rays:", got_counts)
    assert got_counts == counts and (shown.data == want).all()
    today, today_counts = r.present_split_lines(src.data_ptr(), w, h, own)
    assert today_counts["n_pixels"] < counts["n_pixels"] and (today.data != shown.data).any()
    # a cursor of the UI space draws its own lines only (debug_lines.rs:51-58: is_same_space)
    cursor.layer = abi.LAYER_UI
    r.update(cursor)
    ui, ui_counts = r.present_split_lines(src.data_ptr(), w, h, None)
    assert ui_counts == today_counts and (ui.data == today.data).all()
    # the option off: today's image
    cursor.layer = abi.LAYER_WORLD
    o.debug_light_rays_at_cursor = False
    cams.graphics_options = o
    r.update(cursor)
    off, off_counts = r.present_split_lines(src.data_ptr(), w, h, None)
    assert off_counts == today_counts and (off.data == today.data).all()
    assert (src.cpu().numpy() == raw).all(), "the frame changed"
