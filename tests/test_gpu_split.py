"""GPU tests (-m gpu) of AIC_FRAME_OUT_SPLIT: the two texels all-is-cubes-gpu's raytrace_to_texture stores per pixel (raytrace_to_texture.rs:594-675),
as bit patterns and with no pixel left out.

Expected values
 * colour plane: numpy on the SAME frame rendered with AIC_FRAME_OUT_COLORBUF (pinned to the oracle bit for bit by tests/test_gpu_linear_parity.py):
   light times the exposure of the pixel's layer in f32, a = clip(1 - t, 0, 1), `.astype(float16)`;
 * depth plane: oracle.trace_ray's DepthBuf of every sample ray (oracle.project_ndc_into_world at the pixel centre, or at the four sample points of
   renderer.rs:428-433; the UI ray with include_sky = False, the world ray where the UI sample did not end opaque), the minimum per sample and then per
   pixel, +inf for a painted sample, then the depth transform in numpy f64;
 * layer: a sample is the UI's if its UI trace or the backdrop left its ColorBuf visible, else the world's (the world's first visible hit, its sky, or the
   NO_WORLD_TO_SHOW paint, which REPLACES the sample: Split::default and one Paint hit made with the world's options); the pixel takes the first sample's.

Frames of 40 x 24: no multiple of the 16-pixel tile, so partial tiles and all four 8 x 8 quadrants are hit."""
import functools

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi, flat
from tests import scenes
from tests.test_gpu_parity import to_abi_options

pytestmark = pytest.mark.gpu

W, HT = 40, 24
WORLD_EXPOSURE, UI_EXPOSURE = 0.5, 2.0
SAMPLE_POINTS = [(1 / 8, 5 / 8), (3 / 8, 1 / 8), (5 / 8, 7 / 8), (7 / 8, 3 / 8)]  # renderer.rs:428-433
ZW_DEFAULT = (1.0, 0.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def mirror_zw(view_distance: float = 200.0):
    o = H.GraphicsOptions()
    o.view_distance = view_distance
    return tuple(H.Camera(o, H.Viewport.with_scale(1.0, W, HT)).depth_transform_zw())


def two_cube_ui_space() -> flat.FlatSpace:
    """scenes.ui_space with a second cube beside the opaque one, alpha 0.5: a UI sample is either opaque or far from it."""
    sp = flat.FlatSpace((-3, -3, -4), (2, 1, 1))
    sp.set_sky_uniform((1.0, 1.0, 0.5))
    sp.set((-3, -3, -4), sp.add_block(flat.atom((0.0, 1.0, 0.0, 1.0))))
    sp.set((-2, -3, -4), sp.add_block(flat.atom((0.0, 0.0, 1.0, 0.5))))
    return sp


def look(eye, target):
    return tuple(eye), tuple(oracle.look_at_y_up(eye, target))


# name -> (world space or None, UI space or None, options, (eye, quat), backdrop)
@functools.lru_cache(maxsize=None)
def case(name: str):
    plain = oracle.make_options()
    if name == "one_red_cube":
        return scenes.one_red_cube_space(), None, plain, look((0.7, 0.9, 2.5), (0.5, 0.5, 0.5)), (0, 0, 0, 0)
    if name == "partial_voxels":
        return scenes.partial_voxels_space(), None, plain, look((1.2, 1.4, 2.5), (1.0, 0.4, 0.5)), (0, 0, 0, 0)
    if name == "half_transparent_slab":
        return scenes.half_transparent_slab_space(), None, plain, look((0.8, 2.4, 2.2), (0.5, 1.2, 0.5)), (0, 0, 0, 0)
    if name == "antialias":
        return scenes.antialias_test_space()[0], None, oracle.unaltered_colors(antialiasing=2), look((0.0, 0.0, 0.0), (0.4, -0.2, -1.0)), (0, 0, 0, 0)
    if name == "ui_over_world":
        return scenes.one_cube_space(), two_cube_ui_space(), oracle.unaltered_colors(lighting=1, transparency=0), look((0.5, 0.5, 2.0), (0.5, 0.5, 1.0)), (0, 0, 0, 0)
    if name == "ui_over_world_antialiased":
        return scenes.one_cube_space(), scenes.ui_space(), oracle.unaltered_colors(antialiasing=2), look((0.5, 0.5, 2.0), (0.5, 0.5, 1.0)), (0, 0, 0, 0)
    if name == "no_world":
        return None, two_cube_ui_space(), oracle.unaltered_colors(transparency=0), look((0.5, 0.5, 2.0), (0.5, 0.5, 1.0)), (0, 0, 0, 0)
    if name == "backdrop":
        return scenes.one_cube_space(), scenes.ui_space(), oracle.unaltered_colors(lighting=1), look((0.5, 0.5, 2.0), (0.5, 0.5, 1.0)), (0.2, 0.4, 0.6, 0.5)
    raise KeyError(name)


CASES = ["one_red_cube", "partial_voxels", "half_transparent_slab", "antialias", "ui_over_world", "ui_over_world_antialiased", "no_world", "backdrop"]


def cameras(name):
    _, ui, opt, (eye, quat), _ = case(name)
    _, _, inv = oracle.camera_matrices(90.0, opt.view_distance, W / HT, quat, eye)
    ui_inv = None
    if ui is not None:
        _, _, ui_inv = oracle.camera_matrices(90.0, opt.view_distance, W / HT, (0, 0, 0, 1), (0, 0, 0))
    return inv, ui_inv


def load(ctx, name, flags=0, partition=None, tuning=0):
    """Uploads the case and returns its frame."""
    world, ui, opt, _, backdrop = case(name)
    inv, ui_inv = cameras(name)
    if world is not None:
        ctx.upload_space(abi.LAYER_WORLD, world)
    else:
        ctx.clear_space(abi.LAYER_WORLD)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    if ui is not None:
        ctx.upload_space(abi.LAYER_UI, ui)
        ctx.set_options(abi.LAYER_UI, to_abi_options(opt))
    else:
        ctx.clear_space(abi.LAYER_UI)
    return ctx.make_frame(W, HT, world_inv=inv, ui_inv=ui_inv, exposure=WORLD_EXPOSURE, ui_exposure=UI_EXPOSURE, backdrop=backdrop, flags=flags,
                          partition=partition, tuning=tuning)


@functools.lru_cache(maxsize=None)
def expected_split(name: str):
    """(depth [HT, W] f64 before the transform, layer [HT, W]: +1 world, -1 UI, first_sample_depth [HT, W]) from the oracle, computed once per case."""
    world, ui, opt, _, backdrop = case(name)
    inv, ui_inv = cameras(name)
    return split_of(world, ui, opt, inv, ui_inv, backdrop, W, HT)


def split_of(world, ui, opt, inv, ui_inv, backdrop, width, height):
    """expected_split of any scene, cameras and frame size (tests/test_present_goldens_cpu.py and tests/test_gpu_present_goldens.py use it too)."""
    wsp = oracle.Space(world) if world is not None else None
    usp = oracle.Space(ui) if ui is not None else None
    points = SAMPLE_POINTS if opt.antialiasing == 2 else [(0.5, 0.5)]
    has_backdrop = any(v != 0 for v in backdrop)
    depth = np.full((height, width), np.inf)
    first = np.full((height, width), np.inf)
    layer = np.zeros((height, width), np.int8)
    for y in range(height):
        y0, y1 = -(y / height * 2.0 - 1.0), -((y + 1) / height * 2.0 - 1.0)
        for x in range(width):
            x0, x1 = x / width * 2.0 - 1.0, (x + 1) / width * 2.0 - 1.0
            for i, (ux, uy) in enumerate(points):
                if len(points) == 4:
                    px, py = x0 + (x1 - x0) * ux, y0 + (y1 - y0) * uy  # point_within_patch
                else:
                    px, py = (x0 + x1) / 2.0, (y0 + y1) / 2.0  # Box2D::center
                d, t, lay = np.inf, np.float32(1.0), 0
                if usp is not None:
                    _, cb, du = oracle.trace_ray(usp, opt, *oracle.project_ndc_into_world(ui_inv, px, py), include_sky=False)
                    d, t = min(d, du), np.float32(cb[3])
                    if t != 1.0:
                        lay = -1
                if has_backdrop:
                    t = np.float32(t * np.float32(np.float32(1.0) - np.float32(backdrop[3])))
                    if lay == 0 and t != 1.0:
                        lay = -1
                if wsp is not None:
                    if not t < np.float32(1.0 / 256.0):
                        _, _, dw = oracle.trace_ray(wsp, opt, *oracle.project_ndc_into_world(inv, px, py), include_sky=True)
                        d = min(d, dw)
                    if lay == 0:
                        lay = 1  # a surface of the world, or its sky: the sample ends opaque
                elif not t < np.float32(1.0 / 256.0):
                    d, lay = np.inf, 1  # painted NO_WORLD_TO_SHOW: the sample is replaced
                depth[y, x] = min(depth[y, x], d)
                if i == 0:
                    first[y, x] = d
                if layer[y, x] == 0:
                    layer[y, x] = lay
    return depth, layer, first


def expected_planes(name, colorbuf, zw, rows=slice(None)):
    depth, layer, _ = expected_split(name)
    return planes_of(depth[rows], layer[rows], colorbuf, zw, WORLD_EXPOSURE, UI_EXPOSURE)


def planes_of(depth, layer, colorbuf, zw, world_exposure, ui_exposure):
    """expected_planes from split_of's depth and layer: (colour plane f16, depth plane f32)."""
    e = np.where(layer == -1, np.float32(ui_exposure), np.where(layer == 1, np.float32(world_exposure), np.float32(1.0))).astype(np.float32)
    cb = colorbuf.astype(np.float32)
    color = np.empty(cb.shape, np.float32)
    color[..., :3] = cb[..., :3] * e[..., None]
    color[..., 3] = np.clip(np.float32(1.0) - cb[..., 3], np.float32(0.0), np.float32(1.0))
    with np.errstate(over="ignore"):
        color_f16 = color.astype(np.float16)
    zw = np.asarray(zw, np.float64)
    d = np.clip(depth, 0.0, 1.0)
    z = ((0.0 * 0.0 + 0.0 * 0.0) + d * zw[0]) + zw[1]
    w = ((0.0 * 0.0 + 0.0 * 0.0) + d * zw[2]) + zw[3]
    value = (z / w).astype(np.float32) * np.where(layer == 1, np.float32(1.0), np.float32(-1.0)).astype(np.float32)
    return color_f16, value


def assert_planes(got, want_color, want_depth, what=""):
    gc, gd = got["color_f16"], got["depth"]
    assert gc.dtype == np.float16 and gd.dtype == np.float32 and gc.shape == want_color.shape and gd.shape == want_depth.shape
    bad_d = gd.view(np.uint32) != want_depth.view(np.uint32)
    assert not bad_d.any(), f"{what} depth plane: {int(bad_d.sum())} pixels differ, first {np.argwhere(bad_d)[:4].tolist()}: got {gd[bad_d][:4]}, want {want_depth[bad_d][:4]}"
    bad_c = gc.view(np.uint16) != want_color.view(np.uint16)
    assert not bad_c.any(), f"{what} colour plane: {int(bad_c.sum())} values differ, first {np.argwhere(bad_c)[:4].tolist()}: got {gc[bad_c][:4]}, want {want_color[bad_c][:4]}"


def render_planes(ctx, name, zw, **frame_kw):
    frame = load(ctx, name, **frame_kw)
    keep = frame.flags
    frame.flags = keep | abi.FRAME_OUT_COLORBUF
    colorbuf = ctx.render(frame)["rgba8"]
    frame.flags = keep | abi.FRAME_OUT_SPLIT
    ctx.set_depth_transform(zw)
    try:
        got = ctx.render(frame)
    finally:
        ctx.set_depth_transform(ZW_DEFAULT)
    return frame, colorbuf, got


@pytest.mark.parametrize("zw_kind", ["default", "mirror"])
@pytest.mark.parametrize("name", CASES)
def test_split_planes_equal_the_oracle(ctx, name, zw_kind):
    zw = ZW_DEFAULT if zw_kind == "default" else mirror_zw()
    _, colorbuf, got = render_planes(ctx, name, zw)
    assert got["info"].variant == abi.VARIANT_RECORDING and got["info"].rows_rendered == HT
    want_color, want_depth = expected_planes(name, colorbuf, zw)
    assert_planes(got, want_color, want_depth, name)


def test_cases_show_what_they_are_for():
    """The oracle's expected values themselves: each case exercises what the table of cases asks it to."""
    # a transparent first surface decides the depth: the slab's pixels are nearer than anything opaque behind them (there is nothing but sky)
    depth, layer, _ = expected_split("half_transparent_slab")
    assert np.isfinite(depth).any() and np.isinf(depth).any() and (layer == 1).all()
    # antialiasing: the minimum over the samples is not always the first sample's depth
    depth, _, first = expected_split("antialias")
    assert (depth < first).any()
    # UI over a world: negative depths exactly on the UI pixels, which exist, and so do world pixels
    depth, layer, _ = expected_split("ui_over_world")
    assert (layer == -1).any() and (layer == 1).any()
    _, value = expected_planes("ui_over_world", np.zeros((HT, W, 4), np.float32), ZW_DEFAULT)
    assert (np.signbit(value) == (layer == -1)).all()
    # no world: the paint's layer is the world's, its depth the far end -- except where the opaque UI cube covers the pixel
    depth, layer, _ = expected_split("no_world")
    assert (layer == 1).any() and (layer == -1).any() and np.isinf(depth[layer == 1]).all() and np.isfinite(depth[layer == -1]).all()
    _, value = expected_planes("no_world", np.zeros((HT, W, 4), np.float32), ZW_DEFAULT)
    assert (value[layer == 1] == 1.0).all()
    # a backdrop of alpha 0.5 makes every pixel a UI pixel
    assert (expected_split("backdrop")[1] == -1).all()


def test_exposures_follow_the_layer(ctx):
    """The UI exposure (2.0) on the UI pixels, the world's (0.5) on the world pixels, and negative depths exactly on the UI pixels."""
    _, colorbuf, got = render_planes(ctx, "ui_over_world", ZW_DEFAULT)
    _, layer, _ = expected_split("ui_over_world")
    assert (np.signbit(got["depth"]) == (layer == -1)).all()
    light = colorbuf[..., :3].max(axis=-1)
    peak = got["color_f16"][..., :3].astype(np.float32).max(axis=-1)
    for which, exposure in ((-1, UI_EXPOSURE), (1, WORLD_EXPOSURE)):
        sel = (light > 0) & (layer == which)
        assert sel.any()
        assert (peak[sel] == (light[sel] * np.float32(exposure)).astype(np.float16).astype(np.float32)).all()


@pytest.mark.parametrize("name", ["ui_over_world", "antialias"])
def test_partition_parts_equal_the_whole_frames_rows(ctx, name):
    zw = mirror_zw()
    _, _, whole = render_planes(ctx, name, zw)
    seen = np.zeros(HT, bool)
    for part in (0, 1):
        _, colorbuf, got = render_planes(ctx, name, zw, partition=(8, 2, part))
        rows = np.array([y for y in range(HT) if (y // 8) % 2 == part])
        assert got["info"].rows_rendered == len(rows)
        assert_planes(got, whole["color_f16"][rows], whole["depth"][rows], f"{name} part {part}")
        want_color, want_depth = expected_planes(name, colorbuf, zw, rows)
        assert_planes(got, want_color, want_depth, f"{name} part {part} (oracle)")
        seen[rows] = True
    assert seen.all()


def test_same_bytes_through_every_entry_point(ctx):
    import torch

    name = "ui_over_world"
    zw = mirror_zw()
    frame, _, want = render_planes(ctx, name, zw)
    want_raw = np.concatenate([want["color_f16"].reshape(-1).view(np.uint8), want["depth"].reshape(-1).view(np.uint8)])
    n_bytes = W * HT * 12
    ctx.set_depth_transform(zw)
    try:
        bufs = [torch.zeros(n_bytes, dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        # aic_render to device memory
        info = ctx.render_to_device(frame, bufs[0].data_ptr())
        assert info.variant == abi.VARIANT_RECORDING
        assert (bufs[0].cpu().numpy() == want_raw).all(), "aic_render to the device"
        # aic_render_submit / _wait on slots 0 and 1, with counters / no feedback / a variant request mixed in: nothing changes the bytes
        variants = [(0, 0), (abi.FRAME_COUNTERS | abi.FRAME_NO_FEEDBACK, abi.tuning(variant=abi.VARIANT_EXCHANGING))]
        for slot, (extra, tune) in enumerate(variants):
            f = load(ctx, name, flags=abi.FRAME_OUT_SPLIT | extra, tuning=tune)
            ctx.render_submit(f, bufs[1 + slot].data_ptr(), slot)
        for slot in (0, 1):
            info = ctx.render_wait(slot)
            assert info.variant == abi.VARIANT_RECORDING and info.rows_rendered == HT
            ctx.synchronize()
            got = abi.split_planes(bufs[1 + slot].cpu().numpy(), HT, W)
            assert_planes(got, want["color_f16"], want["depth"], f"submit on slot {slot}")
        # the host path with a variant request and AIC_FRAME_AUX
        f = load(ctx, name, flags=abi.FRAME_OUT_SPLIT, tuning=abi.tuning(variant=abi.VARIANT_PLAIN))
        got = ctx.render(f, want_aux=True)
        assert_planes(got, want["color_f16"], want["depth"], "aic_render with aux and a variant request")
        assert got["aux"] is not None and got["aux"].shape == (HT, W)
        # aic_render_submit_batch with two cameras: each frame equals the frame rendered alone
        world, _, opt, (eye, quat), _ = case(name)
        eye2 = (eye[0] + 0.3, eye[1] + 0.2, eye[2])
        _, _, inv2 = oracle.camera_matrices(90.0, opt.view_distance, W / HT, quat, eye2)
        f1 = load(ctx, name, flags=abi.FRAME_OUT_SPLIT)
        f2 = load(ctx, name, flags=abi.FRAME_OUT_SPLIT)
        f2.world.inverse_projection_view[:] = [float(v) for v in np.asarray(inv2).reshape(16)]
        alone2 = ctx.render(f2)
        assert (alone2["depth"].view(np.uint32) != want["depth"].view(np.uint32)).any(), "the second camera sees another picture"
        for b in bufs[:2]:
            b.zero_()
        torch.cuda.synchronize()
        ctx.render_submit_batch([f1, f2], [bufs[0].data_ptr(), bufs[1].data_ptr()], 1)
        infos = ctx.render_wait_batch(1, 2)
        ctx.synchronize()
        assert all(i.variant == abi.VARIANT_RECORDING for i in infos)
        assert_planes(abi.split_planes(bufs[0].cpu().numpy(), HT, W), want["color_f16"], want["depth"], "batch frame 0")
        assert_planes(abi.split_planes(bufs[1].cpu().numpy(), HT, W), alone2["color_f16"], alone2["depth"], "batch frame 1")
    finally:
        ctx.set_depth_transform(ZW_DEFAULT)


def test_rejections_leave_the_context_usable(ctx):
    name = "ui_over_world"
    plain = load(ctx, name)
    before = ctx.render(plain)["rgba8"].copy()

    def unchanged():
        assert (ctx.render(plain)["rgba8"] == before).all()

    for other in (abi.FRAME_OUT_LINEAR, abi.FRAME_OUT_COLORBUF, abi.FRAME_BLOOM):
        f = load(ctx, name, flags=abi.FRAME_OUT_SPLIT | other)
        with pytest.raises(abi.AicError) as err:
            ctx.render(f)
        assert err.value.code == 1, other  # AIC_ERR_INVALID
        unchanged()
    f = load(ctx, name, flags=abi.FRAME_OUT_SPLIT)
    with pytest.raises(abi.AicError) as err:
        ctx.trace_patches(f, [[-0.5, -0.5, 0.5, 0.5]])
    assert err.value.code == 5  # AIC_ERR_UNSUPPORTED
    unchanged()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(abi.AicError) as err:
            ctx.set_depth_transform((1.0, 0.0, bad, 1.0))
        assert err.value.code == 1
        unchanged()
    # the transform a rejected call named was not taken: the plane is still the linear depth
    _, colorbuf, got = render_planes(ctx, name, ZW_DEFAULT)
    assert_planes(got, *expected_planes(name, colorbuf, ZW_DEFAULT), "after the rejections")


def test_multi_device_renders_reject_the_flag():
    world, _, opt, _, _ = case("one_red_cube")
    inv, _ = cameras("one_red_cube")
    with abi.MultiContext([0]) as m:
        m.upload_space(abi.LAYER_WORLD, world)
        m.set_options(abi.LAYER_WORLD, to_abi_options(opt))
        m.set_depth_transform(mirror_zw())  # (replicated on every device; a NaN is rejected there too)
        with pytest.raises(abi.AicError) as err:
            m.set_depth_transform((float("nan"), 0.0, 0.0, 1.0))
        assert err.value.code == 1
        plain = abi.Context.make_frame(W, HT, world_inv=inv)
        before = m.render(plain)["rgba8"].copy()
        flagged = abi.Context.make_frame(W, HT, world_inv=inv, flags=abi.FRAME_OUT_SPLIT)
        with pytest.raises(abi.AicError) as err:
            m.render(flagged)
        assert err.value.code == 5  # AIC_ERR_UNSUPPORTED
        assert (m.render(plain)["rgba8"] == before).all()


def test_frames_without_the_flag_are_unchanged(ctx):
    name = "ui_over_world_antialiased"
    plain = load(ctx, name)
    counted = load(ctx, name, flags=abi.FRAME_COUNTERS)
    before = ctx.render(plain)
    before_counted = ctx.render(counted, want_aux=True)
    render_planes(ctx, name, mirror_zw())
    after = ctx.render(plain)
    after_counted = ctx.render(counted, want_aux=True)
    assert (after["rgba8"] == before["rgba8"]).all() and after["info"].cubes_traced == before["info"].cubes_traced
    assert (after_counted["rgba8"] == before_counted["rgba8"]).all() and (after_counted["aux"] == before_counted["aux"]).all()
    for k in ("cubes_traced", "n_outer", "n_inner", "n_hits", "n_light"):
        assert getattr(after_counted["info"], k) == getattr(before_counted["info"], k), k
    assert (before["rgba8"] == before_counted["rgba8"]).all()


def test_host_mirror_draw_split(ctx):
    """HipRtRenderer::draw_split sets the world camera's depth transform and renders with the flag: the bytes of the ABI called by hand."""
    import all_is_cubes_amd as A

    eye, target = (0.7, 0.9, 2.5), (0.5, 0.5, 0.5)
    world = scenes.one_cube_space()
    cams = H.StandardCameras()
    cams.graphics_options = H.GraphicsOptions()
    cams.viewport = H.Viewport.with_scale(1.0, W, HT)
    cams.world_space = A.space_from_flat(world)
    cams.world_view_transform = H.look_at_y_up(eye, target)
    r = H.HipRtRenderer(cams)
    r.update()
    got = r.draw_split()
    assert (got.width, got.height) == (W, HT)
    opt = oracle.make_options()
    _, _, inv = oracle.camera_matrices(90.0, 200.0, W / HT, oracle.look_at_y_up(eye, target), eye)
    ctx.upload_space(abi.LAYER_WORLD, world)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    ctx.clear_space(abi.LAYER_UI)
    ctx.set_depth_transform(mirror_zw(200.0))
    try:
        want = ctx.render(ctx.make_frame(W, HT, world_inv=inv, flags=abi.FRAME_OUT_SPLIT))
    finally:
        ctx.set_depth_transform(ZW_DEFAULT)
    assert_planes({"color_f16": got.color_f16_bits.view(np.float16), "depth": got.depth}, want["color_f16"], want["depth"], "draw_split")
    assert (want["depth"] > 0).all() and (want["depth"] < 1).any()  # world pixels; the cube is nearer than the far plane
