"""GPU tests (-m gpu): the Split presentation path -- AIC_FRAME_OUT_SPLIT frames through aic_present_split, aic_present_split_lines and
aic_present_split_text, by the C ABI and by the host mirror's draw_split, project_cursor, present_split_lines and present_split_text -- held end to end
to the reference's golden images. The kernels equal tests/present_ref.py, tests/present_lines_ref.py and tests/present_text_ref.py bit for bit elsewhere;
those are this project's reading of the reference's shaders, and tests/test_present_goldens_cpu.py holds that reading to the goldens. Here the device's
own traced frames, the cursor record, the wireframe, the depth transform and the matrix handed to the lines meet the same images.

Cases, bounds and restated frames are tests/present_golden_cases.py's, computed once. Every frame is at most 256 x 320."""
import numpy as np
import pytest

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import present_golden_cases as G
from tests import present_lines_ref, present_ref, scenes
from tests.test_gpu_cursor import assert_cursor_is
from tests.test_gpu_parity import to_abi_options
from tests.test_gpu_reproject import GUARD, SENTINEL, device_bytes, planes_of, split_bytes, to_device
from tests.test_gpu_split import assert_planes
from tests.test_info_text import INFO_TEXT
from tests.test_oracle_goldens import COMMON_VIEWPORT
from tests.test_oracle_light import image_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def trace_split(ctx, size, world_inv, ui_inv=None, exposure=1.0):
    """One AIC_FRAME_OUT_SPLIT frame traced into device memory: (the resident frame, its colour plane u16, its depth plane u32)."""
    w, h = size
    n = w * h
    resident = device_bytes(n * 12 + GUARD)
    frame = ctx.make_frame(w, h, world_inv=world_inv, ui_inv=ui_inv, exposure=exposure, ui_exposure=exposure, flags=abi.FRAME_OUT_SPLIT)
    info = ctx.render_to_device(frame, resident.data_ptr())
    ctx.synchronize()
    raw = resident.cpu().numpy()
    assert info.rows_rendered == h and (raw[n * 12:] == SENTINEL).all(), "guard bytes behind the frame"
    return (resident,) + planes_of(raw, w, h)


# ---- the cursor ----------------------------------------------------------------------------------------------------------

def test_cursor_basic_through_the_host_mirror(golden_dir):
    """cases/src/lib.rs:255-284 as an interactive frame: update(), project_cursor(0, 0), update(cursor), draw_split(), present_split_lines. The lines'
    depth comes from one matrix and the frame's depth plane from the trace under aic_set_depth_transform; the reference's image decides which line
    pixels survive. Without the cursor the same presentation misses the bound."""
    import all_is_cubes_amd as A

    want = G.cursor_restated()
    w, h = COMMON_VIEWPORT
    o = G.cursor_options()
    assert o.bloom_intensity == 0.0
    cams = H.StandardCameras()
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(scenes.one_cube_space())
    cams.world_view_transform = H.look_at_y_up(G.EYE, G.TARGET)
    r = H.HipRtRenderer(cams)
    r.update()
    cursor = r.project_cursor(0.0, 0.0)
    assert cursor is not None, "project_cursor() unexpectedly missed"
    assert_cursor_is(cursor, want["record"])
    assert (cursor.wireframe() == want["lines"]).all()
    r.update(cursor)
    frame = r.draw_split()
    assert (frame.width, frame.height) == (w, h)
    assert_planes({"color_f16": frame.color_f16_bits.view(np.float16), "depth": frame.depth}, want["color"].view(np.float16), want["depth"].view(np.float32), "draw_split")
    assert (G.view_projection_of(r.world_camera()) == want["m"]).all()
    resident = to_device(split_bytes(frame))
    shown, counts = r.present_split_lines(resident.data_ptr(), w, h)
    figures = G.cursor_figures(golden_dir, shown.data, want["plain"])
    print("cursor_basic-all, device:", counts, figures)
    assert (shown.width, shown.height) == (w, h)
    # the restatement of the device's own planes (which are the oracle's, asserted above)
    restated, restated_counts = present_lines_ref.present(frame.color_f16_bits, frame.depth.view(np.uint32), (w, h), cursor.wireframe(), G.view_projection_of(r.world_camera()),
                                                          0.0, int(o.tone_mapping), o.maximum_intensity)
    assert (shown.data == restated).all() and counts == restated_counts
    assert (shown.data == want["image"]).all() and counts == want["counts"]
    assert image_diff(golden_dir, "cursor_basic-all", shown.data).max() <= 1
    # no cursor: nothing drawn, and the golden is missed
    r.update()
    plain, no_counts = r.present_split_lines(resident.data_ptr(), w, h)
    assert no_counts == dict.fromkeys(present_lines_ref.COUNTS, 0) and (plain.data == want["plain"]).all()
    assert image_diff(golden_dir, "cursor_basic-all", plain.data).max() > 1


# ---- the info text -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("half", [False, True], ids=["full-size frame", "half-size frame"])
@pytest.mark.parametrize("scale,name", G.TEXT_SCALES)
def test_info_text_end_to_end(ctx, golden_dir, scale, name, half):
    """cases/src/lib.rs:667-711 through the Split path: the orange sky traced as a Split frame at the window's size or half of it, shown with INFO_TEXT
    in windows of 1, 1.5 and 2 times the nominal 128 x 96 -- by the host mirror (draw_split, present_split_text; its viewport's nominal size makes the
    grid) and by the C ABI (aic_text_geometry, aic_text_layout, aic_set_text_font, aic_present_split_text). Both equal the restatement bit for bit and
    meet the golden as the restatement does; without the text the golden is missed."""
    import all_is_cubes_amd as A

    w, h = G.text_window(scale)
    sw, sh = G.text_source_size(scale, half)
    sp = G.orange_space()
    # the host mirror; a size policy halves the traced frame and leaves the nominal size alone
    cams = H.StandardCameras()
    o = H.GraphicsOptions.unaltered_colors()
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(scale, w, h)
    cams.world_space = A.space_from_flat(sp)
    cams.world_view_transform = H.look_at_y_up(G.EYE, G.TARGET)
    policy = (lambda vp: H.Viewport.with_scale(sw / G.NOMINAL[0], sw, sh)) if half else None
    r = H.HipRtRenderer(cams, policy)
    r.update()
    vp = r.world_camera().viewport()
    assert (vp.nominal_width, vp.nominal_height) == G.NOMINAL and (vp.framebuffer_width, vp.framebuffer_height) == (sw, sh)
    frame = r.draw_split()
    assert (frame.width, frame.height) == (sw, sh)
    assert (frame.color_f16_bits == np.array([*G.ORANGE, 1.0], np.float16).view(np.uint16)).all()
    want = G.text_restated(frame.color_f16_bits, scale)
    resident = to_device(split_bytes(frame))
    shown, _ = r.present_split_text(resident.data_ptr(), w, h, INFO_TEXT)
    assert (shown.width, shown.height) == (w, h) and (shown.data == want).all(), "host mirror"
    exact = G.assert_text_golden(golden_dir, name, shown.data)
    print(f"{name} from {sw}x{sh}: {exact} pixels differ exactly")
    bare = r.present_split(resident.data_ptr(), w, h)
    assert (bare.data == (255, 188, 0, 255)).all() and image_diff(golden_dir, name, bare.data).max() > 100
    # the C ABI, frame traced by aic_render into device memory
    ctx.upload_space(abi.LAYER_WORLD, sp)
    ctx.clear_space(abi.LAYER_UI)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(oracle.unaltered_colors()))
    inv = oracle.camera_matrices(90.0, 200.0, sw / sh, oracle.look_at_y_up(G.EYE, G.TARGET), G.EYE)[2]
    traced, color, _ = trace_split(ctx, (sw, sh), inv)
    assert (color == frame.color_f16_bits).all()
    cell = H.INFO_TEXT_CELL
    ctx.set_text_font(H.info_text_font_atlas(), *cell)
    cols, rows, text_scale, origin = abi.text_geometry(G.NOMINAL, cell)
    codes, _ = abi.text_layout(INFO_TEXT, cols, rows)
    image, _, _ = ctx.present_split_text(traced.data_ptr(), (sw, sh), (w, h), 0.0, int(o.tone_mapping), o.maximum_intensity, text=(codes, text_scale, origin))
    assert (image == want).all(), "C ABI"
    G.assert_text_golden(golden_dir, name, image)


# ---- colour through the f16 plane -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(G.COLOR_CASES))
def test_colour_cases(ctx, golden_dir, name):
    """Each golden the RGBA8 path meets, met by the Split path: traced with AIC_FRAME_OUT_SPLIT on the device with the case's exposure in the frame,
    shown at equal size with bloom 0 and the case's tone map. (a) the bound of the golden's RGBA8 test; (b) the oracle's RGBA8 within the one level an
    f16 store can tip, on every pixel that ends opaque there (tests/present_golden_cases.py: assert_color_bounds). The layers_* cases carry the UI
    layer through the frame: its pixels' depths are negative. Cases left out because the oracle's frame does not end opaque everywhere: none."""
    assert G.opaque_everywhere(name), name
    c = G.color_case(name)
    opt = c["opt"]
    ctx.upload_space(abi.LAYER_WORLD, c["space"])
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    if c["ui"] is not None:
        ctx.upload_space(abi.LAYER_UI, c["ui"])
        ctx.set_options(abi.LAYER_UI, to_abi_options(opt))
    else:
        ctx.clear_space(abi.LAYER_UI)
    resident, color, depth = trace_split(ctx, c["size"], c["inv"], c["ui_inv"], exposure=c["exposure"])
    image, info = ctx.present_split(resident.data_ptr(), c["size"], c["size"], 0.0, opt.tone_mapping, opt.maximum_intensity)
    assert info.bloomed == 0
    assert (image == present_ref.present(color, c["size"], 0.0, opt.tone_mapping, opt.maximum_intensity)).all(), "the device against the restatement of its own frame"
    at = G.assert_color_bounds(golden_dir, name, image, "device")
    print(f"{name}: pixels at each level from the oracle's RGBA8 {at}, from the golden {G.golden_levels(golden_dir, name, image)}")
    ui_pixels = np.signbit(depth.view(np.float32))
    assert ui_pixels.any() == (c["ui"] is not None) and not ui_pixels.all()


# ---- bloom through the presentation ---------------------------------------------------------------------------------------

def test_bloom_through_the_presentation(ctx, golden_dir):
    """cases/src/lib.rs:186-201: the bloom scene's device-traced Split frame with its colour plane clamped to [0, 1] on the host (why:
    tests/test_bloom_cpu.py::test_golden_bloom_025) and uploaded again; aic_present_split at intensity 0.25 meets bloom-0.25-all at the case's
    threshold, 12, and at intensity 0 -- clamped or not -- the bound bloom-0.0-all has for the RGBA8 path."""
    size = (128, 256)
    w, h = size
    eye = (1.5, 3.0, 8.0)
    opt = oracle.unaltered_colors(lighting=3)
    ctx.upload_space(abi.LAYER_WORLD, scenes.bloom_test_space())
    ctx.clear_space(abi.LAYER_UI)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    inv = oracle.camera_matrices(45.0, opt.view_distance, w / h, oracle.look_at_y_up(eye, (1.5, 3.0, 7.0)), eye)[2]
    resident, color, depth = trace_split(ctx, size, inv)
    light = color.view(np.float16)
    assert light[..., :3].max() > 1.0  # the emissive green, 100, is in the frame
    clamped = light.copy()
    clamped[..., :3] = np.minimum(clamped[..., :3], np.float16(1.0))
    again = to_device(np.concatenate([clamped.view(np.uint8).reshape(-1), depth.view(np.uint8).reshape(-1)]))
    bloomed, info = ctx.present_split(again.data_ptr(), size, size, 0.25, opt.tone_mapping, opt.maximum_intensity)
    d = image_diff(golden_dir, "bloom-0.25-all", bloomed)
    print("bloom-0.25-all:", G.levels(d))
    assert info.bloomed == 1 and d.max() <= 12
    for what, frame in (("as traced", resident), ("clamped", again)):
        plain, info = ctx.present_split(frame.data_ptr(), size, size, 0.0, opt.tone_mapping, opt.maximum_intensity)
        d = image_diff(golden_dir, "bloom-0.0-all", plain)
        print(f"bloom-0.0-all, {what}:", G.levels(d))
        assert info.bloomed == 0 and d.max() <= 12, what
    assert image_diff(golden_dir, "bloom-0.25-all", plain).max() > 12  # the golden sees the bloom: the clamped frame without it misses
