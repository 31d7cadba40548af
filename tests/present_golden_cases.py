"""The reference's golden images that hold the Split presentation path (AIC_FRAME_OUT_SPLIT frames through aic_present_split, aic_present_split_lines and
aic_present_split_text): the scenes, cameras, bounds and restated images that tests/test_present_goldens_cpu.py checks on the host and
tests/test_gpu_present_goldens.py runs on the device. Nothing here needs a device; every oracle frame and restated image is computed once per process.

 * cursor_basic-all (cases/src/lib.rs:255-284): one_cube_space, UNALTERED_COLORS with Linear lighting, the cursor StandardCameras::project_cursor finds
   at NDC (0, 0), drawn by the line pass under the frame's own depth plane.
 * info_text-{1.0,1.5,2.0}-all (cases/src/lib.rs:667-711): an orange sky with the info text, at framebuffers of 1, 1.5 and 2 times the nominal 128 x 96.
 * the colour cases: goldens the RGBA8 path already meets, met again by the f16 colour plane shown at equal size without bloom.
"""
import functools

import numpy as np

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi, flat
from tests import cursor_ref, present_lines_ref, present_ref, present_text_ref, scenes
from tests.test_gpu_split import planes_of, split_of
from tests.test_info_text import INFO_TEXT
from tests.test_oracle_goldens import COMMON_VIEWPORT, diff_to, histogram_ok, neighbourhood_diff, with_info_text
from tests.test_oracle_light import image_diff, lit

F = np.float32
EYE, TARGET = (0.5, 0.5, 2.0), (0.5, 0.5, 0.0)  # StandardCameras::from_constant_for_test on one_cube_space: the camera of the no_update-2 test
NOMINAL = COMMON_VIEWPORT


def levels(d) -> dict:
    """{level: count of pixels} of a per-pixel difference, the levels that occur"""
    d = np.asarray(d)
    n = np.bincount((d.max(axis=-1) if d.ndim == 3 else d).astype(np.int64).ravel())
    return {int(k): int(n[k]) for k in np.flatnonzero(n)}


# ---- the cursor ----------------------------------------------------------------------------------------------------------

def cursor_options():
    o = H.GraphicsOptions.unaltered_colors()
    o.lighting_display = H.LightingOption(H.LightingKind.Linear, 0)
    return o


def cursor_camera():
    c = H.Camera(cursor_options(), H.Viewport.with_scale(1.0, *COMMON_VIEWPORT))
    c.set_view_transform(H.look_at_y_up(EYE, TARGET))
    return c


def view_projection_of(camera):
    """the host mirror's matrix: view then projection in f64, the sums in Mat4::then's order, rounded to f32; [c*4+r]"""
    v, p = camera.view_matrix().tolist(), camera.projection_matrix().tolist()
    return np.array([v[r][0] * p[0][c] + v[r][1] * p[1][c] + v[r][2] * p[2][c] + v[r][3] * p[3][c] for r in range(4) for c in range(4)], np.float64).astype(F)


def wireframe_of(rec):
    """aic_cursor_wireframe of a cursor_ref / aic_cursor_raycast record: [2 n, 7] f32"""
    v = abi.cursor_wireframe(rec["cube"], int(rec["face_entered"]), int(rec["face_selected"]), rec["point_entered"], float(rec["distance_to_point"]),
                             rec["voxel_lo"], rec["voxel_size"], int(rec["resolution"]))
    return np.ascontiguousarray(v).view(F).reshape(-1, 7)


@functools.lru_cache(maxsize=None)
def cursor_restated():
    """The cursor_basic frame with nothing from a device: the oracle's linear colour as f16 and its distances under the mirror camera's depth transform
    (tests/test_gpu_split.py's expected planes), cursor_ref's raycast of the ray at NDC (0, 0), the library's host-only wireframe, and the restated line
    pass. dict(color u16 bits, depth u32 bits, record, lines, m, image, counts, plain: the image without lines, owner: the line that owns each pixel)."""
    w, h = COMMON_VIEWPORT
    sp = scenes.one_cube_space()
    opt = oracle.unaltered_colors(lighting=3)
    camera = cursor_camera()
    inv = oracle.camera_matrices(90.0, opt.view_distance, w / h, oracle.look_at_y_up(EYE, TARGET), EYE)[2]
    assert (np.asarray(camera.inverse_projection_view(), np.float64).reshape(4, 4) == np.asarray(inv).reshape(4, 4)).all()
    lin = oracle.render(oracle.Space(sp), opt, oracle.make_camera(inv, w, h), threads=4, want_linear=True)["linear"]
    assert (lin[..., 3] == 1.0).all()
    colorbuf = np.concatenate([lin[..., :3], 1.0 - lin[..., 3:]], axis=-1).astype(F)
    depth, layer, _ = split_of(sp, None, opt, inv, None, (0, 0, 0, 0), w, h)
    color, plane = planes_of(depth, layer, colorbuf, camera.depth_transform_zw(), 1.0, 1.0)
    origin, direction = camera.project_ndc_into_world(0.0, 0.0)
    record = cursor_ref.Scene(sp).raycast(np.concatenate([origin, direction]).astype(np.float64), 6.0)  # stdcam.rs:357-389: the world within 6 cubes
    assert record["hit"] == 1
    lines = wireframe_of(record)
    m = view_projection_of(camera)
    o = cursor_options()
    parts, stats = {}, {}
    color_bits, depth_bits = color.view(np.uint16), np.ascontiguousarray(plane).view(np.uint32)
    parts["S"] = present_ref.scene(color_bits, w, h)
    parts["S'"], parts["counts"] = present_lines_ref.draw(parts["S"], depth_bits, lines, m, stats)
    image, counts = present_lines_ref.present(color_bits, depth_bits, (w, h), lines, m, 0.0, int(o.tone_mapping), o.maximum_intensity, parts=parts)
    plain = present_ref.composite(parts["S"], None, 0.0, int(o.tone_mapping), o.maximum_intensity)
    return {"space": sp, "color": color_bits, "depth": depth_bits, "record": record, "lines": lines, "m": m, "image": image, "counts": counts, "plain": plain,
            "owner": stats["owner"]}


def cursor_figures(golden_dir, image, plain):
    """What the issue's trial measured: the golden's line pixels (those 20 levels or more from the frame without lines), how many of them `image` draws
    a line on, the pixels that differ exactly, and the count of pixels at each level under the harness's comparison."""
    golden = np.load(golden_dir / "png_cursor_basic-all.npy")
    theirs = np.abs(golden.astype(int) - plain.astype(int)).max(axis=-1) >= 20
    ours = (image != plain).any(axis=-1)
    return {"golden line pixels": int(theirs.sum()), "our line pixels": int(ours.sum()), "shared": int((theirs & ours).sum()),
            "exact differences": int((image != golden).any(axis=-1).sum()), "levels": levels(image_diff(golden_dir, "cursor_basic-all", image))}


# ---- the info text -------------------------------------------------------------------------------------------------------

TEXT_SCALES = [(1.0, "info_text-1.0-all"), (1.5, "info_text-1.5-all"), (2.0, "info_text-2.0-all")]
ORANGE = (1.0, 0.5, 0.0)


def text_window(scale):
    return int(NOMINAL[0] * scale), int(NOMINAL[1] * scale)


def text_source_size(scale, half):
    w, h = text_window(scale)
    return (w // 2, h // 2) if half else (w, h)


def orange_space():
    sp = flat.FlatSpace((0, 0, 0), (1, 1, 1))
    sp.set_sky_uniform(ORANGE)
    sp.add_block(flat.air())
    return sp


def text_restated(color_bits, scale):
    """The restated presentation of a Split colour plane in the window of `scale` with INFO_TEXT over it: nominal size 128 x 96, the mirror's atlas."""
    w, h = text_window(scale)
    cell = H.INFO_TEXT_CELL
    cols, rows, text_scale, origin = present_text_ref.geometry(NOMINAL, cell)
    codes, _ = present_text_ref.layout(INFO_TEXT, cols, rows)
    layer = present_text_ref.text_layer(w, h, H.info_text_font_atlas(), cell, codes, text_scale, origin)
    o = H.GraphicsOptions.unaltered_colors()
    return present_text_ref.composite(present_ref.scene(color_bits, w, h), None, 0.0, int(o.tone_mapping), o.maximum_intensity, text=layer)


def assert_text_golden(golden_dir, name, image):
    """1.0 and 2.0 pixel for pixel; 1.5 -- every glyph texel one or two pixels wide -- with nothing left under the harness's comparison. Returns the
    count of pixels that differ exactly."""
    golden = np.load(golden_dir / f"png_{name}.npy")
    assert image.shape == golden.shape
    exact = int((image != golden).any(axis=-1).sum())
    if name == "info_text-1.5-all":
        d = image_diff(golden_dir, name, image)
        assert d.max() == 0, (name, levels(d))
    else:
        assert exact == 0, (name, exact)
    return exact


# ---- the colour cases ----------------------------------------------------------------------------------------------------

def _tone_map_bound(golden_dir, name, img):
    assert histogram_ok(image_diff(golden_dir, name, img), [(10, 100), (3, 500), (1, 1 << 60)]), name
    assert diff_to(golden_dir, name, img).max() <= 1, name


def _exact_bound(tol):
    def check(golden_dir, name, img):
        assert diff_to(golden_dir, name, img).max() <= tol, name
    return check


def _voxel_shape_bound(golden_dir, name, img):
    assert neighbourhood_diff(img, np.load(golden_dir / f"png_{name}.npy")).max() <= 1, name


def _slab_bound(golden_dir, name, img):
    assert image_diff(golden_dir, name, img).max() <= 7, name
    assert diff_to(golden_dir, name, img).max() <= 1, name  # (one of tests/test_oracle_light.py's EXACT goldens)


def _layers_bound(golden_dir, name, img):
    assert diff_to(golden_dir, name, with_info_text(img)).max() <= 1, name  # the "hello world" overlay of the case, drawn by the host as in the RGBA8 test


def _tone_map_eye():
    sp = lit(scenes.tone_mapping_space)
    return tuple(np.array(sp.lo, float) + np.array(sp.size, float) / 2.0 + np.array([0.0, 0.0, 65.0]))


def _case(space, opt, bound, size=COMMON_VIEWPORT, eye=EYE, look=(0.0, 0.0, -1.0), fov=90.0, exposure=1.0, ui=None):
    return {"space": space, "opt": opt, "bound": bound, "size": size, "eye": eye, "look": look, "fov": fov, "exposure": exposure, "ui": ui}


# name -> the scene builder, options and camera of the golden's RGBA8 test (tests/test_gpu_light.py, tests/test_gpu_parity.py) and that test's bound
COLOR_CASES = {
    **{name: (lambda tmo=tmo, mi=mi, e=e: _case(lit(scenes.tone_mapping_space), oracle.unaltered_colors(lighting=1, tone_mapping=tmo, maximum_intensity=mi), _tone_map_bound,
                                                   size=(256, 320), eye=_tone_map_eye(), fov=45.0, exposure=e))
       for name, tmo, mi, e in [("tone_map-Clamp-1.0-0.5-all", 0, 1.0, 0.5), ("tone_map-Clamp-1.0-2.0-all", 0, 1.0, 2.0), ("tone_map-Reinhard-0.5-0.5-all", 1, 0.5, 0.5),
                                ("tone_map-Reinhard-1.0-0.5-all", 1, 1.0, 0.5), ("tone_map-Reinhard-1.0-2.0-all", 1, 1.0, 2.0)]},
    "color_srgb_ramp-all": lambda: _case(scenes.color_srgb_ramp_space(), oracle.unaltered_colors(), _exact_bound(1), size=(128, 128), eye=(16.0, 16.0, 17.0)),
    "emission-all": lambda: _case(scenes.emission_space(), oracle.unaltered_colors(), _exact_bound(1)),
    **{f"emission_{kind}-{mode}-all": (lambda kind=kind, t=t: _case(scenes.voxel_shape_space(kind), oracle.unaltered_colors(transparency=t), _voxel_shape_bound))
       for kind in ("only", "semi") for mode, t in (("surf", 0), ("vol", 1))},
    "transparent_one-surf-all": lambda: _case(scenes.transparent_one_space(), oracle.unaltered_colors(transparency=0), _exact_bound(1)),
    "transparent_one-vol-all": lambda: _case(scenes.transparent_one_space(), oracle.unaltered_colors(transparency=1), _exact_bound(2)),
    "light_on_slab-Linear-all": lambda: _case(lit(scenes.light_on_slab_space), oracle.unaltered_colors(lighting=3), _slab_bound, eye=(0.5, -6.0, 6.0), look=(0.0, 1.0, -1.0), fov=45.0),
    "layers_all-all": lambda: _case(scenes.one_cube_space(), oracle.unaltered_colors(lighting=1), _layers_bound, ui=scenes.ui_space()),
    "layers_hidden_ui-all": lambda: _case(scenes.one_cube_space(), oracle.unaltered_colors(lighting=1), _layers_bound),
}


@functools.lru_cache(maxsize=None)
def color_case(name):
    """The case with its cameras and the oracle's frame: inv, ui_inv (None without a UI space), linear [h][w][4] f32 before exposure and tone map, rgba8."""
    c = COLOR_CASES[name]()
    w, h = c["size"]
    eye = c["eye"]
    quat = oracle.look_at_y_up(eye, tuple(e + l for e, l in zip(eye, c["look"])))
    opt = c["opt"]
    opt.exposure = c["exposure"]
    c["inv"] = oracle.camera_matrices(c["fov"], opt.view_distance, w / h, quat, eye)[2]
    c["ui_inv"] = oracle.camera_matrices(c["fov"], opt.view_distance, w / h, (0, 0, 0, 1), (0, 0, 0))[2] if c["ui"] is not None else None
    ui = c["ui"]
    ref = oracle.render(oracle.Space(c["space"]), opt, oracle.make_camera(c["inv"], w, h), ui=oracle.Space(ui) if ui is not None else None,
                        ui_opt=opt if ui is not None else None, ui_cam=oracle.make_camera(c["ui_inv"], w, h) if ui is not None else None, threads=4, want_linear=True)
    c["linear"], c["rgba8"] = ref["linear"], ref["rgba8"]
    return c


def opaque_everywhere(name) -> bool:
    """The presentation discards alpha: a case belongs here only if the oracle's frame ends opaque on every pixel."""
    c = color_case(name)
    return bool((c["rgba8"][..., 3] == 255).all() and (c["linear"][..., 3] == 1.0).all())


def color_plane_of(name):
    """The f16 colour plane of the oracle's frame: linear light times the case's exposure in f32, stored as f16 (bit patterns, alpha 1.0)."""
    c = color_case(name)
    plane = c["linear"].astype(F).copy()
    plane[..., :3] = plane[..., :3] * F(c["exposure"])
    with np.errstate(over="ignore"):
        return plane.astype(np.float16).view(np.uint16)


def assert_color_bounds(golden_dir, name, image, what):
    """(a) the golden at the bound of its RGBA8 test; (b) the oracle's RGBA8 within one level on every pixel that ends opaque there -- derived: an f16
    store moves linear light by 2^-11 relative at most, which the sRGB curve turns into less than 0.06 of a level, so it can only tip a rounding; Clamp
    and Reinhard have slope <= 1. Returns the count of pixels at each level of (b)."""
    c = color_case(name)
    assert image.shape == c["rgba8"].shape and (image[..., 3] == 255).all(), (what, name)
    c["bound"](golden_dir, name, image)
    opaque = c["rgba8"][..., 3] == 255
    d = np.abs(image[..., :3].astype(int) - c["rgba8"][..., :3].astype(int)).max(axis=-1)[opaque]
    assert d.max() <= 1, (what, name, levels(d))
    return levels(d)


def golden_levels(golden_dir, name, image) -> dict:
    """the figure beside the assertions: pixels at each level from the golden under the harness's comparison (the layers cases with their overlay)"""
    return levels(image_diff(golden_dir, name, with_info_text(image) if name.startswith("layers_") else image))


def present_color_restated(name):
    c = color_case(name)
    return present_ref.present(color_plane_of(name), c["size"], 0.0, c["opt"].tone_mapping, c["opt"].maximum_intensity)
