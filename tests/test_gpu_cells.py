"""The terminal's character cells on the device (run with -m gpu on an MI355X): aic_image_cells and aic_render_cells against the restatement
(tests/cells_ref.py), cell for cell and all three words, the resident frame's terminal target and the host mirror's byte stream."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import cells_ref as ref
from tests import scenes
from tests.test_gpu_parity import to_abi_options
from tests.test_gpu_reproject import GUARD, SENTINEL, device_bytes, split_bytes, to_device

pytestmark = pytest.mark.gpu

F = np.float32
MODE_PAIRS = list(itertools.product(ref.CHARACTER_MODES, ref.COLOR_MODES))
KNOWN = {ref.SHADES: [("r", "  ░░▒▒▓▓██")], ref.SPLIT: [("rr", "  ***▄▀███")], ref.SHAPES: [("rr", "  ░░▒▒▓▓██"), ("br", "   ▁▁▂▂▃▃▄")]}


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def assert_cells(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for word in ("glyph", "fg", "bg"):
        bad = np.argwhere(got[word] != want[word])
        if len(bad):
            p = tuple(bad[0])
            raise AssertionError(f"{what}: {len(bad)} cells differ in {word}; first at {p}: got {int(got[word][p]):#x} want {int(want[word][p]):#x}")


def ramp_inputs(characters):
    """The reference's ramps as 10 x 1 cells of this mode: (image, aux with every pixel a block hit, expected row or None)."""
    rx, ry = ref.RAYS[characters]
    out = []
    for rows_of, want in KNOWN.get(characters, [("r" * ry, None)]):
        image = np.repeat(ref.ramp_image(rows_of if len(rows_of) == ry else "r" * ry), rx, axis=1)
        aux = np.zeros(image.shape[:2], abi.PIXEL_AUX_DTYPE)
        aux["hit"] = 1
        out.append((image, aux, want))
    return out


def first_patch(image, aux, characters):
    rx, ry = ref.RAYS[characters]
    return image[:ry, :rx].copy(), aux[:ry, :rx].copy()


@pytest.mark.parametrize("characters, colors", MODE_PAIRS)
def test_image_cells_equal_the_restatement(ctx, characters, colors):
    """The four known-answer ramps and the edge images, in every mode pair: image on the host and on the device, f32 and f16, cells to the host and to
    the device; 7 x 5 cells (both checkerboard parities, Braille 14 x 20 pixels), 10 x 1 and 1 x 1."""
    cases = [(img, aux, 10, 1, {}, want) for img, aux, want in ramp_inputs(characters)]
    edges = ref.edge_images(characters)
    cases += [(img, aux, 7, 5, ref.EDGE_POST, None) for img, aux in edges]
    cases.append((*first_patch(*edges[0], characters), 1, 1, ref.EDGE_POST, None))
    cases.append((*first_patch(*edges[-1], characters), 0, 0, ref.EDGE_POST, None))  # a grid of 0 x 0 is raised to 1 x 1
    total = dict.fromkeys(ref.COUNTERS, 0)
    for k, (img, aux, cols, rows, post, known) in enumerate(cases):
        for f16 in (False, True):
            image = np.ascontiguousarray(img.astype(np.float16)) if f16 else img
            want, counters = ref.cells(image.astype(F), aux, cols, rows, characters, colors, **post)
            if known is not None and colors == ref.COLOR_NONE and not f16:
                assert ref.glyph_text(want[0]) == known
            dev_image, dev_aux = to_device(image), to_device(aux)
            dev_out = device_bytes(want.size * 12 + GUARD)
            for on_device, out_device in itertools.product((False, True), (False, True)):
                what = f"case {k} ({cols} x {rows}) f16 {f16} image on device {on_device} out on device {out_device}"
                got, info = ctx.image_cells(dev_image.data_ptr() if on_device else image, dev_aux.data_ptr() if on_device else aux, cols, rows, characters, colors,
                                            f16=f16, image_device=on_device, out_device=dev_out.data_ptr() if out_device else None, **post)
                if out_device:
                    raw = dev_out.cpu().numpy()
                    assert (raw[want.size * 12:] == SENTINEL).all(), "bytes behind the cells"
                    got = raw[:want.size * 12].view(abi.CELL_DTYPE).reshape(want.shape)
                assert_cells(got, want, what)
                assert info.n_cells == want.size and info.counters() == counters, (what, info.counters(), counters)
            if not f16:
                for name, v in counters.items():
                    total[name] += v
    assert all(total[name] > 0 for name in ref.expected_counters(characters, colors)), total


@pytest.mark.parametrize("characters", [c for c in ref.CHARACTER_MODES if c != ref.NAMES])
def test_image_cells_without_records_and_postprocessed(ctx, characters):
    """aux NULL: Split without colours shows ' ' where it would have shown the text; AIC_CELLS_POSTPROCESSED skips post_process_color."""
    for colors in ref.COLOR_MODES:
        for img, aux in ref.edge_images(characters)[:2]:
            want, counters = ref.cells(img, None, 7, 5, characters, colors, **ref.EDGE_POST)
            got, info = ctx.image_cells(img, None, 7, 5, characters, colors, **ref.EDGE_POST)
            assert_cells(got, want, f"no records, colours {colors}")
            assert info.counters() == counters
            half = np.ascontiguousarray((img * F(0.25)).astype(np.float16))
            want, counters = ref.cells(half.astype(F), None, 7, 5, characters, colors, postprocessed=True)
            dev = to_device(half)
            got, info = ctx.image_cells(dev.data_ptr(), 0, 7, 5, characters, colors, exposure=7.0, tone_mapping=1, maximum_intensity=0.5, postprocessed=True,
                                        f16=True, image_device=True)
            assert_cells(got, want, f"postprocessed f16 on the device, colours {colors}")
            assert info.counters() == counters


# --- aic_render_cells against the oracle's frame --------------------------------------------------------------------------------------------------------
COLS, ROWS = 12, 6
EYE, TARGET, VD = (6.5, 9.0, 15.0), (6.0, 3.0, 5.0), 40.0


@pytest.fixture(scope="module")
def world():
    sp = scenes.synthetic_space(n=12, resolution=4, n_blocks=6, seed=3)
    sp.set_sky_octants(np.random.default_rng(3).uniform(0.1, 2.4, (8, 3)))
    return sp


def to_abi_aux(oracle_aux, layer):
    aux = np.zeros(oracle_aux.shape, abi.PIXEL_AUX_DTYPE)
    for k in ("hit", "block_index", "cubes_traced"):
        aux[k] = oracle_aux[k]
    aux["layer"] = layer
    return aux


@pytest.mark.parametrize("with_ui", [False, True])
@pytest.mark.parametrize("characters", ref.CHARACTER_MODES)
def test_render_cells_equal_the_restatement_over_the_oracles_frame(ctx, world, characters, with_ui):
    """aic_render_cells == the restatement over oracle.render(want_linear, want_aux): Clamp and Reinhard, antialiasing None (all three words) and Always
    (the colour words). Every pixel, UI pixels included, takes the WORLD camera's exposure and the world options' tone mapping. The oracle's records
    carry no layer: it is taken from the device's own record, whose other fields the test holds to the oracle's."""
    (w, h), _ = ref.geometry(COLS, ROWS, characters)
    exposure = 1.5
    ui = scenes.ui_space()
    ctx.upload_space(abi.LAYER_WORLD, world)
    if with_ui:
        ctx.upload_space(abi.LAYER_UI, ui)
    else:
        ctx.clear_space(abi.LAYER_UI)
    try:
        for tone_mapping, maximum_intensity, aa in ((0, 1.0, 0), (1, 2.0, 0), (1, 1.0, 2)):
            opt = oracle.make_options(fog=2, lighting=3, antialiasing=aa, tone_mapping=tone_mapping, maximum_intensity=maximum_intensity, view_distance=VD)
            ui_opt = oracle.make_options(fog=0, lighting=1, antialiasing=aa, tone_mapping=1 - tone_mapping, maximum_intensity=0.25, view_distance=VD)
            _, _, inv = oracle.camera_matrices(90.0, VD, (COLS * 0.5) / (ROWS * 1.0), oracle.look_at_y_up(EYE, TARGET), EYE)
            _, _, ui_inv = oracle.camera_matrices(90.0, VD, (COLS * 0.5) / (ROWS * 1.0), (0, 0, 0, 1), (-2.2, -2.5, -1.5))
            ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
            kw = {}
            if with_ui:
                ctx.set_options(abi.LAYER_UI, to_abi_options(ui_opt))
                kw = dict(ui=oracle.Space(ui), ui_opt=ui_opt, ui_cam=oracle.make_camera(ui_inv, w, h))
            frame = oracle.render(oracle.Space(world), opt, oracle.make_camera(inv, w, h), want_linear=True, want_aux=True, **kw)
            fd = lambda: ctx.make_frame(w, h, world_inv=inv, ui_inv=ui_inv if with_ui else None, exposure=exposure, ui_exposure=0.3)  # noqa: E731
            device = ctx.render(fd(), want_aux=True)["aux"]
            if aa == 0:
                for k in ("hit", "block_index", "cubes_traced"):
                    assert (device[k] == frame["aux"][k]).all(), k
                if with_ui:
                    assert (device["layer"][device["hit"] == 1] == 1).any() and (device["layer"][device["hit"] == 1] == 0).any(), "both layers show"
            aux = to_abi_aux(frame["aux"], device["layer"])
            for colors in ref.COLOR_MODES:
                want, counters = ref.cells(frame["linear"], aux, COLS, ROWS, characters, colors, exposure=exposure, tone_mapping=tone_mapping,
                                           maximum_intensity=maximum_intensity)
                got, fi, ci = ctx.render_cells(fd(), COLS, ROWS, characters, colors)
                what = f"characters {characters} colours {colors} tone {tone_mapping} aa {aa} ui {with_ui}"
                assert fi.cubes_traced == int(frame["info"]["cubes_traced"]), what
                if aa == 0:
                    assert_cells(got, want, what)
                    assert ci.counters() == counters, what
                else:
                    assert (got["fg"] == want["fg"]).all() and (got["bg"] == want["bg"]).all(), what
                # the cells in device memory are the same cells
                dev_out = device_bytes(want.size * 12)
                none, _, _ = ctx.render_cells(fd(), COLS, ROWS, characters, colors, out_device=dev_out.data_ptr())
                assert none is None and (dev_out.cpu().numpy()[:want.size * 12].view(abi.CELL_DTYPE).reshape(want.shape) == got).all(), what
    finally:
        ctx.clear_space(abi.LAYER_UI)


def test_rejections_leave_the_context_usable(ctx, world):
    characters, colors = ref.SPLIT, ref.COLOR_256
    (w, h), _ = ref.geometry(COLS, ROWS, characters)
    opt = oracle.make_options(view_distance=VD)
    _, _, inv = oracle.camera_matrices(90.0, VD, w / h, oracle.look_at_y_up(EYE, TARGET), EYE)
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, world)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    want = oracle.render(oracle.Space(world), opt, oracle.make_camera(inv, w, h))["rgba8"]

    def still_good(what):
        assert (ctx.render(ctx.make_frame(w, h, world_inv=inv))["rgba8"] == want).all(), what

    def refused(fn, codes, what):
        with pytest.raises(abi.AicError) as e:
            fn()
        assert e.value.code in codes, (what, e.value.code)
        still_good(what)

    invalid, either = (1,), (1, 5)
    good = lambda **kw: ctx.make_frame(w, h, world_inv=inv, **kw)  # noqa: E731
    refused(lambda: ctx.render_cells(good(), COLS, ROWS, 5, colors), invalid, "a bad character mode")
    refused(lambda: ctx.render_cells(good(), COLS, ROWS, characters, 3), invalid, "a bad colour mode")
    refused(lambda: ctx.render_cells(ctx.make_frame(w, h + 1, world_inv=inv), COLS, ROWS, characters, colors), invalid, "a frame that is not the geometry's")
    refused(lambda: ctx.render_cells(good(), COLS, ROWS, ref.BRAILLE, colors), invalid, "the geometry of another mode")
    refused(lambda: ctx.render_cells(good(partition=(4, 2, 0)), COLS, ROWS, characters, colors), either, "a partition")
    for flag in (abi.FRAME_OUT_LINEAR, abi.FRAME_OUT_COLORBUF, abi.FRAME_OUT_SPLIT, abi.FRAME_AUX):
        refused(lambda: ctx.render_cells(good(flags=flag), COLS, ROWS, characters, colors), either, f"the caller's output flag {flag}")
    refused(lambda: ctx.render_cells(good(flags=abi.FRAME_BLOOM), COLS, ROWS, characters, colors), either, "bloom")
    image = np.zeros((ROWS, COLS, 4), F)
    refused(lambda: ctx.image_cells(image, None, COLS, ROWS, ref.NAMES, colors), invalid, "Names without records")
    refused(lambda: ctx.image_cells(image, None, COLS, ROWS, 7, colors), invalid, "a bad mode for an image")
    refused(lambda: ctx.image_cells(image, None, COLS, ROWS, ref.SHADES, colors, tone_mapping=2), invalid, "a bad tone mapping")
    refused(lambda: ctx.image_cells(image, None, COLS, ROWS, ref.SHADES, colors, exposure=-1.0), invalid, "a negative exposure")
    dev = to_device(image)
    refused(lambda: ctx.image_cells(dev.data_ptr() + 4, 0, COLS, ROWS, ref.SHADES, colors, image_device=True), invalid, "a misaligned device image")
    d = abi.CellsDesc(COLS, ROWS, ref.SHADES, colors, 1.0, 0, float("inf"), 16)
    out = np.zeros((ROWS, COLS), abi.CELL_DTYPE)
    assert ctx._lib.aic_image_cells(ctx._h, C.byref(d), image.ctypes.data, None, out.ctypes.data, None) == 1, "an unknown flag"
    still_good("an unknown flag")
    got, _, _ = ctx.render_cells(good(), COLS, ROWS, characters, colors)  # and the call itself still works
    assert got.shape == (ROWS, COLS)


# --- the host mirror ------------------------------------------------------------------------------------------------------------------------------------
def mirror(viewport, space=None, eye=(1.4, 1.1, 2.6), target=(1.5, 0.5, 0.5)):
    import all_is_cubes_amd as A

    cams = H.StandardCameras()
    o = H.GraphicsOptions()
    o.bloom_intensity = 0.0
    cams.graphics_options = o
    cams.viewport = viewport
    cams.world_space = A.space_from_flat(scenes.print_space_test_space() if space is None else space)
    cams.world_view_transform = H.look_at_y_up(eye, target)
    r = H.HipRtRenderer(cams)
    r.update()
    return cams, r


def test_terminal_options_of_the_mirror():
    o = H.TerminalOptions()
    assert (o.colors, o.characters) == (H.TerminalColorMode.TwoFiftySix, H.TerminalCharacterMode.Split)  # options.rs:41-48
    seen = []
    for _ in range(5):
        seen.append(int(o.characters))
        o.cycle_characters()
    assert seen == [2, 3, 4, 0, 1] and int(o.characters) == 2
    o.cycle_colors()
    assert o.colors == H.TerminalColorMode.Rgb
    o.cycle_colors()
    assert o.colors == H.TerminalColorMode.None_
    vp = o.viewport_from_terminal_size(0, 7)
    assert (vp.framebuffer_width, vp.framebuffer_height, vp.nominal_width, vp.nominal_height) == (1, 14, 0.5, 7.0)


@pytest.mark.parametrize("characters", ref.CHARACTER_MODES)
def test_draw_terminal_is_cells_ansi_of_draw_cells(characters):
    o = H.TerminalOptions()
    o.characters = H.TerminalCharacterMode(characters)
    _, r = mirror(o.viewport_from_terminal_size(COLS, ROWS))
    names, widths = r.terminal_names()
    assert names[0][-3:] == ["0", "1", "2"] and widths[0][-3:] == [1, 1, 1] and names[1] == []
    for colors in ref.COLOR_MODES:
        o.colors = H.TerminalColorMode(colors)
        frame = r.draw_cells(o)
        assert (frame.cols, frame.rows) == (COLS, ROWS)
        cells = np.ascontiguousarray(frame.cells).view(abi.CELL_DTYPE).reshape(ROWS, COLS)
        for in_rect, origin in ((False, (0, 0)), (True, (4, 2))):
            assert r.draw_terminal(o, in_rect, origin) == abi.cells_ansi(cells, names, widths, in_rect, origin) == ref.ansi(cells, names, widths, in_rect, origin)
        if characters == ref.NAMES:
            assert {"0", "1", "2"} <= set(ref.ansi(cells, names, widths).decode())
    if characters == ref.NAMES:  # a viewport of 12 x 6 pixels is no grid of 2 x 4 patches
        o.characters = H.TerminalCharacterMode.Braille
        with pytest.raises(ValueError):
            r.draw_cells(o)


def test_present_split_cells_equal_the_restatement_over_the_f16_presentation(world):
    """The resident interactive frame's terminal target: aic_present_split with AIC_PRESENT_OUT_F16 at the cells' framebuffer size, then the cells of
    that image -- which the test reads back from the scratch the call leaves it in."""
    w, h = 48, 32
    _, r = mirror(H.Viewport.with_scale(1.0, w, h), world, EYE, TARGET)
    resident = to_device(split_bytes(r.draw_split()))
    o = H.TerminalOptions()
    for characters, colors in MODE_PAIRS:
        o.characters, o.colors = H.TerminalCharacterMode(characters), H.TerminalColorMode(colors)
        (fw, fh), _ = ref.geometry(COLS, ROWS, characters)
        scratch = device_bytes(fw * fh * 8)
        if characters == ref.NAMES:
            with pytest.raises(ValueError):
                r.present_split_cells(resident.data_ptr(), scratch.data_ptr(), COLS, ROWS, o)
            continue
        frame = r.present_split_cells(resident.data_ptr(), scratch.data_ptr(), COLS, ROWS, o)
        shown = scratch.cpu().numpy()[:fw * fh * 8].view(np.float16).reshape(fh, fw, 4)
        assert (shown[..., 3] == 1.0).all() and len(np.unique(shown[..., :3])) > 4, "a frame that shows something"
        want, counters = ref.cells(shown.astype(F), None, COLS, ROWS, characters, colors, postprocessed=True)
        got = np.ascontiguousarray(frame.cells).view(abi.CELL_DTYPE).reshape(ROWS, COLS)
        assert_cells(got, want, f"characters {characters} colours {colors}")
        assert frame.counters.tolist() == [COLS * ROWS] + [counters[k] for k in ref.COUNTERS]
