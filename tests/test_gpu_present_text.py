"""GPU tests (-m gpu) of aic_present_split_text: the info text of the interactive renderer laid over a presented Split frame on the device
(all-is-cubes-gpu shaders/postprocess.wgsl:160-276, text.rs, everything.rs:777-806).

Yardstick: tests/present_text_ref.py, the NumPy restatement of DESIGN.md 4.14, over tests/present_ref.py's scene and chain. Without bloom both output
kinds equal it bit for bit. With bloom the pixels whose text alpha is 1 are exact -- the scene has weight 0 there -- and the rest keep the bounds the
chain has against its own restatement (tests/test_gpu_bloom.py): f16 within 2 ulps, RGBA8 within 1 level. The frames and their S and B
are tests/test_gpu_present.py's, computed once per size pair. Every combination of a font cell, a nominal size and an origin is run; of a combination's
atlases and grids every other one has a blank space cell and codes in one corner only, which is what lets the library skip pixels, and the restatement
knows nothing of that."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import present_ref
from tests import present_text_ref as ref
from tests import scenes
from tests.test_gpu_bloom import f16_ulps
from tests.test_gpu_present import CASES, KINDS, restated
from tests.test_gpu_reproject import GUARD, SENTINEL, device_bytes, frame_bytes, split_bytes, to_device

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [((1, 1), (1, 1)), ((5, 3), (7, 5)), ((16, 16), (16, 16)), ((64, 48), (200, 120)), ((33, 17), (20, 9))]
CELLS = [(9, 18, 1), (5, 7, 0), (8, 8, 2), (3, 3, 1)]
NOMINALS = ["window", "half", "two thirds", (123.5, 77.25)]  # the window's size, / 2, / 1.5, and a size that has nothing to do with it
ORIGINS = [(5.0, 5.0), (0.0, 0.0), (-11.0, -7.5)]  # the reference's; none; a grid partly off the window to the top left
AIC_ERR_INVALID = 1
IDENTITY = np.eye(4, dtype=F).reshape(16)


def nominal_of(kind, out_size):
    if kind == "window":
        return (float(out_size[0]), float(out_size[1]))
    if kind == "half":
        return (out_size[0] / 2.0, out_size[1] / 2.0)
    if kind == "two thirds":
        return (out_size[0] / 1.5, out_size[1] / 1.5)
    return kind


@functools.lru_cache(maxsize=None)
def font(cell, blank_space, seed=0):
    """A random atlas of bytes 0..255 (values 0 and 255 among them), with cell 0x20 all zero or not."""
    cw, ch, _ = cell
    rng = np.random.default_rng(1000 * cw + 10 * ch + seed)
    atlas = rng.integers(0, 256, (16 * ch, 16 * cw, 4)).astype(np.uint8)
    atlas[rng.random(atlas.shape[:2]) < 0.2] = 0
    atlas[..., 3][rng.random(atlas.shape[:2]) < 0.3] = 255
    if blank_space:
        atlas[2 * ch:3 * ch, 0:cw] = 0
    else:
        atlas[2 * ch, 0, 3] = 77
    atlas.setflags(write=False)
    return atlas


def grid(cols, rows, corner_only, seed):
    """Random codes with 0, 0x20 and 0xFF among them; corner_only: zero outside the top left quarter."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    codes[rng.random((rows, cols)) < 0.2] = 0
    codes[rng.random((rows, cols)) < 0.1] = 0x20
    codes[rng.random((rows, cols)) < 0.1] = 0xFF
    flat = codes.reshape(-1)
    for i, v in enumerate((0xFF, 0x20, 0)):
        flat[(7 * i) % flat.size] = v
    if corner_only:
        codes[(rows + 1) // 2:, :] = 0
        codes[:, (cols + 1) // 2:] = 0
    return codes


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def present(ctx, src, src_size, out_size, case, flags, dtype, text, lines=None):
    """One call into a fresh sentinel-filled device buffer: the image; the guard bytes behind it are checked here. lines: (view_projection, vertices)."""
    n = out_size[0] * out_size[1]
    px = 4 * np.dtype(dtype).itemsize
    out = device_bytes(n * px + GUARD)
    vp, vertices = lines if lines is not None else (None, None)
    none, info, _ = ctx.present_split_text(src.data_ptr(), src_size, out_size, *case, text=text, view_projection=vp, vertices=vertices, flags=flags, out_device=out.data_ptr())
    assert none is None and info.bloomed == int(case[0] > 0)
    raw = out.cpu().numpy()
    assert (raw[n * px:] == SENTINEL).all(), "guard bytes behind out"
    return raw[:n * px].view(dtype).reshape(out_size[1], out_size[0], 4)


def assert_equals_restatement(got, want, layer, bloomed, flags, what):
    """Bit for bit without bloom; with bloom exact where the text is opaque, and the chain's own bounds elsewhere."""
    if not bloomed:
        assert (got == want).all(), what
        return
    opaque = layer[..., 3] == 1.0
    assert (got[opaque] == want[opaque]).all(), what
    if flags:
        assert (got[..., 3] == present_ref.ONE_F16).all(), what
        assert f16_ulps(got[..., :3].view(np.float16), want[..., :3].view(np.float16)).max() <= 2, what
    else:
        assert (got[..., 3] == 255).all(), what
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, what


@pytest.mark.parametrize("src_size,out_size", SIZES)
def test_synthetic_frames_equal_the_restatement(ctx, src_size, out_size):
    color, depth, parts = restated(src_size, out_size)
    src_bytes = frame_bytes(color, depth)
    src = to_device(src_bytes)
    w, h = out_size
    shown = skipped = 0
    for i, (cell, nominal, origin_px) in enumerate(itertools.product(CELLS, NOMINALS, ORIGINS)):
        corner = i % 2 == 1
        atlas = font(cell, corner)
        cols, rows, scale, origin = abi.text_geometry(nominal_of(nominal, out_size), cell, origin_px)
        codes = grid(cols, rows, corner, 100 * w + i)
        ctx.set_text_font(atlas, *cell)
        layer = ref.text_layer(w, h, atlas, cell, codes, scale, origin)
        shown += int((layer[..., 3] > 0).sum())
        skipped += int(corner)
        for case in CASES:
            for flags, dtype in KINDS:
                bi, tm, mi = case
                want = ref.composite(parts["S"], parts["B"], bi, tm, mi, out_f16=bool(flags), text=layer)
                got = present(ctx, src, src_size, out_size, case, flags, dtype, (codes, scale, origin))
                what = f"{src_size} -> {out_size} cell {cell} nominal {nominal} origin {origin_px} case {case} {'f16' if flags else 'rgba8'}"
                assert_equals_restatement(got, want, layer, bi > 0, flags, what)
    print(f"{src_size} -> {out_size}: {shown} text pixels over {len(CELLS) * len(NOMINALS) * len(ORIGINS)} combinations, {skipped} with a blank space")
    assert shown > 0
    assert (src.cpu().numpy() == src_bytes).all(), "src changed"


def test_a_space_that_is_not_blank_shows_on_every_covered_pixel(ctx):
    """An all-zero grid reads cell 0x20 everywhere: with an opaque space every pixel the grid covers shows it, and none is skipped."""
    src_size, out_size = (33, 17), (20, 9)
    color, depth, parts = restated(src_size, out_size)
    src = to_device(frame_bytes(color, depth))
    cell = (5, 7, 0)
    atlas = np.zeros((16 * 7, 16 * 5, 4), np.uint8)
    atlas[2 * 7:3 * 7, 0:5] = (64, 128, 191, 255)
    ctx.set_text_font(atlas, *cell)
    cols, rows, scale, origin = abi.text_geometry((20.0, 9.0), cell, (0.0, 0.0))
    codes = np.zeros((rows, cols), np.uint8)
    layer = ref.text_layer(20, 9, atlas, cell, codes, scale, origin)
    assert (layer[..., 3] == 1.0).all()
    for case in CASES:
        got = present(ctx, src, src_size, out_size, case, abi.PRESENT_OUT_F16, np.uint16, (codes, scale, origin))
        assert (got == ref.composite(parts["S"], parts["B"], *case, out_f16=True, text=layer)).all()
        assert (got.view(np.float16)[..., :3] == (np.array([64, 128, 191], F) / F(255)).astype(np.float16)).all()
    # half covered: origin at the middle of the window
    origin = np.array([0.5, 0.0], F)
    layer = ref.text_layer(20, 9, atlas, cell, codes, scale, origin)
    assert (layer[:, :10, 3] == 0.0).all() and (layer[:, 10:, 3] == 1.0).all()
    got = present(ctx, src, src_size, out_size, CASES[0], 0, np.uint8, (codes, scale, origin))
    assert (got == ref.composite(parts["S"], None, *CASES[0], text=layer)).all()
    assert (got[:, :10] == present_ref.composite(parts["S"], None, *CASES[0])[:, :10]).all()


def test_device_codes_host_target_and_the_same_call_twice(ctx):
    src_size, out_size = (64, 48), (200, 120)
    color, depth, parts = restated(src_size, out_size)
    src_bytes = frame_bytes(color, depth)
    src = to_device(src_bytes)
    cell = (9, 18, 1)
    for blank in (True, False):
        atlas = font(cell, blank)
        ctx.set_text_font(atlas, *cell)
        cols, rows, scale, origin = abi.text_geometry((200.0, 120.0), cell)
        codes = grid(cols, rows, True, 9)
        on_device = to_device(np.concatenate([codes.reshape(-1), np.full(GUARD, SENTINEL, np.uint8)]))
        layer = ref.text_layer(200, 120, atlas, cell, codes, scale, origin)
        for case in (CASES[1], CASES[3]):
            for flags, dtype in KINDS:
                got = present(ctx, src, src_size, out_size, case, flags, dtype, (codes, scale, origin))
                want = ref.composite(parts["S"], parts["B"], *case, out_f16=bool(flags), text=layer)
                assert_equals_restatement(got, want, layer, case[0] > 0, flags, (blank, case, flags))
                again = present(ctx, src, src_size, out_size, case, flags, dtype, (codes, scale, origin))
                assert (again == got).all(), "the same call twice"
                from_device = present(ctx, src, src_size, out_size, case, flags, dtype, ((on_device.data_ptr(), cols, rows), scale, origin))
                assert (from_device == got).all(), "device codes"
                on_host, info, _ = ctx.present_split_text(src.data_ptr(), src_size, out_size, *case, text=(codes, scale, origin), flags=flags)
                assert on_host.dtype == dtype and (on_host == got).all(), "host target"
        raw = on_device.cpu().numpy()
        assert (raw[:codes.size] == codes.reshape(-1)).all() and (raw[codes.size:] == SENTINEL).all(), "device codes changed"
    assert (src.cpu().numpy() == src_bytes).all(), "src changed"


def line_frame(w, h, row=3):
    """A frame every line fragment at depth 0.5 passes: random colours, depth 1.0; and a horizontal line across `row` under the identity matrix."""
    rng = np.random.default_rng(w * h)
    color = rng.exponential(0.5, (h, w, 4)).astype(np.float16).view(np.uint16)
    depth = np.full((h, w), np.array([1.0], F).view(np.uint32)[0], np.uint32)
    y = 1.0 - (row + 0.5) / h * 2.0
    vertices = np.array([[[-1.0, y, 0.5, 4.0, 0.0, 0.25, 1.0], [1.0, y, 0.5, 4.0, 0.0, 0.25, 1.0]]], F)
    return color, depth, vertices


def test_no_text_is_aic_present_split_lines(ctx):
    w, h = 40, 24
    color, depth, vertices = line_frame(w, h)
    src = to_device(frame_bytes(color, depth))
    ctx.set_text_font(font((9, 18, 1), True), 9, 18, 1)
    for out_size in ((w, h), (100, 37)):
        for case in (CASES[0], CASES[3]):
            for flags, dtype in KINDS:
                for given in (None, vertices):
                    with_lines, _, li = ctx.present_split_lines(src.data_ptr(), (w, h), out_size, *case, IDENTITY, vertices=given, flags=flags)
                    got = present(ctx, src, (w, h), out_size, case, flags, dtype, None, (IDENTITY, given))
                    assert (got == with_lines).all(), (out_size, case, flags, given is None)
                    assert (li.n_pixels > 0) == (given is not None)
                plain, _ = ctx.present_split(src.data_ptr(), (w, h), out_size, *case, flags=flags)
                assert (present(ctx, src, (w, h), out_size, case, flags, dtype, None) == plain).all()


def test_text_lies_over_lines(ctx):
    """A line pixel under a glyph shows the glyph; where the text is clear it shows the line."""
    w, h = 40, 24
    cell = (9, 18, 1)
    atlas = H.info_text_font_atlas()
    ctx.set_text_font(atlas, *cell)
    cols, rows, scale, origin = abi.text_geometry((w, h), cell, (0.0, 0.0))
    codes, _ = abi.text_layout("MMM", cols, rows)
    layer = ref.text_layer(w, h, atlas, cell, codes, scale, origin)
    row = int(np.argmax((layer[..., 3] == 1.0).sum(axis=1)))  # the row of the window with the most glyph and outline pixels
    color, depth, vertices = line_frame(w, h, row)
    src = to_device(frame_bytes(color, depth))
    case = (0.0, 0, np.inf)
    lines_only = present(ctx, src, (w, h), (w, h), case, abi.PRESENT_OUT_F16, np.uint16, None, (IDENTITY, vertices))
    line_colour = np.array([4.0, 0.0, 0.25, 1.0], np.float16).view(np.uint16)
    assert (lines_only[row] == line_colour).all() and (lines_only[row - 1] != line_colour).any()
    s_lines = lines_only.view(np.float16).astype(F)  # no tone map and no bloom: the f16 output is the scene with its lines
    for flags, dtype in KINDS:
        got = present(ctx, src, (w, h), (w, h), case, flags, dtype, (codes, scale, origin), (IDENTITY, vertices))
        assert (got == ref.composite(s_lines, None, *case, out_f16=bool(flags), text=layer)).all()
    under = layer[row, :, 3] == 1.0
    assert under.sum() >= 6 and (~under).sum() >= 6
    got = present(ctx, src, (w, h), (w, h), case, abi.PRESENT_OUT_F16, np.uint16, (codes, scale, origin), (IDENTITY, vertices))
    assert (got[row][under][:, :3].view(np.float16) == layer[row][under][:, :3].astype(np.float16)).all()
    assert (got[row][~under] == line_colour).all()
    # bloomed too: the text is not bloomed, so its opaque pixels are exactly the atlas's
    bloomed = present(ctx, src, (w, h), (w, h), (0.25, 1, 1.0), abi.PRESENT_OUT_F16, np.uint16, (codes, scale, origin), (IDENTITY, vertices))
    opaque = layer[..., 3] == 1.0
    assert (bloomed[opaque][:, :3].view(np.float16) == layer[opaque][:, :3].astype(np.float16)).all()


def test_replacing_the_font_between_two_calls(ctx):
    src_size, out_size = (16, 16), (16, 16)
    color, depth, parts = restated(src_size, out_size)
    src = to_device(frame_bytes(color, depth))
    case = CASES[1]
    images = []
    for cell, seed in (((9, 18, 1), 0), ((3, 3, 1), 0), ((9, 18, 1), 5), ((8, 8, 2), 0)):
        atlas = font(cell, False, seed)
        ctx.set_text_font(atlas, *cell)
        cols, rows, scale, origin = abi.text_geometry((16.0, 16.0), cell)
        codes = grid(cols, rows, False, 3)
        got = present(ctx, src, src_size, out_size, case, 0, np.uint8, (codes, scale, origin))
        assert (got == ref.composite(parts["S"], None, *case, text=ref.text_layer(16, 16, atlas, cell, codes, scale, origin))).all(), (cell, seed)
        images.append(got)
    assert (images[0] != images[2]).any()
    ctx.set_text_font(None)
    with pytest.raises(abi.AicError) as err:
        present(ctx, src, src_size, out_size, case, 0, np.uint8, (codes, scale, origin))
    assert err.value.code == AIC_ERR_INVALID
    assert (present(ctx, src, src_size, out_size, case, 0, np.uint8, None) == present_ref.composite(parts["S"], None, *case)).all()


def test_rejections_leave_the_context_usable(ctx):
    import oracle

    src_size, out_size = (33, 17), (20, 9)
    color, depth, parts = restated(src_size, out_size)
    src = to_device(frame_bytes(color, depth))
    out = device_bytes(20 * 9 * 8 + GUARD)
    cell = (5, 7, 0)
    atlas = font(cell, True)
    cols, rows, scale, origin = abi.text_geometry((20.0, 9.0), cell)
    codes = grid(cols, rows, False, 1)
    on_device = to_device(codes)
    case = (0.25, 1, 1.0)
    want = ref.composite(parts["S"], parts["B"], *case, text=ref.text_layer(20, 9, atlas, cell, codes, scale, origin))

    def good(what):
        ctx.set_text_font(atlas, *cell)
        got = present(ctx, src, src_size, out_size, case, 0, np.uint8, (codes, scale, origin))
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, what

    def raw_call(text=None, lines=None, src_ptr=None, out_ptr=None, **kw):
        """the good call with fields of the text descriptor (`text`, a dict) or of the presentation's (`kw`) replaced"""
        d = abi.PresentDesc()
        d.src_width, d.src_height, d.out_width, d.out_height = *src_size, *out_size
        d.bloom_intensity, d.tone_mapping, d.maximum_intensity, d.flags = 0.25, 1, 1.0, 0
        t = abi.TextDesc()
        t.scale[:], t.origin[:], t.cols, t.rows, t.codes = list(scale), list(origin), cols, rows, codes.ctypes.data
        for k, v in (text or {}).items():
            if k in ("scale", "origin"):
                getattr(t, k)[:] = v
            else:
                setattr(t, k, v)
        for k, v in kw.items():
            setattr(d, k, v)
        info, li = abi.PresentInfo(), abi.LinesInfo()
        ctx._check(ctx._lib.aic_present_split_text(ctx._h, C.byref(d), C.byref(lines) if lines is not None else None, C.byref(t),
                                                   C.c_void_p(src.data_ptr() if src_ptr is None else src_ptr), C.c_void_p(out.data_ptr() if out_ptr is None else out_ptr), 1,
                                                   C.byref(info), C.byref(li)))

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert (out.cpu().numpy() == SENTINEL).all(), what
        good(what)

    good("before")
    # the font: a cell dimension outside 1..1024, a margin that leaves no logical cell
    for bad in ((0, 7, 0), (5, 0, 0), (1025, 7, 0), (5, 1025, 0), (5, 7, 3), (4, 7, 2), (6, 6, 3)):
        rejected(lambda: ctx._check(ctx._lib.aic_set_text_font(ctx._h, atlas.ctypes.data_as(C.c_void_p), *bad)), f"font cell {bad}")
    # text given but no font set
    ctx.set_text_font(None)
    with pytest.raises(abi.AicError) as err:
        raw_call()
    assert err.value.code == AIC_ERR_INVALID and (out.cpu().numpy() == SENTINEL).all()
    good("after no font")
    # the text's own
    rejected(lambda: raw_call({"codes": None}), "NULL codes")
    rejected(lambda: raw_call({"codes": None, "flags": abi.TEXT_DEVICE}), "NULL device codes")
    for k in ("cols", "rows"):
        for bad in (0, 65536, 1 << 31):
            rejected(lambda: raw_call({k: bad}), f"{k} {bad}")
    for k in ("scale", "origin"):
        for bad in ([float("nan"), 1.0], [1.0, float("inf")], [float("-inf"), 0.0]):
            rejected(lambda: raw_call({k: bad}), f"{k} {bad}")
    for bad in (2, 3, 1 << 31):
        rejected(lambda: raw_call({"flags": bad}), f"text flags {bad}")
    # everything aic_present_split_lines rejects: a sample of the presentation's and of the lines' own
    rejected(lambda: raw_call(src_ptr=src.data_ptr() + 4), "src at 4 bytes")
    rejected(lambda: raw_call(out_ptr=out.data_ptr() + 2), "out at 2 bytes")
    rejected(lambda: raw_call(out_ptr=src.data_ptr()), "out == src")
    rejected(lambda: raw_call(out_width=65536), "out width above 65535")
    rejected(lambda: raw_call(src_width=0), "an empty source")
    rejected(lambda: raw_call(bloom_intensity=float("nan")), "bloom_intensity NaN")
    rejected(lambda: raw_call(maximum_intensity=-1.0), "maximum_intensity negative")
    rejected(lambda: raw_call(tone_mapping=2), "tone_mapping 2")
    rejected(lambda: raw_call(flags=2), "flags 2")
    ld = abi.LinesDesc()
    ld.view_projection[:] = [float(v) for v in IDENTITY]
    ld.n_lines, ld.vertices = 1, None
    rejected(lambda: raw_call(lines=ld), "lines without vertices")
    ld.n_lines, ld.flags = 0, 2
    rejected(lambda: raw_call(lines=ld), "unknown line flags")
    ld.flags = 0
    ld.view_projection[5] = float("nan")
    rejected(lambda: raw_call(lines=ld), "NaN in view_projection")
    # a frame still occupying slot 0: the presentation and the font
    ctx.upload_space(abi.LAYER_WORLD, scenes.one_cube_space())
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    eye = (0.7, 0.9, 2.5)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, 40 / 24, oracle.look_at_y_up(eye, (0.5, 0.5, 0.5)), eye)
    busy = device_bytes(40 * 24 * 4)
    ctx.render_submit(ctx.make_frame(40, 24, world_inv=inv), busy.data_ptr(), 0)
    for call in (raw_call, lambda: ctx.set_text_font(atlas, *cell)):
        with pytest.raises(abi.AicError) as err:
            call()
        assert err.value.code == AIC_ERR_INVALID, "slot 0 busy"
    ctx.render_wait(0)
    ctx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    good("after slot 0 busy")
    # an empty output: AIC_OK and nothing written
    raw_call(out_width=0)
    assert (out.cpu().numpy() == SENTINEL).all()
    assert (on_device.cpu().numpy() == codes.reshape(-1)).all()
    good("after the empty output")


def test_through_the_host_mirror():
    """A small scene's Split frame presented at 96 x 64 with "a b\\nc": present_split without text, overlaid by draw_info_text in black and white; with
    debug_info_text off, no overlay."""
    import all_is_cubes_amd as A

    w, h = 96, 64
    cams = H.StandardCameras()
    o = H.GraphicsOptions()
    o.bloom_intensity = 0.0
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(scenes.one_cube_space())
    cams.world_view_transform = H.look_at_y_up((0.7, 0.9, 2.5), (0.5, 0.5, 0.5))
    r = H.HipRtRenderer(cams)
    r.update()
    resident = to_device(split_bytes(r.draw_split()))
    text = "a b\nc"
    plain = r.present_split(resident.data_ptr(), w, h)
    want = plain.data.copy()
    H.draw_info_text(want, text, (0, 0, 0, 255), (255, 255, 255, 255))
    assert (want != plain.data).any(axis=-1).sum() >= 3 * 20
    shown, lines_info = r.present_split_text(resident.data_ptr(), w, h, text)
    assert (shown.width, shown.height) == (w, h) and lines_info["n_pixels"] == 0
    assert (shown.data == want).all()
    again, _ = r.present_split_text(resident.data_ptr(), w, h, text)  # (the font is set already)
    assert (again.data == want).all()
    # the device form, with the lines pass of a list of no lines
    out = device_bytes(w * h * 4 + GUARD)
    info, _ = r.present_split_text(resident.data_ptr(), w, h, text, True, np.zeros((0, 7), F), 0, out.data_ptr())
    raw = out.cpu().numpy()
    assert info["bloomed"] == 0 and (raw[w * h * 4:] == SENTINEL).all()
    assert (raw[:w * h * 4].reshape(h, w, 4) == want).all()
    o.debug_info_text = False
    cams.graphics_options = o
    r.update()
    hidden, _ = r.present_split_text(resident.data_ptr(), w, h, text)
    assert (hidden.data == plain.data).all()
