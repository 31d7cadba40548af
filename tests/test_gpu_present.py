"""GPU tests (-m gpu) of aic_present_split: a resident Split frame stretched to the window, bloomed, tone-mapped and encoded
(raytrace_to_texture.rs:546-568, shaders/rt-copy.wgsl:41-71, bloom.rs:41-60, shaders/postprocess.wgsl:140-158 and 251-276).

Yardstick: tests/present_ref.py, the NumPy restatement of DESIGN.md 4.11. Without bloom both output kinds equal it bit for bit; with bloom the bounds are
those the chain already has against its own restatement (tests/test_gpu_bloom.py): f16 within 2 ulps, RGBA8 within 1 level. Sizes (source -> output):
one texel, a one-level chain stretched, equal sizes with odd edges, up- and down-scales by whole and fractional ratios, several 256-thread blocks,
T0 larger than the output in one axis. S and B of a (source, output) pair are computed once and shared by the cases and tests that need them."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import bloom_ref, scenes
from tests import present_ref as ref
from tests.test_gpu_bloom import bloom_scene_camera, f16_ulps, to_abi
from tests.test_gpu_reproject import GUARD, SENTINEL, device_bytes, frame_bytes, split_bytes, to_device

pytestmark = pytest.mark.gpu

SIZES = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((2, 2), (2, 2)), ((3, 5), (3, 5)), ((3, 5), (7, 11)), ((17, 9), (34, 18)), ((17, 9), (33, 20)),
         ((64, 48), (40, 30)), ((64, 48), (256, 192)), ((128, 256), (128, 256))]
CASES = [(0.0, 0, np.inf), (0.0, 1, 1.0), (0.125, 0, np.inf), (0.25, 1, 1.0), (1.0, 0, 2.0)]  # (bloom_intensity, tone_mapping, maximum_intensity)
KINDS = [(0, np.uint8), (abi.PRESENT_OUT_F16, np.uint16)]
AIC_ERR_INVALID = 1
MARKER = (0, 0, 0, 0xBC00)


def synthetic_frame(w, h):
    """(colour [h, w, 4] u16, depth [h, w] u32 bit patterns): colours exponential-random f16 >= 0, one colour value in a hundred infinity or 65504; alpha
    random in [0, 1) with marker texels (0, 0, 0, -1) among them; a depth plane of random bits, NaNs and -0.0."""
    rng = np.random.default_rng(2000 * w + h)
    color = rng.exponential(2.0, (h, w, 4)).astype(np.float16).view(np.uint16)
    color[..., 3] = rng.random((h, w)).astype(np.float16).view(np.uint16)
    top = rng.random((h, w, 3)) < 0.01
    color[..., :3][top] = np.where(rng.random(int(top.sum())) < 0.5, 0x7C00, 0x7BFF).astype(np.uint16)
    if w * h >= 4:
        color[0, 0, 0], color[-1, -1, 1] = 0x7C00, 0x7BFF
        color[rng.random((h, w)) < 0.05] = MARKER
        color[h // 2, w // 2] = MARKER
    depth = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    depth[rng.random((h, w)) < 0.1] = 0x7FC00000
    depth[rng.random((h, w)) < 0.1] = 0x80000000
    return color, depth


@functools.lru_cache(maxsize=None)
def restated(src, out):
    """The frame of a size pair and the parts of its restatement that do not depend on the case: S and B."""
    color, depth = synthetic_frame(*src)
    parts = {"S": ref.scene(color, *out)}
    parts["B"] = ref.chain(parts["S"])
    for a in (color, depth, parts["S"], parts["B"]):
        a.setflags(write=False)
    return color, depth, parts


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def present_to_device(ctx, src, src_size, out_size, case, flags, dtype):
    """One call into a fresh sentinel-filled device buffer: (image, info); the guard bytes behind the image are checked here."""
    n = out_size[0] * out_size[1]
    px = 4 * np.dtype(dtype).itemsize
    out = device_bytes(n * px + GUARD)
    assert out.data_ptr() % 8 == 0
    none, info = ctx.present_split(src.data_ptr(), src_size, out_size, *case, flags=flags, out_device=out.data_ptr())
    assert none is None
    raw = out.cpu().numpy()
    assert (raw[n * px:] == SENTINEL).all(), "guard bytes behind out"
    return raw[:n * px].view(dtype).reshape(out_size[1], out_size[0], 4), info


@pytest.mark.parametrize("src_size,out_size", SIZES)
def test_synthetic_frames_equal_the_restatement(ctx, src_size, out_size):
    color, depth, parts = restated(src_size, out_size)
    src_bytes = frame_bytes(color, depth)
    src = to_device(src_bytes)
    levels, t0 = bloom_ref.geometry(*out_size)
    for case in CASES:
        i, tm, mi = case
        for flags, dtype in KINDS:
            want = ref.composite(parts["S"], parts["B"], i, tm, mi, out_f16=bool(flags))
            got, info = present_to_device(ctx, src, src_size, out_size, case, flags, dtype)
            what = f"{src_size[0]}x{src_size[1]} -> {out_size[0]}x{out_size[1]} i {i} tm {tm} max {mi} {'f16' if flags else 'rgba8'}"
            print(f"{what}: exact {float((got == want).all(axis=-1).mean()):.4f}")
            assert (info.levels, tuple(info.t0), info.bloomed) == (levels, t0, int(i > 0)), what
            if i == 0:
                assert (got == want).all(), what
            elif flags:
                assert (got[..., 3] == ref.ONE_F16).all(), what
                assert f16_ulps(got[..., :3].view(np.float16), want[..., :3].view(np.float16)).max() <= 2, what
            else:
                assert (got[..., 3] == 255).all(), what
                assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, what
            again, _ = present_to_device(ctx, src, src_size, out_size, case, flags, dtype)
            assert (again == got).all(), "the same call twice: " + what
            on_host, host_info = ctx.present_split(src.data_ptr(), src_size, out_size, i, tm, mi, flags=flags)
            assert on_host.dtype == dtype and (on_host == got).all(), "host target: " + what
            assert (host_info.levels, host_info.bloomed) == (info.levels, info.bloomed)
    assert (src.cpu().numpy() == src_bytes).all(), "src changed"


def test_source_alpha_and_depth_are_never_read(ctx):
    src_size, out_size = (17, 9), (33, 20)
    color, depth, _ = restated(src_size, out_size)
    rng = np.random.default_rng(5)
    other = color.copy()
    other[..., 3] = rng.integers(0, 1 << 16, color.shape[:2])  # any bits: NaNs, infinities, negatives
    other_depth = rng.integers(0, 1 << 32, depth.shape, dtype=np.uint64).astype(np.uint32)
    assert (other[..., 3] != color[..., 3]).any() and (other_depth != depth).any()
    a, b = to_device(frame_bytes(color, depth)), to_device(frame_bytes(other, other_depth))
    for sizes in ((src_size, out_size), (src_size, src_size)):
        for case in ((0.25, 1, 1.0), (0.0, 0, np.inf)):
            for flags, dtype in KINDS:
                first, _ = present_to_device(ctx, a, *sizes, case, flags, dtype)
                second, _ = present_to_device(ctx, b, *sizes, case, flags, dtype)
                assert (first == second).all(), (sizes, case, flags)


def test_opaque_frames_against_the_colorbuf_path(ctx):
    """The bloom test scene as a Split frame presented at its own size, against the same frame's ColorBuf through the ColorBuf bloom path. Where the
    ColorBuf's t is 0 the two scene textures hold the same f16 texels, so B is the same and the images differ only by the f16 rounding of the
    composite's scene term: at most 2^-12 relative, under 0.03 of an sRGB8 level, so at most one threshold is crossed."""
    w, h = 128, 256
    n = w * h
    opt = to_abi(oracle.unaltered_colors(lighting=3), 0.25)
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, scenes.bloom_test_space())
    ctx.set_options(abi.LAYER_WORLD, opt)
    inv = np.ctypeslib.as_array(bloom_scene_camera().inverse_projection_view).copy()
    resident = device_bytes(n * 12)
    ctx.render_to_device(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_SPLIT), resident.data_ptr())
    cb = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_COLORBUF))["rgba8"]
    plain = ctx.render(ctx.make_frame(w, h, world_inv=inv))["rgba8"]
    opaque = cb[..., 3] == 0.0
    print(f"share of pixels with t == 0: {float(opaque.mean()):.4f}")
    assert opaque.mean() >= 0.95
    bloomed, info = ctx.present_split(resident.data_ptr(), (w, h), (w, h), 0.25, opt.tone_mapping, opt.maximum_intensity)
    assert info.bloomed == 1
    probe = ctx.probe_bloom(cb, 1.0, opt)
    diff = np.abs(bloomed.astype(int) - probe.astype(int))[opaque]
    print(f"bloom 0.25 against aic_probe_bloom: exact {float((diff == 0).all(-1).mean()):.4f}, max {int(diff.max())}")
    assert diff.max() <= 1
    assert (bloomed != plain).any()
    unbloomed, info = ctx.present_split(resident.data_ptr(), (w, h), (w, h), 0.0, opt.tone_mapping, opt.maximum_intensity)
    assert info.bloomed == 0
    diff = np.abs(unbloomed.astype(int) - plain.astype(int))[opaque]
    print(f"bloom 0 against aic_render: exact {float((diff == 0).all(-1).mean()):.4f}, max {int(diff.max())}")
    assert diff.max() <= 1


def test_the_loop_through_the_host_mirror():
    """draw_split -> reproject_split -> trace_pixels_into every pixel -> present_split: at the frame's size the window shows draw() of the new camera;
    at twice the size it shows the restatement's stretch of the resident bytes."""
    import all_is_cubes_amd as A

    w, h = 40, 24
    n = w * h
    cams = H.StandardCameras()
    o = H.GraphicsOptions()
    o.bloom_intensity = 0.0
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(scenes.one_cube_space())
    cams.world_view_transform = H.look_at_y_up((0.7, 0.9, 2.5), (0.5, 0.5, 0.5))
    r = H.HipRtRenderer(cams)
    r.update()
    first = r.draw_split()
    traced_with = r.world_camera()
    src = to_device(split_bytes(first))
    cams.world_view_transform = H.look_at_y_up((0.9, 1.0, 2.3), (0.45, 0.5, 0.5))
    r.update()
    resident = device_bytes(n * 12)
    r.reproject_split(src.data_ptr(), resident.data_ptr(), traced_with)
    every = to_device(np.arange(n, dtype=np.uint32))
    r.trace_pixels_into(resident.data_ptr(), every.data_ptr(), n)
    small = r.present_split(resident.data_ptr(), w, h)
    large = r.present_split(resident.data_ptr(), 2 * w, 2 * h)
    drawn = r.draw_rgba("")
    assert (small.width, small.height, large.width, large.height) == (w, h, 2 * w, 2 * h)
    diff = np.abs(small.data.astype(int) - drawn.data.astype(int))
    print(f"present at {w}x{h} against draw(): exact {float((diff == 0).all(-1).mean()):.4f}, max {int(diff.max())}")
    assert diff.max() <= 1
    bytes_now = resident.cpu().numpy()
    color = bytes_now[:n * 8].view(np.uint16).reshape(h, w, 4)
    assert (large.data == ref.present(color, (2 * w, 2 * h), 0.0, int(o.tone_mapping), o.maximum_intensity)).all()
    # the device form, both output kinds, with the options' bloom switched on
    o.bloom_intensity = 0.125
    cams.graphics_options = o
    r.update()
    for flags, dtype in KINDS:
        px = 4 * np.dtype(dtype).itemsize
        out = device_bytes(4 * n * px + GUARD)
        info = r.present_split(resident.data_ptr(), 2 * w, 2 * h, flags, out.data_ptr())
        assert info["bloomed"] == 1 and info["levels"] == bloom_ref.geometry(2 * w, 2 * h)[0]
        raw = out.cpu().numpy()
        assert (raw[4 * n * px:] == SENTINEL).all()
        got = raw[:4 * n * px].view(dtype).reshape(2 * h, 2 * w, 4)
        want = ref.present(color, (2 * w, 2 * h), 0.125, int(o.tone_mapping), o.maximum_intensity, out_f16=bool(flags))
        if flags:
            assert f16_ulps(got[..., :3].view(np.float16), want[..., :3].view(np.float16)).max() <= 2 and (got[..., 3] == ref.ONE_F16).all()
        else:
            assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    assert (resident.cpu().numpy() == bytes_now).all()


def test_rejections_leave_the_context_usable(ctx):
    import torch

    src_size, out_size = (17, 9), (33, 20)
    n_src, n_out = 17 * 9, 33 * 20
    color, depth, parts = restated(src_size, out_size)
    case = (0.25, 1, 1.0)
    want = ref.composite(parts["S"], parts["B"], *case)
    src_bytes = frame_bytes(color, depth)
    src = to_device(src_bytes)
    out = device_bytes(n_out * 8 + GUARD)
    assert src.data_ptr() % 8 == 0 and out.data_ptr() % 8 == 0

    def good(what):
        got, _ = present_to_device(ctx, src, src_size, out_size, case, 0, np.uint8)
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, what

    def call(src_ptr=None, out_ptr=None, src_size=src_size, out_size=out_size, i=0.25, tm=1, mi=1.0, flags=0):
        ctx.present_split(src.data_ptr() if src_ptr is None else src_ptr, src_size, out_size, i, tm, mi, flags=flags,
                          out_device=out.data_ptr() if out_ptr is None else out_ptr)

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert (out.cpu().numpy() == SENTINEL).all(), what
        good(what)

    def desc(**kw):
        d = abi.PresentDesc()
        d.src_width, d.src_height, d.out_width, d.out_height = *src_size, *out_size
        d.bloom_intensity, d.tone_mapping, d.maximum_intensity, d.flags = 0.25, 1, 1.0, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def raw_call(desc_ptr, src_ptr, out_ptr, is_device=1):
        info = abi.PresentInfo()
        ctx._check(ctx._lib.aic_present_split(ctx._h, desc_ptr, C.c_void_p(src_ptr), C.c_void_p(out_ptr), is_device, C.byref(info)))

    good("before")
    # a frame still occupying slot 0
    ctx.upload_space(abi.LAYER_WORLD, scenes.one_cube_space())
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    eye = (0.7, 0.9, 2.5)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, 40 / 24, oracle.look_at_y_up(eye, (0.5, 0.5, 0.5)), eye)
    busy = device_bytes(40 * 24 * 4)
    ctx.render_submit(ctx.make_frame(40, 24, world_inv=inv), busy.data_ptr(), 0)
    with pytest.raises(abi.AicError) as err:
        call()
    assert err.value.code == AIC_ERR_INVALID, "slot 0 busy"
    ctx.render_wait(0)
    ctx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    good("after slot 0 busy")
    # NULL pointers
    rejected(lambda: raw_call(None, src.data_ptr(), out.data_ptr()), "NULL desc")
    rejected(lambda: raw_call(C.byref(desc()), None, out.data_ptr()), "NULL src")
    rejected(lambda: raw_call(C.byref(desc()), src.data_ptr(), None), "NULL device out")
    rejected(lambda: raw_call(C.byref(desc()), src.data_ptr(), None, 0), "NULL host out")
    # src off an 8-byte boundary; a device out off its element's boundary
    wide_src = to_device(np.concatenate([src_bytes, np.zeros(16, np.uint8)]))
    rejected(lambda: call(src_ptr=wide_src.data_ptr() + 4), "src at 4 bytes")
    rejected(lambda: call(out_ptr=out.data_ptr() + 2), "RGBA8 out at 2 bytes")
    rejected(lambda: call(out_ptr=out.data_ptr() + 4, flags=abi.PRESENT_OUT_F16), "f16 out at 4 bytes")
    # a device out overlapping src: its colour plane, its depth plane, or src starting inside out
    both = device_bytes(n_src * 12 + n_out * 8)
    rejected(lambda: call(src_ptr=both.data_ptr(), out_ptr=both.data_ptr()), "out == src")
    rejected(lambda: call(src_ptr=both.data_ptr(), out_ptr=both.data_ptr() + n_src * 12 - 4), "out starts in src's depth plane")
    rejected(lambda: call(src_ptr=both.data_ptr() + n_out * 4 - 8, out_ptr=both.data_ptr()), "src starts inside out")
    rejected(lambda: call(src_ptr=both.data_ptr() + n_out * 8 - 8, out_ptr=both.data_ptr(), flags=abi.PRESENT_OUT_F16), "src starts inside an f16 out")
    assert (both.cpu().numpy() == SENTINEL).all()
    # a dimension above 65535; more output pixels than the kernels' 32-bit texel indices address; nothing to fill the output from
    rejected(lambda: call(src_size=(65536, 1)), "src width above 65535")
    rejected(lambda: call(src_size=(1, 65536)), "src height above 65535")
    rejected(lambda: call(out_size=(65536, 1)), "out width above 65535")
    rejected(lambda: call(out_size=(1, 65536)), "out height above 65535")
    rejected(lambda: call(out_size=(65535, 32769)), "more than 2^31 output pixels")
    for empty in ((0, 9), (17, 0), (0, 0)):
        rejected(lambda: call(src_size=empty), f"src {empty} with a non-empty output")
    # bloom_intensity NaN, negative or infinite; maximum_intensity NaN or negative; tone_mapping other than 0 or 1; unknown flag bits
    for bad in (float("nan"), -0.125, float("inf"), float("-inf")):
        rejected(lambda: call(i=bad), f"bloom_intensity {bad}")
    for bad in (float("nan"), -1.0, float("-inf")):
        rejected(lambda: call(mi=bad), f"maximum_intensity {bad}")
    for bad in (2, -1, 1 << 30):
        rejected(lambda: call(tm=bad), f"tone_mapping {bad}")
    for bad in (2, 1 << 31, 3):
        rejected(lambda: call(flags=bad), f"flags {bad}")
    # an empty output: AIC_OK, nothing written, the info zeroed -- whatever the source's size
    for ow, oh in ((0, 20), (33, 0), (0, 0)):
        for sw, sh in (src_size, (0, 0)):
            d = desc(src_width=sw, src_height=sh, out_width=ow, out_height=oh)
            info = abi.PresentInfo()
            C.memset(C.byref(info), 0xFF, C.sizeof(info))
            ctx._check(ctx._lib.aic_present_split(ctx._h, C.byref(d), C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), 1, C.byref(info)))
            assert bytes(info) == bytes(C.sizeof(info))
            assert (out.cpu().numpy() == SENTINEL).all() and (src.cpu().numpy() == src_bytes).all()
    good("after the empty outputs")
    torch.cuda.synchronize()
