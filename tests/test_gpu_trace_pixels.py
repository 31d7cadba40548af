"""GPU tests (-m gpu) of aic_trace_pixels: listed pixels of a frame traced into compact results or in place into a resident frame -- one round of
all-is-cubes-gpu's Inner::do_some_tracing (raytrace_to_texture.rs:591-751).

Yardstick: in every comparison the expected value is the aic_render frame for the same `frame` (pinned to the oracle by tests/test_gpu_parity.py,
tests/test_gpu_linear_parity.py and tests/test_gpu_split.py), byte for byte -- no tolerance: pixel (x, y) is the same arithmetic on the same inputs.
Scenes are tests/test_gpu_split.py's: ui_over_world_antialiased and backdrop (two layers, four samples, a backdrop), half_transparent_slab, no_world.
Frames: 40 x 24 (partial 8 x 8 tiles) and 64 x 40 = 2560 pixels (a list can exceed one 2048-column row of the batch's image)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import scenes
from tests.test_gpu_parity import to_abi_options
from tests.test_gpu_split import case

pytestmark = pytest.mark.gpu

WORLD_EXPOSURE, UI_EXPOSURE = 0.5, 2.0
SENTINEL = 0xA5
SCENES = ["ui_over_world_antialiased", "backdrop", "half_transparent_slab", "no_world"]
# kind -> (frame flag, bytes per pixel)
KINDS = {"rgba8": (0, 4), "linear": (abi.FRAME_OUT_LINEAR, 16), "colorbuf": (abi.FRAME_OUT_COLORBUF, 16), "split": (abi.FRAME_OUT_SPLIT, 12)}
AIC_ERR_INVALID, AIC_ERR_UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def ctx():
    o = H.GraphicsOptions()
    o.view_distance = 200.0
    c = abi.Context(0)
    c.set_depth_transform(tuple(H.Camera(o, H.Viewport.with_scale(1.0, 40, 24)).depth_transform_zw()))  # a projective depth, not the identity
    yield c
    c.close()


def load(ctx, name, w, h, flags=0, partition=None):
    """Uploads the case and returns its frame of w x h."""
    world, ui, opt, (eye, quat), backdrop = case(name)
    _, _, inv = oracle.camera_matrices(90.0, opt.view_distance, w / h, quat, eye)
    ui_inv = None
    if world is not None:
        ctx.upload_space(abi.LAYER_WORLD, world)
    else:
        ctx.clear_space(abi.LAYER_WORLD)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    if ui is not None:
        _, _, ui_inv = oracle.camera_matrices(90.0, opt.view_distance, w / h, (0, 0, 0, 1), (0, 0, 0))
        ctx.upload_space(abi.LAYER_UI, ui)
        ctx.set_options(abi.LAYER_UI, to_abi_options(opt))
    else:
        ctx.clear_space(abi.LAYER_UI)
    return ctx.make_frame(w, h, world_inv=inv, ui_inv=ui_inv, exposure=WORLD_EXPOSURE, ui_exposure=UI_EXPOSURE, backdrop=backdrop, flags=flags, partition=partition)


def device_bytes(n_bytes, fill=SENTINEL):
    import torch

    t = torch.full((int(n_bytes),), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def to_device(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def trace_device(ctx, frame, px, target, aux=None, in_place=False):
    """aic_trace_pixels with AIC_PIXELS_DEVICE: the list copied to the device (and kept there for the call), results into `target`."""
    dev = to_device(px)
    return ctx.trace_pixels_device(frame, len(px), dev.data_ptr(), target.data_ptr(), aux_ptr=aux.data_ptr() if aux is not None else 0, in_place=in_place)


def whole_frame(ctx, frame, kind):
    """The yardstick: aic_render of `frame` into device memory, as raw bytes in aic_render's layout."""
    npix = frame.width * frame.height
    buf = device_bytes(npix * KINDS[kind][1], 0)
    ctx.render_to_device(frame, buf.data_ptr())
    return buf.cpu().numpy()


def texels(raw, count, kind, px):
    """The bytes of pixels `px` out of a buffer laid out for `count` pixels, as the compact layout of len(px) results."""
    px = np.asarray(px, np.int64)
    if kind == "split":
        return np.concatenate([raw[:count * 8].reshape(count, 8)[px].reshape(-1), raw[count * 8:count * 12].reshape(count, 4)[px].reshape(-1)])
    bpp = KINDS[kind][1]
    return raw[:count * bpp].reshape(count, bpp)[px].reshape(-1)


def untouched_mask(count, kind, px, total_bytes):
    """Bytes of a frame buffer that a trace of `px` must leave alone."""
    m = np.ones(total_bytes, bool)
    px = np.asarray(px, np.int64)
    if kind == "split":
        m[:count * 8].reshape(count, 8)[px] = False
        m[count * 8:count * 12].reshape(count, 4)[px] = False
    else:
        bpp = KINDS[kind][1]
        m[:count * bpp].reshape(count, bpp)[px] = False
    return m


def shuffled_parts(count, seed):
    """A shuffled third of the pixels with five of them listed twice, and the rest."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(count).astype(np.uint32)
    subset = np.concatenate([perm[:count // 3], perm[:5]])
    rng.shuffle(subset)
    return subset, perm[count // 3:]


IN_PLACE_CASES = [(name, kind, 40, 24) for name in SCENES for kind in KINDS] + [("ui_over_world_antialiased", kind, 64, 40) for kind in KINDS]


@pytest.mark.parametrize("name,kind,w,h", IN_PLACE_CASES)
def test_in_place_writes_the_listed_texels_and_nothing_else(ctx, name, kind, w, h):
    count = w * h
    frame = load(ctx, name, w, h, flags=KINDS[kind][0])
    want = whole_frame(ctx, frame, kind)
    subset, rest = shuffled_parts(count, 11)
    target = device_bytes(want.size)
    info = trace_device(ctx, frame, subset, target, in_place=True)
    assert info.rows_rendered == len(subset) and info.variant == abi.VARIANT_RECORDING
    got = target.cpu().numpy()
    assert (texels(got, count, kind, subset) == texels(want, count, kind, subset)).all(), "the listed texels"
    assert (got[untouched_mask(count, kind, subset, got.size)] == SENTINEL).all(), "every other byte"
    trace_device(ctx, frame, rest, target, in_place=True)
    assert (target.cpu().numpy() == want).all(), "after the complement: the whole frame"


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ["ui_over_world_antialiased", "half_transparent_slab"])
def test_compact_results_in_list_order(ctx, name, kind):
    w, h = 64, 40
    count = w * h
    frame = load(ctx, name, w, h, flags=KINDS[kind][0])
    want = whole_frame(ctx, frame, kind)
    rng = np.random.default_rng(5)
    px = np.concatenate([rng.permutation(count), rng.integers(0, count, 40)]).astype(np.uint32)  # 2600 > 2048: two rows of the batch's image, the second partial
    expect = texels(want, count, kind, px)
    # a host list, host results
    got = ctx.trace_pixels(frame, px)
    assert got["info"].rows_rendered == len(px) and got["info"].variant == abi.VARIANT_RECORDING
    if kind == "split":
        raw = np.concatenate([got["color_f16"].reshape(-1).view(np.uint8), got["depth"].reshape(-1).view(np.uint8)])
    else:
        raw = got["rgba8"].reshape(-1).view(np.uint8)
    assert (raw == expect).all(), "host list"
    # a device list, a device target
    n_bytes = len(px) * KINDS[kind][1]
    target = device_bytes(n_bytes + 64)
    trace_device(ctx, frame, px, target)
    dev = target.cpu().numpy()
    assert (dev[:n_bytes] == expect).all(), "device list"
    assert (dev[n_bytes:] == SENTINEL).all(), "nothing past the n results"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
def test_list_lengths(ctx, n):
    w, h = 64, 40
    count = w * h
    px = np.random.default_rng(n).permutation(count)[:n].astype(np.uint32)
    split = load(ctx, "backdrop", w, h, flags=abi.FRAME_OUT_SPLIT)
    want = whole_frame(ctx, split, "split")
    got = ctx.trace_pixels(split, px)
    raw = np.concatenate([got["color_f16"].reshape(-1).view(np.uint8), got["depth"].reshape(-1).view(np.uint8)])
    assert (raw == texels(want, count, "split", px)).all(), "compact Split: the depth plane at n * 8"
    assert got["info"].rows_rendered == n
    plain = load(ctx, "backdrop", w, h)
    want = whole_frame(ctx, plain, "rgba8")
    target = device_bytes(want.size)
    trace_device(ctx, plain, px, target, in_place=True)
    dev = target.cpu().numpy()
    assert (texels(dev, count, "rgba8", px) == texels(want, count, "rgba8", px)).all()
    assert (dev[untouched_mask(count, "rgba8", px, dev.size)] == SENTINEL).all()


def test_an_empty_list_is_ok(ctx):
    frame = load(ctx, "backdrop", 40, 24, flags=abi.FRAME_OUT_SPLIT)
    got = ctx.trace_pixels(frame, np.zeros(0, np.uint32), want_aux=True)
    assert got["info"].rows_rendered == 0 and got["depth"].size == 0


@pytest.mark.parametrize("name", ["ui_over_world_antialiased", "half_transparent_slab"])
def test_aux_records_and_counters(ctx, name):
    w, h = 64, 40
    count = w * h
    frame = load(ctx, name, w, h, flags=abi.FRAME_COUNTERS)
    whole = ctx.render(frame, want_aux=True)
    want_aux = whole["aux"].reshape(-1)
    assert whole["info"].cubes_traced > 0
    rng = np.random.default_rng(3)
    px = np.concatenate([rng.permutation(count)[:2100], rng.integers(0, count, 30)]).astype(np.uint32)  # duplicates included, more than one batch row
    got = ctx.trace_pixels(frame, px, want_aux=True)
    assert (got["aux"] == want_aux[px]).all(), "aux[i] is the whole frame's record at pixels[i]"
    assert (got["rgba8"] == whole["rgba8"].reshape(-1, 4)[px]).all()
    assert got["info"].cubes_traced == int(got["aux"]["cubes_traced"].astype(np.uint64).sum()), "the sum over the list, duplicates included"
    # device pointers: the records go to the caller's buffer, in list order whatever the mode
    target = device_bytes(count * 4)
    aux_dev = device_bytes(len(px) * abi.PIXEL_AUX_DTYPE.itemsize)
    info = trace_device(ctx, frame, px, target, aux=aux_dev, in_place=True)
    assert (aux_dev.cpu().numpy().view(abi.PIXEL_AUX_DTYPE) == want_aux[px]).all()
    assert info.cubes_traced == got["info"].cubes_traced


def test_picker_driven_cycle_fills_the_frame(ctx):
    w, h = 48, 32
    count = w * h
    frame = load(ctx, "ui_over_world_antialiased", w, h, flags=abi.FRAME_OUT_SPLIT)
    want = whole_frame(ctx, frame, "split")
    order, central, cycle = abi.pixel_order(w, h)
    assert central == count // 4 and cycle == 2 * (count - central)
    k = np.arange(cycle, dtype=np.int64)
    picks = order[np.where(k % 2 == 0, (k // 2) % central, central + (k // 2) % (count - central))]  # the pick sequence of include/aic_hip.h
    target = device_bytes(want.size)
    for start in range(0, cycle, 1000):  # do_some_tracing: the next rays_per_frame pixels of the picker, stored in place
        chunk = picks[start:start + 1000]
        trace_device(ctx, frame, chunk, target, in_place=True)
    assert (target.cpu().numpy() == want).all()


def test_scene_change_between_batches(ctx):
    w, h = 40, 24
    count = w * h
    frame = load(ctx, "half_transparent_slab", w, h, flags=abi.FRAME_OUT_SPLIT)
    perm = np.random.default_rng(9).permutation(count).astype(np.uint32)
    first, second = perm[:count // 2], perm[count // 2:]
    want_a = whole_frame(ctx, frame, "split")
    target = device_bytes(want_a.size)
    trace_device(ctx, frame, first, target, in_place=True)
    ctx.update_cubes(abi.LAYER_WORLD, [[0, 2, 0]], [1])  # a second slab above the first (block 1 of scenes.half_transparent_slab_space)
    trace_device(ctx, frame, second, target, in_place=True)
    want_b = whole_frame(ctx, frame, "split")
    assert (want_a != want_b).any(), "the update changes the picture"
    got = target.cpu().numpy()
    assert (texels(got, count, "split", first) == texels(want_a, count, "split", first)).all(), "the first half: the scene before the update"
    assert (texels(got, count, "split", second) == texels(want_b, count, "split", second)).all(), "the second half: the scene after it"


@pytest.mark.parametrize("kind", ["rgba8", "split"])
def test_out_of_range_entry_in_a_device_list(ctx, kind):
    w, h = 40, 24
    count = w * h
    bpp = KINDS[kind][1]
    frame = load(ctx, "ui_over_world_antialiased", w, h, flags=KINDS[kind][0] | abi.FRAME_COUNTERS)
    want = whole_frame(ctx, frame, kind)
    px = np.random.default_rng(2).permutation(count).astype(np.uint32)
    bad_at = [0, 70, count - 1]
    listed = px.copy()
    listed[bad_at] = count  # the first index outside the frame
    valid = np.delete(px, bad_at)
    # in place: the target has one row more than the frame, so that even a wrong store lands inside the allocation
    target = device_bytes((h + 1) * w * bpp)
    aux_dev = device_bytes(count * abi.PIXEL_AUX_DTYPE.itemsize)
    info = trace_device(ctx, frame, listed, target, aux=aux_dev, in_place=True)
    got = target.cpu().numpy()
    assert (texels(got, count, kind, valid) == texels(want, count, kind, valid)).all(), "the frame's other texels"
    assert (got[untouched_mask(count, kind, valid, got.size)] == SENTINEL).all(), "the unlisted texels and the extra row"
    aux = aux_dev.cpu().numpy().view(abi.PIXEL_AUX_DTYPE)
    ok = np.ones(count, bool)
    ok[bad_at] = False
    assert info.cubes_traced == int(aux["cubes_traced"][ok].astype(np.uint64).sum()), "the entry counts nothing"
    assert (aux_dev.cpu().numpy().reshape(count, -1)[bad_at] == SENTINEL).all(), "and has no record"
    # compact: result i of such an entry is not stored
    compact = device_bytes(count * bpp + w * bpp)
    trace_device(ctx, frame, listed, compact)
    got = compact.cpu().numpy()
    idx = np.flatnonzero(ok)
    assert (texels(got, count, kind, idx) == texels(want, count, kind, valid)).all()
    assert (got[untouched_mask(count, kind, idx, got.size)] == SENTINEL).all()


def test_rejections_leave_the_context_usable(ctx):
    import torch

    w, h = 40, 24
    count = w * h
    name = "ui_over_world_antialiased"
    plain = load(ctx, name, w, h)
    before = ctx.render(plain)["rgba8"].copy()
    px = np.arange(16, dtype=np.uint32)
    px_dev = to_device(px)
    out_dev = device_bytes(count * 16 + 64)
    assert out_dev.data_ptr() % 16 == 0

    def rejected(code, fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == code, what
        assert (ctx.render(plain)["rgba8"] == before).all(), what
        assert (ctx.trace_pixels(plain, px)["rgba8"] == before.reshape(-1, 4)[px]).all(), what

    def raw_call(frame, n, pixels_ptr, mode, out_ptr):
        info = abi.FrameInfo()
        ctx._check(ctx._lib.aic_trace_pixels(ctx._h, C.byref(frame), n, C.c_void_p(pixels_ptr), mode, C.c_void_p(out_ptr), None, C.byref(info)))

    # slot 0 busy
    busy = device_bytes(count * 4)
    ctx.render_submit(plain, busy.data_ptr(), 0)
    with pytest.raises(abi.AicError) as err:
        ctx.trace_pixels(plain, px)
    assert err.value.code == AIC_ERR_INVALID, "slot 0 busy"
    ctx.render_wait(0)
    ctx.synchronize()
    assert (busy.cpu().numpy().reshape(h, w, 4) == before).all()
    # a host list holding an index >= width * height
    rejected(AIC_ERR_INVALID, lambda: ctx.trace_pixels(plain, np.array([0, count, 1], np.uint32)), "index out of range in a host list")
    # more than 2048 x 65535 pixels (checked before the list is looked at: a device list of 16 entries stands in)
    rejected(AIC_ERR_INVALID, lambda: ctx.trace_pixels_device(plain, abi.MAX_PIXELS + 1, px_dev.data_ptr(), out_dev.data_ptr()), "too many pixels")
    # width or height above 65535
    for ww, hh in ((65536, 1), (1, 65536)):
        wide = load(ctx, name, w, h)
        wide.width, wide.height = ww, hh
        rejected(AIC_ERR_INVALID, lambda: ctx.trace_pixels(wide, np.zeros(1, np.uint32)), "frame dimension above 65535")
    # in place without device pointers
    host_out = np.zeros(count, np.uint32)
    rejected(AIC_ERR_INVALID, lambda: raw_call(plain, len(px), px.ctypes.data, abi.PIXELS_IN_PLACE, host_out.ctypes.data), "in place needs device pointers")
    # Split combined with a float flag
    for other in (abi.FRAME_OUT_LINEAR, abi.FRAME_OUT_COLORBUF):
        f = load(ctx, name, w, h, flags=abi.FRAME_OUT_SPLIT | other)
        rejected(AIC_ERR_INVALID, lambda: ctx.trace_pixels(f, px), "Split with a float flag")
    # a misaligned device `out`: 8 bytes for Split, 16 for the float outputs
    f = load(ctx, name, w, h, flags=abi.FRAME_OUT_SPLIT)
    rejected(AIC_ERR_INVALID, lambda: ctx.trace_pixels_device(f, len(px), px_dev.data_ptr(), out_dev.data_ptr() + 4), "Split out at 4 bytes")
    for flag in (abi.FRAME_OUT_LINEAR, abi.FRAME_OUT_COLORBUF):
        f = load(ctx, name, w, h, flags=flag)
        rejected(AIC_ERR_INVALID, lambda: ctx.trace_pixels_device(f, len(px), px_dev.data_ptr(), out_dev.data_ptr() + 8, in_place=True), "float out at 8 bytes")
    # a negative or NaN exposure
    for bad in (-1.0, float("nan")):
        f = load(ctx, name, w, h)
        f.world.exposure = bad
        rejected(AIC_ERR_INVALID, lambda: ctx.trace_pixels(f, px), "world exposure")
        f = load(ctx, name, w, h)
        f.ui.exposure = bad
        rejected(AIC_ERR_INVALID, lambda: ctx.trace_pixels(f, px), "UI exposure")
    # bloom, a partition
    f = load(ctx, name, w, h, flags=abi.FRAME_BLOOM)
    rejected(AIC_ERR_UNSUPPORTED, lambda: ctx.trace_pixels(f, px), "bloom")
    f = load(ctx, name, w, h, partition=(8, 2, 0))
    rejected(AIC_ERR_UNSUPPORTED, lambda: ctx.trace_pixels(f, px), "a partition")
    # aic_trace_patches keeps its rejection of Split
    f = load(ctx, name, w, h, flags=abi.FRAME_OUT_SPLIT)
    rejected(AIC_ERR_UNSUPPORTED, lambda: ctx.trace_patches(f, [[-0.5, -0.5, 0.5, 0.5]]), "aic_trace_patches with Split")
    torch.cuda.synchronize()


def test_pixel_centers_follow_the_target_frame(ctx):
    """AIC_FRAME_PIXEL_CENTERS divides by the frame's width and height, not the batch's."""
    w, h = 40, 24
    count = w * h
    frame = load(ctx, "half_transparent_slab", w, h, flags=abi.FRAME_PIXEL_CENTERS)
    whole = ctx.render(frame, want_aux=True)
    px = np.random.default_rng(4).permutation(count)[:300].astype(np.uint32)
    got = ctx.trace_pixels(frame, px, want_aux=True)
    assert (got["rgba8"] == whole["rgba8"].reshape(-1, 4)[px]).all()
    assert (got["aux"] == whole["aux"].reshape(-1)[px]).all()


def test_host_mirror_trace_pixels(ctx):
    """HipRtRenderer::trace_pixels / trace_pixels_into: the texels of its own draw_split, and the bytes of the ctypes path."""
    import all_is_cubes_amd as A

    w, h = 40, 24
    count = w * h
    eye, target = (0.7, 0.9, 2.5), (0.5, 0.5, 0.5)
    world = scenes.one_cube_space()
    cams = H.StandardCameras()
    cams.graphics_options = H.GraphicsOptions()
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(world)
    cams.world_view_transform = H.look_at_y_up(eye, target)
    r = H.HipRtRenderer(cams)
    r.update()
    whole = r.draw_split()
    color, depth = whole.color_f16_bits.reshape(count, 4), whole.depth.reshape(count)
    picker = H.PixelPicker(w, h)
    px = picker.take(700)
    got = r.trace_pixels(px)
    assert (got["color_f16_bits"] == color[px]).all() and (got["depth"].view(np.uint32) == depth.view(np.uint32)[px]).all()
    assert got["info"].rows_rendered == len(px)
    # the ctypes path on a context of its own
    _, _, inv = oracle.camera_matrices(90.0, 200.0, w / h, oracle.look_at_y_up(eye, target), eye)
    ctx.upload_space(abi.LAYER_WORLD, world)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(oracle.make_options()))
    ctx.clear_space(abi.LAYER_UI)
    via_abi = ctx.trace_pixels(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_SPLIT), px, want_aux=True)
    assert (got["hits"].reshape(-1).view(abi.PIXEL_AUX_DTYPE) == via_abi["aux"]).all() and via_abi["aux"]["hit"].any()
    assert (got["color_f16_bits"] == via_abi["color_f16"].view(np.uint16)).all() and (got["depth"].view(np.uint32) == via_abi["depth"].view(np.uint32)).all()
    # in place into a resident frame: a whole cycle of the picker fills it
    resident = device_bytes(count * 12)
    rest = picker.take(picker.cycle_length())
    for chunk in (px, rest):
        dev = to_device(chunk)
        info = r.trace_pixels_into(resident.data_ptr(), dev.data_ptr(), len(chunk))
        assert info.rows_rendered == len(chunk)
    planes = abi.split_planes(resident.cpu().numpy(), h, w)
    assert (planes["color_f16"].view(np.uint16).reshape(count, 4) == color).all() and (planes["depth"].view(np.uint32).reshape(count) == depth.view(np.uint32)).all()
