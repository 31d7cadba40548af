"""GPU tests (-m gpu) of aic_export_split: a resident Split frame exported as sRGB8 colour and metric depth (all-is-cubes-gpu/src/rerun_image.rs:62-225,
shaders/rerun-copy.wgsl).

Yardstick: tests/export_ref.py, the NumPy restatement of DESIGN.md 4.15. Every comparison is bit for bit: each operation is an f32 with a single rounding,
and the same device code (the stretch, the encoder, the linearisation) is held to NumPy that way by the presentation and reprojection tests. Frames are
at most 96 x 64; the restatement of a (frame, size) pair is computed once and shared. The one exception to "bit for bit" is the payload of a NaN depth
(same_bits below)."""
import ctypes as C
import functools

import numpy as np
import pytest

from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import export_ref as ref
from tests import reproject_ref, scenes
from tests import test_gpu_split as split
from tests.test_gpu_reproject import GUARD, SENTINEL, device_bytes, frame_bytes, split_bytes, to_device

pytestmark = pytest.mark.gpu

F = np.float32
AIC_ERR_INVALID = 1
MARKER = (0, 0, 0, 0xBC00)
IPZW = (0.25, -1.0, 1.0, 0.5)
# (source, output): one texel; one texel stretched; a frame into one pixel; one row and one column by fractional ratios across several blocks; odd sizes by
# a fractional ratio; an output of exactly one 256-thread block (and a source row of one texel per four pixels)
SIZES = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((5, 3), (1, 1)), ((64, 1), (257, 1)), ((1, 64), (1, 255)), ((33, 17), (65, 31)), ((33, 17), (33, 17)), ((16, 4), (64, 4))]
SPECIAL_DEPTHS = np.array([1.0, np.nextafter(F(1.0), F(0.0)), 0.0, -0.0, -0.5, np.nan, np.inf, 1e-40, 0.5, 0.999], F)  # (1e-40: a subnormal)


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def synthetic_frame(w, h):
    """(colour [h, w, 4] u16, depth [h, w] f32): colour halves random in [0, 4) with 0, 65504 and +inf among them, alpha random in [0, 1] with marker
    texels beside valid ones; depths random in [0, 1) with every special value in SPECIAL_DEPTHS placed first (as far as the frame has room), a tenth of
    the rest negative. No NaN colours."""
    rng = np.random.default_rng(3000 * w + h)
    color = (rng.random((h, w, 4)) * 4).astype(np.float16).view(np.uint16)
    color[..., 3] = rng.random((h, w)).astype(np.float16).view(np.uint16)
    pick = rng.random((h, w, 3))
    color[..., :3][pick < 0.05] = 0
    color[..., :3][(pick >= 0.05) & (pick < 0.08)] = 0x7BFF
    color[..., :3][(pick >= 0.08) & (pick < 0.11)] = 0x7C00
    depth = rng.random((h, w)).astype(F)
    depth[rng.random((h, w)) < 0.1] *= F(-1.0)
    flat_d, flat_c = depth.reshape(-1), color.reshape(-1, 4)
    n = min(len(SPECIAL_DEPTHS), flat_d.size)
    flat_d[:n] = SPECIAL_DEPTHS[:n]
    if flat_d.size >= 4:
        flat_c[rng.random(flat_d.size) < 0.1] = MARKER
        flat_c[:n] = h16(0.5, 1.0, 2.0, 1.0)  # the special depths under valid texels ...
        flat_c[flat_d.size // 2] = MARKER        # ... and a marker over a plain depth beside them
        flat_d[flat_d.size // 2] = F(0.25)
    return color, depth


def h16(*values):
    return np.array(values, np.float16).view(np.uint16)


@functools.lru_cache(maxsize=None)
def restated(src, out):
    color, depth = synthetic_frame(*src)
    want = ref.export(color, depth, IPZW, out)
    for a in (color, depth, want[0], want[1]):
        a.setflags(write=False)
    return color, depth, want


def same_bits(a, b):
    """Two depth planes hold the same bit patterns; where both hold a NaN (the +inf depth texel unprojects to inf / inf) any NaN equals any other: IEEE 754
    leaves the sign and payload of an invalid operation's result to the implementation, and NumPy's own differ between host architectures."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def stats_of(info):
    return (info.n_surface, F(info.depth_min), F(info.depth_max))


def assert_stats(info, want, what):
    got = stats_of(info)
    assert got[0] == want[0] and got[1].view(np.uint32) == F(want[1]).view(np.uint32) and got[2].view(np.uint32) == F(want[2]).view(np.uint32), (what, got, want)


def export_to_device(ctx, src, src_size, out_size, ipzw, color=True, depth=True):
    """One call into fresh sentinel-filled device planes with guard bytes before and after each: (colour or None, depth or None, info)."""
    n = out_size[0] * out_size[1]
    bufs = [device_bytes(GUARD + n * 4 + GUARD) if wanted else None for wanted in (color, depth)]
    ptrs = [b.data_ptr() + GUARD if b is not None else 0 for b in bufs]
    none_c, none_d, info = ctx.export_split(src.data_ptr(), src_size, out_size, ipzw, device_outs=ptrs)
    assert none_c is None and none_d is None
    planes = []
    for b, dtype, shape in zip(bufs, (np.uint8, F), ((out_size[1], out_size[0], 4), (out_size[1], out_size[0]))):
        if b is None:
            planes.append(None)
            continue
        raw = b.cpu().numpy()
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + n * 4:] == SENTINEL).all(), "guard bytes around a plane"
        planes.append(raw[GUARD:GUARD + n * 4].view(dtype).reshape(shape))
    return planes[0], planes[1], info


@pytest.mark.parametrize("src_size,out_size", SIZES)
def test_synthetic_frames_equal_the_restatement(ctx, src_size, out_size):
    color, depth, (want_c, want_z, want_stats) = restated(src_size, out_size)
    what = f"{src_size} -> {out_size}"
    src_bytes = frame_bytes(color, depth)
    src = to_device(src_bytes)
    got_c, got_z, info = ctx.export_split(src.data_ptr(), src_size, out_size, IPZW)
    print(f"{what}: n_surface {info.n_surface} of {out_size[0] * out_size[1]}, depth {info.depth_min} .. {info.depth_max}, zeros {int((got_z == 0).sum())}")
    assert got_c.dtype == np.uint8 and (got_c == want_c).all(), what
    assert got_z.dtype == F and same_bits(got_z, want_z), (what, np.argwhere(got_z.view(np.uint32) != want_z.view(np.uint32))[:4].tolist())
    assert_stats(info, want_stats, what)
    # colour is the presentation's, byte for byte
    shown, _ = ctx.present_split(src.data_ptr(), src_size, out_size, 0.0, 0, np.inf)
    assert (got_c == shown).all(), what
    # plane combinations and targets: the same planes and the same statistics
    for kw in ({"depth": False}, {"color": False}, {"color": False, "depth": False}):
        c2, z2, i2 = ctx.export_split(src.data_ptr(), src_size, out_size, IPZW, **kw)
        assert (c2 is None) == (not kw.get("color", True)) and (z2 is None) == (not kw.get("depth", True))
        assert (c2 is None or (c2 == got_c).all()) and (z2 is None or same_bits(z2, got_z)), (what, kw)
        assert_stats(i2, want_stats, (what, kw))
        c3, z3, i3 = export_to_device(ctx, src, src_size, out_size, IPZW, **kw)
        assert (c3 is None or (c3 == got_c).all()) and (z3 is None or same_bits(z3, got_z)), (what, kw, "device")
        assert_stats(i3, want_stats, (what, kw, "device"))
    c4, z4, i4 = export_to_device(ctx, src, src_size, out_size, IPZW)
    assert (c4 == got_c).all() and same_bits(z4, got_z)
    assert_stats(i4, want_stats, (what, "device"))
    assert (src.cpu().numpy() == src_bytes).all(), "src changed"


def test_the_synthetic_frames_hold_what_they_are_for():
    """(no device needed) every rule decides some pixel of the restatement, and the special depths are there."""
    color, depth, (_, z, stats) = restated((33, 17), (65, 31))
    bits = depth.view(np.uint32)
    assert (depth == 1.0).any() and (depth == np.nextafter(F(1.0), F(0.0))).any() and (bits == 0x80000000).any() and (bits == 0).any()
    assert np.isnan(depth).any() and np.isposinf(depth).any() and ((depth > 0) & (depth < 1e-38)).any() and (depth == -0.5).any()
    valid = reproject_ref.valid(color)
    assert (~valid).any() and (~valid & (depth > 0) & (depth < 1)).any() and (valid & (depth > 0) & (depth < 1)).any()
    for value in (0, 0x7BFF, 0x7C00):
        assert (color[..., :3] == value).any()
    assert not np.isnan(color.view(np.float16)).any()
    assert 0 < stats[0] < z.size and (z == 0).any() and 0 < stats[1] < stats[2]
    # the subnormal texel is a surface at -b / e = 2 (d / 4 - 1 rounds to -1, d + 1 / 2 to 1 / 2); the +inf texel gives inf / inf, a NaN exported as it is
    one = h16(0, 0, 0, 1).reshape(1, 1, 4)
    assert ref.depth(one, np.array([[1e-40]], F), IPZW, 1, 1)[0, 0] == 2.0
    assert np.isnan(ref.depth(one, np.array([[np.inf]], F), IPZW, 1, 1)[0, 0])


def test_a_frame_with_no_surface(ctx):
    w, h = 33, 17
    color, _ = synthetic_frame(w, h)
    depth = np.where(np.arange(w * h).reshape(h, w) % 3 == 0, F(1.0), np.where(np.arange(w * h).reshape(h, w) % 3 == 1, F(-0.25), F(np.nan))).astype(F)
    src = to_device(frame_bytes(color, depth))
    for out_size in ((w, h), (65, 31)):
        got_c, got_z, info = ctx.export_split(src.data_ptr(), (w, h), out_size, IPZW)
        assert (got_z.view(np.uint32) == 0).all()
        assert stats_of(info) == (0, F(0.0), F(0.0)) and np.signbit(F(info.depth_min)) == np.signbit(F(info.depth_max)) == False  # noqa: E712
        assert (got_c == ref.color(color, *out_size)).all()
        _, _, info = ctx.export_split(src.data_ptr(), (w, h), out_size, IPZW, color=False, depth=False)
        assert stats_of(info) == (0, F(0.0), F(0.0))


@functools.lru_cache(maxsize=None)
def traced_case():
    """ui_over_world's options, the mirror's camera for them, and which pixels show a surface of the world (from the oracle, not from the frame)."""
    name = "ui_over_world"
    _, _, opt, _, _ = split.case(name)
    o = H.GraphicsOptions()
    o.view_distance = opt.view_distance
    camera = H.Camera(o, H.Viewport.with_scale(1.0, split.W, split.HT))
    depth, layer, _ = split.expected_split(name)
    return tuple(camera.depth_transform_zw()), np.array(camera.inverse_projection_zw(), F), (layer == 1) & np.isfinite(depth), float(opt.view_distance)


def test_a_traced_frame(ctx):
    name = "ui_over_world"
    zw, ipzw, world_surface, view_distance = traced_case()
    w, h = split.W, split.HT
    frame = split.load(ctx, name, flags=abi.FRAME_OUT_SPLIT)
    resident = device_bytes(w * h * 12)
    ctx.set_depth_transform(zw)
    try:
        ctx.render_to_device(frame, resident.data_ptr())
    finally:
        ctx.set_depth_transform(split.ZW_DEFAULT)
    raw = resident.cpu().numpy()
    color = raw[:w * h * 8].view(np.uint16).reshape(h, w, 4)
    depth = raw[w * h * 8:].view(F).reshape(h, w)
    assert world_surface.any() and not world_surface.all()
    for out_size in ((w, h), (37, 23), (131, 77)):
        want_c, want_z, want_stats = ref.export(color, depth, ipzw, out_size)
        got_c, got_z, info = ctx.export_split(resident.data_ptr(), (w, h), out_size, ipzw)
        shown, _ = ctx.present_split(resident.data_ptr(), (w, h), out_size, 0.0, 0, np.inf)
        print(f"{name} -> {out_size}: n_surface {info.n_surface}, depth {info.depth_min} .. {info.depth_max}")
        assert (got_c == shown).all() and (got_c == want_c).all(), out_size
        assert same_bits(got_z, want_z), out_size
        assert_stats(info, want_stats, out_size)
        # world pixels carry a positive distance not above the view distance; UI and sky pixels carry 0
        iy, ix = ref.nearest(w, h, *out_size)
        surface = world_surface[iy, ix]
        assert (got_z[surface] > 0).all() and (got_z[surface] <= F(view_distance)).all(), out_size
        assert (got_z[~surface].view(np.uint32) == 0).all(), out_size
        assert info.n_surface == int(surface.sum())
    assert (resident.cpu().numpy() == raw).all(), "src changed"


def host_renderer(w, h):
    import all_is_cubes_amd as A

    cams = H.StandardCameras()
    o = H.GraphicsOptions()
    o.bloom_intensity = 0.0
    o.fov_y = 60.0
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(scenes.one_cube_space())
    cams.world_view_transform = H.look_at_y_up((0.7, 0.9, 2.5), (0.5, 0.5, 0.5))
    r = H.HipRtRenderer(cams)
    r.update()
    return cams, r


def test_a_reprojected_frame_with_markers(ctx):
    """A sparse frame -- a patch of surface, NaN depth (nothing drawn) everywhere else -- reprojected: the gap fill reaches only so far, and the frame keeps
    the marker texel over most of its area (2352 of 3072 by tests/reproject_ref.py). Marker pixels export depth 0, whatever the depth plane holds there."""
    from tests.test_gpu_reproject import matrix
    from tests.test_gpu_reproject import synthetic_frame as reproject_frame

    w, h = 64, 48
    color, depth = reproject_frame(w, h)
    sparse = np.full((h, w), np.nan, F)
    sparse[4:12, 5:14] = depth[4:12, 5:14]
    m, zw = matrix("identity", w, h)
    src = to_device(frame_bytes(color, sparse))
    dst = device_bytes(w * h * 12)
    info = ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr(), 0)
    now = dst.cpu().numpy()
    got_color = now[:w * h * 8].view(np.uint16).reshape(h, w, 4)
    got_depth = now[w * h * 8:].view(F).reshape(h, w).copy()
    markers = ~reproject_ref.valid(got_color)
    print(f"reprojected: {int(markers.sum())} marker texels of {w * h} (n_unfilled {info.n_unfilled})")
    assert markers.any() and not markers.all() and int(markers.sum()) == info.n_unfilled
    assert (got_depth[markers] == 1.0).all()
    for out_size in ((w, h), (37, 23)):
        iy, ix = ref.nearest(w, h, *out_size)
        want_c, want_z, want_stats = ref.export(got_color, got_depth, zw, out_size)
        got_c, got_z, einfo = ctx.export_split(dst.data_ptr(), (w, h), out_size, zw)
        assert (got_c == want_c).all() and same_bits(got_z, want_z)
        assert_stats(einfo, want_stats, out_size)
        assert (got_z[markers[iy, ix]].view(np.uint32) == 0).all()
    # the same frame with a plain depth under every marker: it is the marker that decides, not the far plane's 1.0
    got_depth[markers] = F(0.5)
    again = to_device(frame_bytes(got_color, got_depth))
    for out_size in ((w, h), (37, 23)):
        iy, ix = ref.nearest(w, h, *out_size)
        _, got_z, einfo = ctx.export_split(again.data_ptr(), (w, h), out_size, zw)
        assert same_bits(got_z, ref.depth(got_color, got_depth, zw, *out_size))
        assert (got_z[markers[iy, ix]].view(np.uint32) == 0).all()
        assert einfo.n_surface <= int((~markers[iy, ix]).sum())


def test_the_mirror_returns_what_the_reference_attaches(ctx):
    w, h = 96, 64
    cams, r = host_renderer(w, h)
    first = r.draw_split()
    resident = to_device(split_bytes(first))
    camera = r.world_camera()
    ipzw = np.array(camera.inverse_projection_zw(), F)
    e = r.export_split(resident.data_ptr())
    assert e["size"] == abi.export_size((w, h)) == (w, h)  # under the cap: the frame's size
    want_c, want_z, info = ctx.export_split(resident.data_ptr(), (w, h), (w, h), ipzw)
    assert (e["color"] == want_c).all() and same_bits(e["depth"], want_z)
    color = first.color_f16_bits
    rc, rz, rstats = ref.export(color, first.depth, ipzw, (w, h))
    assert (want_c == rc).all() and same_bits(want_z, rz)
    assert (e["n_surface"], F(e["depth_min"]), F(e["depth_max"])) == stats_of(info) == rstats and e["n_surface"] > 0
    matrix, resolution, transform = e["pinhole"]
    assert (matrix.view(np.uint32) == ref.pinhole(60.0, w, h).view(np.uint32)).all() and resolution.tolist() == [float(w), float(h)]
    assert transform.rotation == camera.view_transform().rotation and transform.translation == camera.view_transform().translation
    assert e["depth_range"] == (camera.near_plane_distance(), camera.view_distance()) == (1.0 / 32.0, 200.0)
    # a size given: the pinhole is the world camera's with its viewport set to that size
    e2 = r.export_split(resident.data_ptr(), (37, 23))
    c2, z2, _ = ctx.export_split(resident.data_ptr(), (w, h), (37, 23), ipzw)
    assert e2["size"] == (37, 23) and (e2["color"] == c2).all() and same_bits(e2["depth"], z2)
    assert (e2["pinhole"][0].view(np.uint32) == ref.pinhole(60.0, 37, 23).view(np.uint32)).all() and e2["pinhole"][1].tolist() == [37.0, 23.0]
    # the unit cube at the origin seen from (0.7, 0.9, 2.5): along the view axis its corners lie between 1.41 (1, 1, 1) and 2.6 (0, 0, 0)
    assert 1.3 < e["depth_min"] < e["depth_max"] < 2.7


def test_rejections_leave_the_context_usable(ctx):
    import oracle

    src_size, out_size = (33, 17), (65, 31)
    n_src, n_out = 33 * 17, 65 * 31
    color, depth, (want_c, want_z, want_stats) = restated(src_size, out_size)
    src_bytes = frame_bytes(color, depth)
    src = to_device(src_bytes)
    outs = device_bytes(2 * n_out * 4 + GUARD)
    color_ptr, depth_ptr = outs.data_ptr(), outs.data_ptr() + n_out * 4
    assert src.data_ptr() % 8 == 0 and outs.data_ptr() % 8 == 0
    # the render whose result must not change
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, scenes.one_cube_space())
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    eye = (0.7, 0.9, 2.5)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, 40 / 24, oracle.look_at_y_up(eye, (0.5, 0.5, 0.5)), eye)
    frame = ctx.make_frame(40, 24, world_inv=inv)
    before = ctx.render(frame)["rgba8"].copy()

    def desc(**kw):
        d = abi.ExportDesc()
        d.src_width, d.src_height, d.out_width, d.out_height = *src_size, *out_size
        d.inverse_projection_zw[:] = IPZW
        for k, v in kw.items():
            if k == "ipzw":
                d.inverse_projection_zw[:] = v
            else:
                setattr(d, k, v)
        return d

    def raw_call(d, src_ptr, c_ptr, z_ptr, is_device=1, want_info=True):
        info = abi.ExportInfo()
        ctx._check(ctx._lib.aic_export_split(ctx._h, C.byref(d) if d is not None else None, C.c_void_p(src_ptr), C.c_void_p(c_ptr), C.c_void_p(z_ptr), is_device,
                                             C.byref(info) if want_info else None))
        return info

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert "aic_export_split" in str(err.value), what
        assert (outs.cpu().numpy() == SENTINEL).all(), what
        assert (ctx.render(frame)["rgba8"] == before).all(), what

    s = src.data_ptr()
    # a frame still occupying slot 0
    busy = device_bytes(40 * 24 * 4)
    ctx.render_submit(frame, busy.data_ptr(), 0)
    with pytest.raises(abi.AicError) as err:
        raw_call(desc(), s, color_ptr, depth_ptr)
    assert err.value.code == AIC_ERR_INVALID and "slot 0" in str(err.value)
    ctx.render_wait(0)
    ctx.synchronize()
    assert (busy.cpu().numpy().view(np.uint8).reshape(24, 40, 4) == before).all() and (outs.cpu().numpy() == SENTINEL).all()
    # NULL desc or src; nothing asked for
    rejected(lambda: raw_call(None, s, color_ptr, depth_ptr), "NULL desc")
    rejected(lambda: raw_call(desc(), None, color_ptr, depth_ptr), "NULL src")
    rejected(lambda: raw_call(desc(), s, None, None, 1, False), "all three NULL")
    rejected(lambda: raw_call(desc(), s, None, None, 0, False), "all three NULL, host")
    # alignment
    wide_src = to_device(np.concatenate([src_bytes, np.zeros(16, np.uint8)]))
    rejected(lambda: raw_call(desc(), wide_src.data_ptr() + 4, color_ptr, depth_ptr), "src at 4 bytes")
    rejected(lambda: raw_call(desc(), s, color_ptr + 2, depth_ptr), "color_out at 2 bytes")
    rejected(lambda: raw_call(desc(), s, color_ptr, depth_ptr + 1), "depth_out at 1 byte")
    rejected(lambda: raw_call(desc(), s, None, depth_ptr + 2), "depth_out alone at 2 bytes")
    # overlaps: with src's colour plane, its depth plane, src starting inside an output, the outputs with each other
    both = device_bytes(n_src * 12 + 2 * n_out * 4)
    b = both.data_ptr()
    rejected(lambda: raw_call(desc(), b, b, depth_ptr), "color_out == src")
    rejected(lambda: raw_call(desc(), b, color_ptr, b + n_src * 12 - 4), "depth_out starts in src's depth plane")
    rejected(lambda: raw_call(desc(), b + n_out * 4 - 8, b, depth_ptr), "src starts inside color_out")
    rejected(lambda: raw_call(desc(), b + n_out * 4 - 8, None, b), "src starts inside depth_out, no colour")
    rejected(lambda: raw_call(desc(), s, color_ptr, color_ptr), "depth_out == color_out")
    rejected(lambda: raw_call(desc(), s, color_ptr + n_out * 4 - 4, color_ptr), "color_out starts in depth_out's last word")
    assert (both.cpu().numpy() == SENTINEL).all()
    # sizes
    rejected(lambda: raw_call(desc(src_width=65536, src_height=1), s, color_ptr, depth_ptr), "src width above 65535")
    rejected(lambda: raw_call(desc(src_width=1, src_height=65536), s, color_ptr, depth_ptr), "src height above 65535")
    rejected(lambda: raw_call(desc(out_width=65536, out_height=1), s, color_ptr, depth_ptr), "out width above 65535")
    rejected(lambda: raw_call(desc(out_width=1, out_height=65536), s, color_ptr, depth_ptr), "out height above 65535")
    rejected(lambda: raw_call(desc(out_width=65535, out_height=32769), s, color_ptr, depth_ptr), "more than 2^31 output pixels")
    for empty in ((0, 17), (33, 0), (0, 0)):
        rejected(lambda: raw_call(desc(src_width=empty[0], src_height=empty[1]), s, color_ptr, depth_ptr), f"src {empty} with a non-empty output")
    # a non-finite component of inverse_projection_zw; unknown flag bits
    for at in range(4):
        for bad in (float("nan"), float("inf"), float("-inf")):
            zw = list(IPZW)
            zw[at] = bad
            rejected(lambda: raw_call(desc(ipzw=zw), s, color_ptr, depth_ptr), f"ipzw[{at}] = {bad}")
    for bad in (1, 2, 1 << 31):
        rejected(lambda: raw_call(desc(flags=bad), s, color_ptr, depth_ptr), f"flags {bad}")
    # an empty output: AIC_OK, nothing written, the info zeroed -- whatever the source's size, even where the pointers would overlap
    for ow, oh in ((0, 31), (65, 0), (0, 0)):
        for sw, sh in (src_size, (0, 0)):
            d = desc(src_width=sw, src_height=sh, out_width=ow, out_height=oh)
            info = abi.ExportInfo()
            C.memset(C.byref(info), 0xFF, C.sizeof(info))
            ctx._check(ctx._lib.aic_export_split(ctx._h, C.byref(d), C.c_void_p(s), C.c_void_p(color_ptr), C.c_void_p(depth_ptr), 1, C.byref(info)))
            assert bytes(info) == bytes(C.sizeof(info))
            assert (outs.cpu().numpy() == SENTINEL).all() and (src.cpu().numpy() == src_bytes).all()
    # and the good call still gives what it gave
    info = raw_call(desc(), s, color_ptr, depth_ptr)
    raw = outs.cpu().numpy()
    assert (raw[:n_out * 4].reshape(out_size[1], out_size[0], 4) == want_c).all() and same_bits(raw[n_out * 4:2 * n_out * 4].view(F).reshape(out_size[1], out_size[0]), want_z)
    assert (raw[2 * n_out * 4:] == SENTINEL).all()
    assert_stats(info, want_stats, "after the rejections")
    assert (ctx.render(frame)["rgba8"] == before).all()
