"""GPU tests (-m gpu) of aic_reproject_split: a resident Split frame drawn into a new camera as depth-tested point sprites and gap-filled
(raytrace_to_texture.rs:433-540, shaders/rt-copy.wgsl:73-223, shaders/resampling.wgsl:119-176).

Yardstick: tests/reproject_ref.py, the NumPy restatement of DESIGN.md 4.10, bit for bit -- both planes compared as uint16 / uint32 patterns and all four
counts equal; no tolerance. Sizes: 1 x 1 (a chain of one level: no upsample), 2 x 2 and 3 x 5 (two levels: upsample 0 only), 17 x 9 (four levels, odd
sizes, partial blocks), 64 x 48 and 128 x 256 (several 256-thread blocks, T0 larger than the frame in one axis). The restatement of a (size, matrix) pair
is computed once and shared by the tests that need it."""
import ctypes as C
import functools

import numpy as np
import pytest

from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import reproject_ref as ref
from tests import scenes

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (64, 48), (128, 256)]
MATRICES = ["identity", "yaw", "forward", "backward", "half_turn", "w_zero"]
SENTINEL = 0xA5
GUARD = 256
AIC_ERR_INVALID = 1
NEAR, FAR = 1.0, 10.0  # the synthetic frames' projection: depth d is the distance FAR NEAR / (FAR - d (FAR - NEAR)), 1 .. 10


def synthetic_frame(w, h):
    """(colour [h, w, 4] u16, depth [h, w] f32): random finite f16 colour with alpha in [0, 1]; depth uniform in [0, 1); blocks of exactly equal depth
    with a NaN (dropped) pixel inside, so that its neighbours' sprites tie there; some pixels exactly 1.0 and 0.0; a tenth of the pixels UI, -0.0 among
    them."""
    rng = np.random.default_rng(1000 * w + h)
    color = rng.integers(0, 0x7C00, (h, w, 4)).astype(np.uint16) | (rng.integers(0, 2, (h, w, 4)).astype(np.uint16) << 15)
    color[..., 3] = rng.random((h, w)).astype(np.float16).view(np.uint16)
    depth = rng.random((h, w)).astype(np.float32)
    for _ in range(max(1, w * h // 400)):
        bw, bh = min(w, 5), min(h, 4)
        x0, y0 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        depth[y0:y0 + bh, x0:x0 + bw] = np.float32(rng.random())
        if bw >= 3 and bh >= 3:
            depth[y0 + 1, x0 + 2] = np.nan
    flat = depth.reshape(-1)
    n = w * h
    flat[rng.integers(0, n, max(1, n // 50))] = 1.0
    flat[rng.integers(0, n, max(1, n // 100))] = 0.0
    ui = rng.random(n) < 0.1
    if n >= 4:
        ui[rng.integers(0, n, 2)] = True
    flat[ui] = -np.abs(flat[ui])
    zero_ui = np.flatnonzero(ui)[::5]
    flat[zero_ui] = -0.0
    return color, depth


def matrix(name, w, h):
    """(reprojection [16] f32 column-major, inverse_projection_zw [4] f32) from a perspective projection of the frame's aspect"""
    proj = ref.perspective(90.0, w / h, NEAR, FAR)
    old = ref.view()
    if name == "identity":
        _, zw = ref.reprojection(proj, old, old)
        return np.eye(4, dtype=np.float32).reshape(16), zw
    if name == "yaw":
        return ref.reprojection(proj, old, ref.view(yaw=0.02))
    if name == "forward":  # surfaces nearer than 1.2 end behind the camera, those up to 1.37 reach the ratio cap
        return ref.reprojection(proj, old, ref.view(position=(0.0, 0.0, -1.2)))
    if name == "backward":  # the old image shrinks towards the centre: gaps all round
        return ref.reprojection(proj, old, ref.view(position=(0.0, 0.0, 2.0)))
    if name == "half_turn":  # every world pixel is behind the new camera: only UI sprites are drawn
        return ref.reprojection(proj, old, ref.view(yaw=np.pi))
    assert name == "w_zero"
    # h_w = nx - nx_k: exactly 0 in column k, negative to its left
    _, zw = ref.reprojection(proj, old, old)
    k = w // 3
    nx_k = (np.float32(k) + np.float32(0.5)) * (np.float32(1) / np.float32(w)) * np.float32(2) - np.float32(1)
    m = np.eye(4, dtype=np.float32)
    m[3] = (1.0, 0.0, 0.0, -nx_k)
    return m.T.reshape(16).copy(), zw


@functools.lru_cache(maxsize=None)
def restated(w, h, name):
    """The restatement of one synthetic case: the splat stage, the chain (shared by both flag values) and both final stores."""
    color, depth = synthetic_frame(w, h)
    m, zw = matrix(name, w, h)
    out = ref.splat(color, depth, m, zw)
    chain = ref.gap_fill(out["R"])
    out["final"] = {flags: ref.finish(out["R"], flags, filled=chain) for flags in (0, 1)}
    for a in (out["R"], out["D"]):
        a.setflags(write=False)
    return out


def frame_bytes(color, depth):
    return np.concatenate([np.ascontiguousarray(color).view(np.uint8).reshape(-1), np.ascontiguousarray(depth).view(np.uint8).reshape(-1)])


def to_device(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def device_bytes(n_bytes, fill=SENTINEL):
    import torch

    t = torch.full((int(n_bytes),), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def planes_of(raw, w, h):
    n = w * h
    return raw[:n * 8].view(np.uint16).reshape(h, w, 4), raw[n * 8:n * 12].view(np.uint32).reshape(h, w)


def counts(info):
    return (info.n_splats, info.n_dropped, info.n_gaps, info.n_unfilled)


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def run(ctx, w, h, m, zw, src_bytes, flags):
    """One call on fresh buffers: (dst colour u16, dst depth u32, info); src and the guard bytes behind dst are checked here."""
    n = w * h
    src = to_device(src_bytes)
    dst = device_bytes(n * 12 + GUARD)
    info = ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr(), flags)
    raw = dst.cpu().numpy()
    assert (raw[n * 12:] == SENTINEL).all(), "guard bytes behind dst"
    assert (src.cpu().numpy() == src_bytes).all(), "src changed"
    color, depth = planes_of(raw, w, h)
    return color, depth, info


@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_frames_equal_the_restatement(ctx, w, h, name):
    color, depth = synthetic_frame(w, h)
    m, zw = matrix(name, w, h)
    want = restated(w, h, name)
    src_bytes = frame_bytes(color, depth)
    for flags in (0, abi.REPROJECT_KEEP_SPLATS):
        fin = want["final"][flags]
        got_color, got_depth, info = run(ctx, w, h, m, zw, src_bytes, flags)
        print(f"{w}x{h} {name} flags {flags}: splats {info.n_splats} dropped {info.n_dropped} gaps {info.n_gaps} unfilled {info.n_unfilled}; "
              f"colour texels differing {int((got_color != fin['color']).any(-1).sum())}, depths differing {int((got_depth != want['D'].view(np.uint32)).sum())}")
        assert (got_depth == want["D"].view(np.uint32)).all()
        assert (got_color == fin["color"]).all()
        assert counts(info) == (want["n_splats"], want["n_dropped"], want["n_gaps"], fin["n_unfilled"])
        assert (info.levels, tuple(info.t0)) == (fin["levels"], fin["t0"])
        if flags:  # dst equals R wherever R is valid
            keep = ref.valid(want["R"])
            assert (got_color[keep] == want["R"][keep]).all()
        again_color, again_depth, again = run(ctx, w, h, m, zw, src_bytes, flags)
        assert (again_color == got_color).all() and (again_depth == got_depth).all() and counts(again) == counts(info), "the same call twice"
    # what the cases are there for
    if name == "identity":
        assert want["n_gaps"] < w * h
    if name == "half_turn":
        ui = (depth.view(np.uint32) >> 31 != 0) & ~np.isnan(depth)
        assert want["n_splats"] == int(ui.sum())
    if name == "backward" and w * h >= 64 * 48:
        assert want["n_gaps"] > 0
    if name == "w_zero" and w >= 3:
        assert want["n_dropped"] >= h  # column k and everything to its left


def test_nothing_drawn_leaves_the_marker_everywhere(ctx):
    """Every depth NaN: no sprite, every pixel a gap, nothing to fill from -- the marker, depth 1.0, n_unfilled = W * H."""
    w, h = 17, 9
    color, _ = synthetic_frame(w, h)
    depth = np.full((h, w), np.nan, np.float32)
    m, zw = matrix("yaw", w, h)
    want = ref.reproject(color, depth, m, zw)
    assert want["n_unfilled"] == w * h and (want["color"] == ref.MARKER).all()
    for flags in (0, abi.REPROJECT_KEEP_SPLATS):
        got_color, got_depth, info = run(ctx, w, h, m, zw, frame_bytes(color, depth), flags)
        assert (got_color == ref.MARKER).all() and (got_depth == np.float32(1.0).view(np.uint32)).all()
        assert counts(info) == (0, w * h, w * h, w * h)


def test_the_cases_reach_the_cap_the_ties_and_the_drops():
    """(no device needed) The synthetic cases do exercise what they were built for, by the restatement's own arithmetic."""
    w, h = 64, 48
    color, depth = synthetic_frame(w, h)
    assert np.isnan(depth).any() and (depth == 1.0).any() and (depth.view(np.uint32) == 0x80000000).any()
    m, zw = matrix("forward", w, h)
    mm = m.reshape(4, 4).T
    d = np.abs(depth)
    sy, sx = np.mgrid[0:h, 0:w]
    nx = ((sx + 0.5) / w * 2 - 1).astype(np.float32)
    hw = mm[3, 0] * nx + mm[3, 2] * d + mm[3, 3]
    hz = mm[2, 2] * d + mm[2, 3]
    with np.errstate(all="ignore"):
        ratio = ref._lin(d, zw) / ref._lin(hz / hw, zw)
    world = (depth.view(np.uint32) >> 31 == 0) & ~np.isnan(depth)
    assert (world & (hw > 0) & (ratio > 8.0)).any() and (world & (hw < 0)).any()


def host_renderer(w, h, eye, target):
    import all_is_cubes_amd as A

    cams = H.StandardCameras()
    cams.graphics_options = H.GraphicsOptions()
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(scenes.one_cube_space())
    cams.world_view_transform = H.look_at_y_up(eye, target)
    r = H.HipRtRenderer(cams)
    r.update()
    return cams, r


def split_bytes(rendering):
    return frame_bytes(rendering.color_f16_bits, rendering.depth)


@pytest.mark.parametrize("flags", [0, abi.REPROJECT_KEEP_SPLATS])
def test_scene_through_the_host_mirror(flags):
    """A real Split frame of the test scene, reprojected to a nearby camera by HipRtRenderer::reproject_split."""
    w, h = 128, 96
    n = w * h
    cams, r = host_renderer(w, h, (0.7, 0.9, 2.5), (0.5, 0.5, 0.5))
    first = r.draw_split()
    traced_with = r.world_camera()
    src_bytes = split_bytes(first)
    src = to_device(src_bytes)
    cams.world_view_transform = H.look_at_y_up((0.85, 0.95, 2.4), (0.5, 0.5, 0.5))
    r.update()
    dst = device_bytes(n * 12 + GUARD)
    info = r.reproject_split(src.data_ptr(), dst.data_ptr(), traced_with, flags)
    raw = dst.cpu().numpy()
    assert (raw[n * 12:] == SENTINEL).all() and (src.cpu().numpy() == src_bytes).all()
    got_color, got_depth = planes_of(raw, w, h)
    now = r.world_camera()
    m = np.array(H.Camera.reprojection_matrix(traced_with, now), np.float32)
    zw = np.array(now.inverse_projection_zw(), np.float32)
    want = ref.reproject(first.color_f16_bits.reshape(h, w, 4), first.depth.reshape(h, w), m, zw, flags)
    retraced = r.draw_split()
    same = (got_color == retraced.color_f16_bits.reshape(h, w, 4)).all(-1).mean()
    print(f"scene {w}x{h} flags {flags}: splats {info['n_splats']} dropped {info['n_dropped']} gaps {info['n_gaps']} unfilled {info['n_unfilled']}; "
          f"{100 * same:.1f} % of the pixels have the re-traced frame's colour")
    assert (got_depth == want["D"].view(np.uint32)).all()
    assert (got_color == want["color"]).all()
    assert (info["n_splats"], info["n_dropped"], info["n_gaps"], info["n_unfilled"]) == (want["n_splats"], want["n_dropped"], want["n_gaps"], want["n_unfilled"])
    assert info["n_splats"] + info["n_dropped"] == n


def test_pipeline_reprojected_frame_is_a_resident_frame():
    """draw_split -> reproject_split -> trace_pixels_into the result for every pixel at the new camera: the aic_render Split frame of the new camera."""
    w, h = 40, 24
    n = w * h
    cams, r = host_renderer(w, h, (0.7, 0.9, 2.5), (0.5, 0.5, 0.5))
    first = r.draw_split()
    traced_with = r.world_camera()
    src = to_device(split_bytes(first))
    cams.world_view_transform = H.look_at_y_up((0.9, 1.0, 2.3), (0.45, 0.5, 0.5))
    r.update()
    resident = device_bytes(n * 12)
    r.reproject_split(src.data_ptr(), resident.data_ptr(), traced_with)
    every = to_device(np.arange(n, dtype=np.uint32))
    info = r.trace_pixels_into(resident.data_ptr(), every.data_ptr(), n)
    assert info.rows_rendered == n
    want = r.draw_split()
    assert (resident.cpu().numpy() == split_bytes(want)).all()
    # and it can be reprojected again
    again = device_bytes(n * 12)
    info = r.reproject_split(resident.data_ptr(), again.data_ptr(), r.world_camera())
    assert info["n_splats"] + info["n_dropped"] == n


def test_rejections_leave_the_context_usable(ctx):
    import torch

    w, h = 17, 9
    n = w * h
    color, depth = synthetic_frame(w, h)
    m, zw = matrix("yaw", w, h)
    want = restated(w, h, "yaw")
    src_bytes = frame_bytes(color, depth)
    src = to_device(src_bytes)
    dst = device_bytes(n * 12 + GUARD)
    assert src.data_ptr() % 8 == 0 and dst.data_ptr() % 8 == 0

    def good(what):
        got_color, got_depth, info = run(ctx, w, h, m, zw, src_bytes, 0)
        assert (got_color == want["final"][0]["color"]).all() and (got_depth == want["D"].view(np.uint32)).all(), what

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert (dst.cpu().numpy() == SENTINEL).all(), what
        good(what)

    def raw_call(desc_ptr, src_ptr, dst_ptr):
        info = abi.ReprojectInfo()
        ctx._check(ctx._lib.aic_reproject_split(ctx._h, desc_ptr, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.byref(info)))

    def desc(width=w, height=h, flags=0):
        d = abi.ReprojectDesc()
        d.width, d.height, d.flags = width, height, flags
        d.reprojection[:] = [float(v) for v in m]
        d.inverse_projection_zw[:] = [float(v) for v in zw]
        return d

    good("before")
    # a frame still occupying slot 0
    world = scenes.one_cube_space()
    ctx.upload_space(abi.LAYER_WORLD, world)
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    import oracle

    eye = (0.7, 0.9, 2.5)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, 40 / 24, oracle.look_at_y_up(eye, (0.5, 0.5, 0.5)), eye)
    busy = device_bytes(40 * 24 * 4)
    ctx.render_submit(ctx.make_frame(40, 24, world_inv=inv), busy.data_ptr(), 0)
    with pytest.raises(abi.AicError) as err:
        ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr())
    assert err.value.code == AIC_ERR_INVALID, "slot 0 busy"
    ctx.render_wait(0)
    ctx.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()
    good("after slot 0 busy")
    # NULL pointers
    rejected(lambda: raw_call(None, src.data_ptr(), dst.data_ptr()), "NULL desc")
    rejected(lambda: raw_call(C.byref(desc()), None, dst.data_ptr()), "NULL src")
    rejected(lambda: raw_call(C.byref(desc()), src.data_ptr(), None), "NULL dst")
    # src or dst not at an 8-byte boundary
    wide_src = to_device(np.concatenate([src_bytes, np.zeros(16, np.uint8)]))
    rejected(lambda: ctx.reproject_split(w, h, m, zw, wide_src.data_ptr() + 4, dst.data_ptr()), "src at 4 bytes")
    rejected(lambda: ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr() + 4), "dst at 4 bytes")
    # overlapping ranges, equal pointers included
    both = device_bytes(n * 24)
    rejected(lambda: ctx.reproject_split(w, h, m, zw, both.data_ptr(), both.data_ptr()), "src == dst")
    rejected(lambda: ctx.reproject_split(w, h, m, zw, both.data_ptr(), both.data_ptr() + n * 12 // 8 * 8 - 8), "dst starts inside src")
    rejected(lambda: ctx.reproject_split(w, h, m, zw, both.data_ptr() + 8, both.data_ptr()), "src starts inside dst")
    assert (both.cpu().numpy() == SENTINEL).all()
    # width or height above 65535
    rejected(lambda: ctx.reproject_split(65536, 1, m, zw, src.data_ptr(), dst.data_ptr()), "width above 65535")
    rejected(lambda: ctx.reproject_split(1, 65536, m, zw, src.data_ptr(), dst.data_ptr()), "height above 65535")
    # a component that is not finite
    for bad in (float("nan"), float("inf"), float("-inf")):
        for i in (0, 7, 15):
            mm = m.copy()
            mm[i] = bad
            rejected(lambda: ctx.reproject_split(w, h, mm, zw, src.data_ptr(), dst.data_ptr()), f"matrix[{i}] = {bad}")
        for i in (0, 3):
            z = zw.copy()
            z[i] = bad
            rejected(lambda: ctx.reproject_split(w, h, m, z, src.data_ptr(), dst.data_ptr()), f"inverse_projection_zw[{i}] = {bad}")
    # unknown flag bits
    for flags in (2, 1 << 31, 3):
        rejected(lambda: ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr(), flags), f"flags {flags}")
    # a width or height of 0: AIC_OK, nothing written, the info zeroed
    for ww, hh in ((0, h), (w, 0), (0, 0)):
        d = desc(ww, hh)
        info = abi.ReprojectInfo()
        C.memset(C.byref(info), 0xFF, C.sizeof(info))
        ctx._check(ctx._lib.aic_reproject_split(ctx._h, C.byref(d), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.byref(info)))
        assert bytes(info) == bytes(C.sizeof(info))
        assert (dst.cpu().numpy() == SENTINEL).all() and (src.cpu().numpy() == src_bytes).all()
    good("after the empty frames")
    torch.cuda.synchronize()
