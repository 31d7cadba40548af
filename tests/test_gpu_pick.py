"""GPU tests (-m gpu) of aic_pick_pixels: the next pixels to trace written on the device -- the unknown pixels of the context's last reprojection first, in
the picker's order, then PixelPicker's sequence from a cursor.

Yardstick: tests/pick_ref.py, the restatement of DESIGN.md 4.12 in NumPy and Python integers, on the splat image of tests/reproject_ref.py. Whole uint32
lists are compared, every info field, and the guard words behind pixels_out[n); there is no tolerance anywhere. Sizes: 1 x 1 (central = 0), 3 x 5,
17 x 9 (one scan block, not full), 64 x 48 (12 scan blocks of 256 ranks) and 257 x 129 (130 scan blocks, a partial last one; a multiple of nothing). No
size here has more than 1024 scan blocks: the scan's second round, with its carry, is the code of csrc/aic_rank_list.h that all pickers share, and the
523 x 503 frames (1028 scan blocks) of tests/test_gpu_stale.py and tests/test_gpu_stale_cubes.py cover it for aic_pick_pixels too. The
restatement of a (size, matrix) pair and every picker list are computed once and shared.

The first test needs no device: it shows from the restatement alone that the cases are not vacuous."""
import ctypes as C
import functools

import numpy as np
import pytest

from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import pick_ref
from tests import reproject_ref as ref
from tests import scenes
from tests import test_gpu_reproject as rp

gpu = pytest.mark.gpu

SIZES = [(1, 1), (3, 5), (17, 9), (64, 48), (257, 129)]
MATRICES = ["identity", "yaw", "forward"]
ORDERS = ["picker", "row_major"]
GUARD_WORDS = 64
SENTINEL_WORD = 0xA5A5A5A5
AIC_ERR_INVALID = 1
MAX_PICKS = 2048 * 65535
MARKER_SEED = {(1, 1): 0, (3, 5): 2, (17, 9): 0, (64, 48): 0, (257, 129): 0}  # checked by test_the_cases_are_not_vacuous


def marked_frame(w, h):
    """(colour with markers, colour without, depth): test_gpu_reproject's synthetic frame (random f16 colour, depths in [0, 1), a tenth UI, NaN pixels)
    with the marker texel (0, 0, 0, -1) in about 5 % of the source pixels, so that some winning sprites carry it."""
    free, depth = rp.synthetic_frame(w, h)
    rng = np.random.default_rng(77 * w + h + 100003 * MARKER_SEED[(w, h)])
    color = free.copy()
    color[rng.random((h, w)) < 0.05] = ref.MARKER
    return color, free, depth


@functools.lru_cache(maxsize=None)
def restated(w, h, name):
    """One synthetic case: the splat image R of the marked frame, the gaps (the same keys: they depend on the depths alone) and n_gaps."""
    color, free, depth = marked_frame(w, h)
    m, zw = rp.matrix(name, w, h)
    out = ref.splat(color, depth, m, zw)
    gaps = ~ref.valid(ref.splat(free, depth, m, zw)["R"])  # the unmarked colours are all valid: invalid there = no sprite
    assert int(gaps.sum()) == out["n_gaps"]
    out["gaps"] = gaps
    out["R"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def picker_order(w, h):
    order, central, cycle = abi.pixel_order(w, h)
    order.setflags(write=False)
    return order, central, cycle


def order_of(w, h, kind):
    return picker_order(w, h)[0] if kind == "picker" else None


@functools.lru_cache(maxsize=None)
def picker_list(w, h, kind, n, cursor):
    got, _ = pick_ref.pick_list(w * h, order_of(w, h, kind), n, cursor=cursor)
    got.setflags(write=False)
    return got


def expected(w, h, kind, R, n, max_unknown=0, skip_unknown=0, cursor=0):
    """pick_ref.pick_list, with the picker part taken from the shared lists"""
    order = order_of(w, h, kind)
    if max_unknown == 0:
        return picker_list(w, h, kind, n, cursor), {"n_unknown": 0, "next_cursor": (cursor + n) % 2**64, "n_from_unknown": 0, "n_from_order": n}
    ranks = pick_ref.rank_list(R, order)
    g = pick_ref.taken(n, max_unknown, len(ranks), skip_unknown)
    want = np.concatenate([ranks[skip_unknown:skip_unknown + g] if g else np.zeros(0, np.uint32), picker_list(w, h, kind, n - g, cursor)]).astype(np.uint32)
    return want, {"n_unknown": len(ranks), "next_cursor": (cursor + n - g) % 2**64, "n_from_unknown": g, "n_from_order": n - g}


def test_the_cases_are_not_vacuous():
    """(no device needed) From the restatement alone: every non-identity case has 1 <= n_unknown < count, and at least one case has an unknown pixel some
    sprite did cover -- a winner that carried the marker. 1 x 1 is left out of the first: a frame of one pixel cannot have both an unknown and a known
    pixel; it is there for central = 0."""
    marker_winner = False
    for w, h in SIZES:
        for name in MATRICES:
            out = restated(w, h, name)
            unknown = pick_ref.unknown(out["R"])
            print(f"{w}x{h} {name}: n_unknown {int(unknown.sum())} of {w * h}, gaps {out['n_gaps']}, marker winners {int((unknown & ~out['gaps'].reshape(-1)).sum())}")
            assert (unknown | ~out["gaps"].reshape(-1)).all(), "a gap is unknown"
            if name != "identity" and w * h > 1:
                assert 1 <= int(unknown.sum()) < w * h
            marker_winner |= bool((unknown & ~out["gaps"].reshape(-1)).any())
    assert marker_winner
    # the shared lists are the restatement
    order = picker_order(17, 9)[0]
    R = restated(17, 9, "yaw")["R"]
    a, ia = expected(17, 9, "picker", R, 40, max_unknown=5, skip_unknown=1, cursor=3)
    b, ib = pick_ref.pick_list(17 * 9, order, 40, R=R, max_unknown=5, skip_unknown=1, cursor=3)
    assert (a == b).all() and ia == ib


def to_device_words(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return t


def out_words(n):
    import torch

    t = torch.full((int(n) + GUARD_WORDS,), SENTINEL_WORD - 2**32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def info_dict(info):
    return {"n_unknown": info.n_unknown, "next_cursor": info.next_cursor, "n_from_unknown": info.n_from_unknown, "n_from_order": info.n_from_order}


def pick(ctx, w, h, order_dev, n, **kw):
    """One call into a fresh list: (pixels_out [n] uint32, info fields); the guard words behind it are checked here."""
    out = out_words(n)
    info = ctx.pick_pixels(w, h, n, order_dev.data_ptr() if order_dev is not None else 0, out.data_ptr(), **kw)
    raw = out.cpu().numpy().view(np.uint32)
    assert (raw[n:] == SENTINEL_WORD).all(), "guard words behind pixels_out[n)"
    assert info.kernel_ms >= 0.0 and info.reserved == 0
    return raw[:n].copy(), info_dict(info)


def check(ctx, w, h, kind, order_dev, R, n, what, **kw):
    want, want_info = expected(w, h, kind, R, n, **kw)
    got, got_info = pick(ctx, w, h, order_dev, n, **kw)
    differing = int((got != want).sum())
    print(f"{w}x{h} {kind} {what}: n {n} {kw} -> {got_info}; entries differing {differing}")
    assert got_info == want_info, what
    assert differing == 0, what
    return got


def reproject(ctx, w, h, color, depth, name):
    m, zw = rp.matrix(name, w, h)
    src = rp.to_device(rp.frame_bytes(color, depth))
    dst = rp.device_bytes(w * h * 12)
    info = ctx.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr(), abi.REPROJECT_KEEP_SPLATS)
    return info, dst


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


@gpu
@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_frames_equal_the_restatement(ctx, w, h, name, kind):
    color, _, depth = marked_frame(w, h)
    R = restated(w, h, name)["R"]
    count = w * h
    _, central, cycle = picker_order(w, h)  # (they depend on the size alone: the same without an order)
    assert central == min(pick_ref.CENTRAL_MAX, count // 4) and cycle == 2 * max(central, count - central)
    reproject(ctx, w, h, color, depth, name)
    order_dev = to_device_words(picker_order(w, h)[0]) if kind == "picker" else None
    nu = int(pick_ref.unknown(R).sum())
    # all of U, then seven picks; and the same call again
    n = nu + 7
    first = check(ctx, w, h, kind, order_dev, R, n, "all of U and 7 picks", max_unknown=n)
    again = check(ctx, w, h, kind, order_dev, R, n, "the same call twice", max_unknown=n)
    assert (first == again).all()
    # the pure picker
    for n in (1, 63, 64, 65, cycle):
        check(ctx, w, h, kind, order_dev, R, n, "pure picker")
    # unknown pixels already handed out
    for skip in (1, nu - 1, nu, nu + 5):
        if skip >= 0:
            check(ctx, w, h, kind, order_dev, R, nu + 7, "skip", max_unknown=nu + 7, skip_unknown=skip)
    # max_unknown < n < n_unknown (needs three unknown pixels)
    if nu >= 3:
        check(ctx, w, h, kind, order_dev, R, nu - 1, "max_unknown < n < n_unknown", max_unknown=(nu - 1) // 2)
    # cursors: the start, the wrap of the inner cycle, the end of the whole cycle, beyond 32 bits -- behind some unknown pixels and alone
    for cursor in (0, max(2 * central - 1, 0), cycle - 1, 2**40 + 3):
        check(ctx, w, h, kind, order_dev, R, 70, "cursor", max_unknown=4, cursor=cursor)
        check(ctx, w, h, kind, order_dev, R, 70, "cursor, pure picker", cursor=cursor)


@gpu
@pytest.mark.parametrize("w,h", [(17, 9), (64, 48)])
def test_marker_free_sources_count_the_gaps(ctx, w, h):
    """Without markers in the source a pixel is unknown exactly where no sprite landed: n_unknown is aic_reproject_info.n_gaps."""
    _, free, depth = marked_frame(w, h)
    for name in MATRICES:
        rinfo, _ = reproject(ctx, w, h, free, depth, name)
        want = restated(w, h, name)
        assert rinfo.n_gaps == want["n_gaps"]
        R = np.where(want["gaps"][..., None], ref.MARKER, free).astype(np.uint16)  # (only its validity matters)
        got, info = pick(ctx, w, h, None, 5, max_unknown=5)
        assert info["n_unknown"] == rinfo.n_gaps, name
        assert (got == expected(w, h, "row_major", R, 5, max_unknown=5)[0]).all()


@gpu
def test_nothing_drawn_lists_the_order_itself(ctx):
    """Every depth NaN (test_nothing_drawn_leaves_the_marker_everywhere's frame): every pixel is unknown and the list is the order."""
    w, h = 17, 9
    count = w * h
    color, _ = rp.synthetic_frame(w, h)
    depth = np.full((h, w), np.nan, np.float32)
    rinfo, _ = reproject(ctx, w, h, color, depth, "yaw")
    assert rinfo.n_gaps == count
    order = picker_order(w, h)[0]
    got, info = pick(ctx, w, h, to_device_words(order), count, max_unknown=count)
    assert info == {"n_unknown": count, "next_cursor": 0, "n_from_unknown": count, "n_from_order": 0}
    assert (got == order).all()
    got, info = pick(ctx, w, h, None, count, max_unknown=count)
    assert info["n_unknown"] == count and (got == np.arange(count)).all()


@gpu
def test_state_follows_the_last_reprojection(ctx):
    import oracle

    w, h = 64, 48
    count = w * h
    color, _, depth = marked_frame(w, h)
    order = picker_order(w, h)[0]
    order_dev = to_device_words(order)
    R_yaw, R_fwd = restated(w, h, "yaw")["R"], restated(w, h, "forward")["R"]
    nu = int(pick_ref.unknown(R_yaw).sum())
    _, dst = reproject(ctx, w, h, color, depth, "yaw")
    before = check(ctx, w, h, "picker", order_dev, R_yaw, nu + 7, "after the reprojection", max_unknown=nu + 7)
    # a presentation and a round of tracing into the reprojected frame in between: the list does not change
    ctx.present_split(dst.data_ptr(), (w, h), (w, h), 0.25, 1, 1.0)
    ctx.upload_space(abi.LAYER_WORLD, scenes.one_cube_space())
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    eye = (0.7, 0.9, 2.5)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, w / h, oracle.look_at_y_up(eye, (0.5, 0.5, 0.5)), eye)
    frame = ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_SPLIT)
    traced = to_device_words(before[:nu])
    info = ctx.trace_pixels_device(frame, nu, traced.data_ptr(), dst.data_ptr(), in_place=True)
    assert info.rows_rendered == nu
    after = check(ctx, w, h, "picker", order_dev, R_yaw, nu + 7, "after present and trace", max_unknown=nu + 7)
    assert (after == before).all()
    # a second reprojection of the same size under another matrix: the list follows the new R
    reproject(ctx, w, h, color, depth, "forward")
    nf = int(pick_ref.unknown(R_fwd).sum())
    assert not np.array_equal(pick_ref.rank_list(R_fwd, order), pick_ref.rank_list(R_yaw, order))
    check(ctx, w, h, "picker", order_dev, R_fwd, nf + 7, "after a second reprojection", max_unknown=nf + 7)
    # a reprojection of another size: the old size's unknown pixels are gone, its picker is not
    w2, h2 = 17, 9
    color2, _, depth2 = marked_frame(w2, h2)
    reproject(ctx, w2, h2, color2, depth2, "yaw")
    out = out_words(16)
    with pytest.raises(abi.AicError) as err:
        ctx.pick_pixels(w, h, 16, order_dev.data_ptr(), out.data_ptr(), max_unknown=1)
    assert err.value.code == AIC_ERR_INVALID
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all()
    check(ctx, w, h, "picker", order_dev, None, 70, "the old size, pure picker", cursor=5)
    check(ctx, w2, h2, "row_major", None, restated(w2, h2, "yaw")["R"], 30, "the new size", max_unknown=30)
    # a rejected reprojection leaves the state as it was
    m, zw = rp.matrix("yaw", w2, h2)
    with pytest.raises(abi.AicError):
        ctx.reproject_split(w, h, m, zw, dst.data_ptr(), dst.data_ptr())
    check(ctx, w2, h2, "row_major", None, restated(w2, h2, "yaw")["R"], 30, "after a rejected reprojection", max_unknown=30)


@gpu
def test_a_fresh_context_has_no_unknown_pixels():
    with abi.Context(0) as c:
        out = out_words(8)
        with pytest.raises(abi.AicError) as err:
            c.pick_pixels(17, 9, 8, 0, out.data_ptr(), max_unknown=8)
        assert err.value.code == AIC_ERR_INVALID
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all()
        got, info = pick(c, 17, 9, None, 8)
        assert (got == picker_list(17, 9, "row_major", 8, 0)).all() and info["n_from_order"] == 8


@gpu
def test_pipeline_traces_the_unknown_pixels_first():
    """draw_split at camera A, reproject_split to B keeping the splats, pick_pixels for every unknown pixel, trace_pixels_into with that device list: the
    listed pixels are the restatement's U by picker rank, each now holds aic_render's texel at B, and no other texel of the frame moved."""
    w, h = 40, 24
    n = w * h
    cams, r = rp.host_renderer(w, h, (0.7, 0.9, 2.5), (0.5, 0.5, 0.5))
    first = r.draw_split()
    traced_with = r.world_camera()
    src = rp.to_device(rp.split_bytes(first))
    cams.world_view_transform = H.look_at_y_up((0.9, 1.0, 2.3), (0.45, 0.5, 0.5))
    r.update()
    now = r.world_camera()
    m = np.array(H.Camera.reprojection_matrix(traced_with, now), np.float32)
    zw = np.array(now.inverse_projection_zw(), np.float32)
    R = ref.splat(first.color_f16_bits.reshape(h, w, 4), first.depth.reshape(h, w), m, zw)["R"]
    order = picker_order(w, h)[0]
    ranks = pick_ref.rank_list(R, order)
    nu = len(ranks)
    print(f"pipeline {w}x{h}: {nu} unknown pixels")
    assert nu >= 1
    resident = rp.device_bytes(n * 12)
    rinfo = r.reproject_split(src.data_ptr(), resident.data_ptr(), traced_with, abi.REPROJECT_KEEP_SPLATS)
    assert r.pick_skip_unknown == 0
    before = resident.cpu().numpy().copy()
    order_dev = to_device_words(order)
    picks = out_words(nu)
    info = r.pick_pixels(order_dev.data_ptr(), picks.data_ptr(), nu, nu)
    assert (info["n_unknown"], info["n_from_unknown"], info["n_from_order"], info["next_cursor"]) == (nu, nu, 0, 0)
    assert rinfo["n_gaps"] <= nu and (r.pick_cursor, r.pick_skip_unknown) == (0, nu)
    raw = picks.cpu().numpy().view(np.uint32)
    assert (raw[nu:] == SENTINEL_WORD).all()
    listed = raw[:nu]
    assert (listed == ranks).all()
    tinfo = r.trace_pixels_into(resident.data_ptr(), picks.data_ptr(), nu)
    assert tinfo.rows_rendered == nu
    after = resident.cpu().numpy()
    want = rp.split_bytes(r.draw_split())
    b_color, b_depth = before[:n * 8].view(np.uint64), before[n * 8:].view(np.uint32)
    a_color, a_depth = after[:n * 8].view(np.uint64), after[n * 8:].view(np.uint32)
    w_color, w_depth = want[:n * 8].view(np.uint64), want[n * 8:].view(np.uint32)
    assert (a_color[listed] == w_color[listed]).all() and (a_depth[listed] == w_depth[listed]).all()
    rest = np.ones(n, bool)
    rest[listed] = False
    assert (a_color[rest] == b_color[rest]).all() and (a_depth[rest] == b_depth[rest]).all()
    # the unknown pixels are handed out: the next call with max_unknown is the reference's picker from its cursor
    more = out_words(10)
    info = r.pick_pixels(order_dev.data_ptr(), more.data_ptr(), 10, 10)
    assert (info["n_unknown"], info["n_from_unknown"], info["next_cursor"]) == (nu, 0, 10)
    assert (more.cpu().numpy().view(np.uint32)[:10] == H.PixelPicker(w, h).take(10)).all()
    # a reprojection starts the unknown pixels again, the cursor stays; a new viewport size starts both
    r.reproject_split(src.data_ptr(), resident.data_ptr(), traced_with, abi.REPROJECT_KEEP_SPLATS)
    assert (r.pick_cursor, r.pick_skip_unknown) == (10, 0)
    cams.viewport = H.Viewport.with_scale(1.0, 17, 9)
    r.update()
    info = r.pick_pixels(0, more.data_ptr(), 4, 0)
    assert info["next_cursor"] == 4 and (more.cpu().numpy().view(np.uint32)[:4] == picker_list(17, 9, "row_major", 4, 0)).all()


@gpu
def test_rejections_leave_the_context_usable(ctx):
    import oracle
    import torch

    w, h = 17, 9
    color, _, depth = marked_frame(w, h)
    R = restated(w, h, "yaw")["R"]
    order_dev = to_device_words(picker_order(w, h)[0])
    reproject(ctx, w, h, color, depth, "yaw")
    n = 40
    out = out_words(n + 4)
    assert out.data_ptr() % 4 == 0 and order_dev.data_ptr() % 4 == 0

    def good(what):
        check(ctx, w, h, "picker", order_dev, R, n, what, max_unknown=n, skip_unknown=1, cursor=9)

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all(), what
        good(what)

    def desc(width=w, height=h, n=n, max_unknown=n, flags=0):
        d = abi.PickDesc()
        d.width, d.height, d.n, d.max_unknown, d.flags = width, height, n, max_unknown, flags
        return d

    def raw_call(desc_ptr, order_ptr, out_ptr, info_ptr):
        ctx._check(ctx._lib.aic_pick_pixels(ctx._h, desc_ptr, C.c_void_p(order_ptr), C.c_void_p(out_ptr), info_ptr))

    good("before")
    info = abi.PickInfo()
    rejected(lambda: raw_call(None, order_dev.data_ptr(), out.data_ptr(), C.byref(info)), "NULL desc")
    rejected(lambda: raw_call(C.byref(desc()), order_dev.data_ptr(), out.data_ptr(), None), "NULL info")
    rejected(lambda: raw_call(C.byref(desc()), order_dev.data_ptr(), None, C.byref(info)), "NULL pixels_out with n > 0")
    for off in (1, 2, 3):
        rejected(lambda: ctx.pick_pixels(w, h, n, order_dev.data_ptr(), out.data_ptr() + off, max_unknown=n), f"pixels_out at {off} bytes")
        rejected(lambda: ctx.pick_pixels(w, h, n, order_dev.data_ptr() + off, out.data_ptr(), max_unknown=n), f"order at {off} bytes")
    for ww, hh in ((0, h), (w, 0), (0, 0)):
        rejected(lambda: ctx.pick_pixels(ww, hh, n, 0, out.data_ptr()), f"n > 0 in an empty frame {ww}x{hh}")
    rejected(lambda: ctx.pick_pixels(65536, 1, n, 0, out.data_ptr()), "width above 65535")
    rejected(lambda: ctx.pick_pixels(1, 65536, n, 0, out.data_ptr()), "height above 65535")
    rejected(lambda: ctx.pick_pixels(w, h, MAX_PICKS + 1, 0, out.data_ptr()), "n above 2048 x 65535")
    for flags in (1, 2, 1 << 31):
        rejected(lambda: ctx.pick_pixels(w, h, n, 0, out.data_ptr(), flags=flags), f"flags {flags}")
    rejected(lambda: ctx.pick_pixels(w + 1, h, n, 0, out.data_ptr(), max_unknown=1), "max_unknown without a reprojection of this size")
    rejected(lambda: ctx.pick_pixels(h, w, n, 0, out.data_ptr(), max_unknown=1), "max_unknown with the reprojection's size transposed")
    # a frame still occupying slot 0
    ctx.upload_space(abi.LAYER_WORLD, scenes.one_cube_space())
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    eye = (0.7, 0.9, 2.5)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, 40 / 24, oracle.look_at_y_up(eye, (0.5, 0.5, 0.5)), eye)
    busy = rp.device_bytes(40 * 24 * 4)
    ctx.render_submit(ctx.make_frame(40, 24, world_inv=inv), busy.data_ptr(), 0)
    with pytest.raises(abi.AicError) as err:
        ctx.pick_pixels(w, h, n, order_dev.data_ptr(), out.data_ptr(), max_unknown=n)
    assert err.value.code == AIC_ERR_INVALID, "slot 0 busy"
    ctx.render_wait(0)
    ctx.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all()
    good("after slot 0 busy")
    # n = 0 and an empty frame: AIC_OK, nothing written, the info zeroed -- a NULL list is then fine
    for ww, hh, out_ptr in ((w, h, out.data_ptr()), (w, h, None), (0, h, out.data_ptr()), (0, 0, None)):
        d = desc(ww, hh, n=0, max_unknown=3 if ww else 0)
        C.memset(C.byref(info), 0xFF, C.sizeof(info))
        raw_call(C.byref(d), order_dev.data_ptr(), out_ptr, C.byref(info))
        assert bytes(info) == bytes(C.sizeof(info))
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all()
    good("after the empty calls")
    torch.cuda.synchronize()
