"""GPU tests (-m gpu) of aic_pick_stale: the next pixels to trace written on the device -- the pixels a scene change made stale first, in the picker's
order, then PixelPicker's sequence from a cursor.

Yardstick: tests/stale_ref.py, the restatement of DESIGN.md 4.17 in NumPy and Python integers. Whole uint32 lists are compared, every info field, and the
guard words behind pixels_out[n); there is no tolerance anywhere. Sizes: 61 x 37 (2257 ranks: a partial wave, a partial scan block, 9 blocks),
300 x 220 (66 000 ranks: more than 65 536, 258 scan blocks) and 523 x 503 (263 069 ranks, 1028 scan blocks: the scan's second round of 1024). Frames,
orders and rectangle sets are made once and shared.

The end-to-end tests take tests/stale_scenes.py's edits, whose stale sets tests/test_stale_cpu.py checks against the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from all_is_cubes_amd import abi
from tests import pick_ref, scenes, stale_ref
from tests import stale_scenes as S
from tests import test_gpu_pick as pk
from tests import test_gpu_reproject as rp
from tests.test_gpu_parity import to_abi_options

gpu = pytest.mark.gpu

SIZES = [(61, 37), (300, 220), (523, 503)]
ORDERS = ["picker", "row_major"]
SENTINEL_WORD = pk.SENTINEL_WORD
AIC_ERR_INVALID = 1
MAX_PICKS = 2048 * 65535
CHUNK = 256  # rectangles the count phase stages through LDS at a time (aic_stale.h)
DMIN = np.float32(0.5)
ALPHA_BELOW_ONE = 0x3BFF  # the f16 just below 1.0


@functools.lru_cache(maxsize=None)
def frame(w, h):
    """(colour [h, w, 4] u16, depth [h, w] f32): test_gpu_reproject's synthetic frame (a tenth UI depths with the sign bit, -0.0 among them, NaN depths,
    alpha anywhere in [0, 1]) with, over it, alpha exactly 1 in half the pixels and just below 1 in a tenth, marker texels, NaN alphas, and depths exactly
    DMIN, one step below it and one above."""
    color, depth = rp.synthetic_frame(w, h)
    color, depth = color.copy(), depth.copy()
    rng = np.random.default_rng(31 * w + h)
    u = rng.random((h, w))
    color[..., 3][u < 0.5] = np.float16(1.0).view(np.uint16)
    color[..., 3][(u >= 0.5) & (u < 0.6)] = ALPHA_BELOW_ONE
    color[..., 3][(u >= 0.6) & (u < 0.63)] = 0x7E00  # NaN
    color[(u >= 0.63) & (u < 0.68)] = rp.ref.MARKER
    v = rng.random((h, w))
    depth[v < 0.1] = DMIN
    depth[(v >= 0.1) & (v < 0.2)] = np.nextafter(DMIN, np.float32(0.0))
    depth[(v >= 0.2) & (v < 0.3)] = np.nextafter(DMIN, np.float32(1.0))
    color.setflags(write=False)
    depth.setflags(write=False)
    return color, depth


def recs(items):
    out = np.zeros(len(items), stale_ref.RECT_DTYPE)
    for i, (x0, y0, x1, y1, dmin) in enumerate(items):
        out[i] = (x0, y0, x1, y1, dmin, 0)
    return out


@functools.lru_cache(maxsize=None)
def rect_sets(w, h):
    rng = np.random.default_rng(w * 7 + h)
    inf = np.float32(np.inf)
    many = []
    for _ in range(CHUNK + 1):  # one more than an LDS chunk holds; the last one alone reaches the frame's last pixel
        x0, y0 = int(rng.integers(0, w - 3)), int(rng.integers(0, h // 2))
        many.append((x0, y0, x0 + int(rng.integers(1, 4)), y0 + int(rng.integers(1, 3)), float(rng.choice([0.25, 0.5, 0.75]))))
    many[-1] = (w - 2, h - 1, w, h, 0.5)
    sets = {
        "none": recs([]),
        "single_pixel": recs([(w // 2, h // 3, w // 2 + 1, h // 3 + 1, 0.5)]),
        "whole_frame": recs([(0, 0, w, h, 0.5)]),
        "whole_frame_unknown_depth": recs([(0, 0, w, h, -inf)]),
        "overlapping": recs([(2, 2, w // 2, h // 2, 0.9), (w // 4, h // 4, w - 3, h - 2, 0.5), (w // 3, 1, w // 3 + 9, h - 1, 0.1), (5, 5, 20, 20, inf)]),
        "empty_ones": recs([(0, 0, 0, 0, 0.0), (7, 3, 7, 30, 0.5), (4, h, w, h, 0.5), (w - 9, 6, w - 2, 21, 0.5), (3, 3, 3, 3, 0.5)]),
        "only_empty": recs([(0, 0, 0, 0, 0.0), (w, 0, w, h, 0.5)]),
        "frame_edges": recs([(0, 0, w, 1, 0.5), (0, h - 1, w, h, 0.5), (0, 0, 1, h, 0.5), (w - 1, 0, w, h, 0.5)]),
        "chunk_plus_one": recs(many),
    }
    for s in sets.values():
        s.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def picker_order(w, h):
    order = abi.pixel_order(w, h)[0]
    order.setflags(write=False)
    return order


def order_of(w, h, kind):
    return picker_order(w, h) if kind == "picker" else None


@functools.lru_cache(maxsize=None)
def picker_list(w, h, kind, n, cursor):
    order = order_of(w, h, kind)
    got = np.array([pick_ref.pick(cursor + j, w * h, order) for j in range(n)], np.uint32)
    got.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def ranks_of(w, h, kind, set_name, flags):
    color, depth = frame(w, h)
    r = stale_ref.rank_list(stale_ref.stale_mask(w, h, rect_sets(w, h)[set_name], color, depth, flags), order_of(w, h, kind))
    r.setflags(write=False)
    return r


def expected(w, h, kind, set_name, flags, n, max_stale=0, skip_stale=0, cursor=0):
    """stale_ref.pick_list, with the rank list and the picker part taken from the shared copies"""
    look = max_stale > 0 and len(rect_sets(w, h)[set_name]) > 0
    ranks = ranks_of(w, h, kind, set_name, flags) if look else np.zeros(0, np.uint32)
    g = pick_ref.taken(n, max_stale, len(ranks), skip_stale)
    want = np.concatenate([ranks[skip_stale:skip_stale + g], picker_list(w, h, kind, n - g, cursor)]).astype(np.uint32)
    return want, {"n_stale": len(ranks), "next_cursor": (cursor + n - g) % 2**64, "n_from_stale": g, "n_from_order": n - g}


def info_dict(info):
    return {"n_stale": info.n_stale, "next_cursor": info.next_cursor, "n_from_stale": info.n_from_stale, "n_from_order": info.n_from_order}


def pick(ctx, w, h, rects, src, order_dev, n, **kw):
    """One call into a fresh list: (pixels_out [n] uint32, info fields); the guard words behind it are checked here."""
    out = pk.out_words(n)
    info = ctx.pick_stale(w, h, n, rects, src.data_ptr() if src is not None else 0, order_dev.data_ptr() if order_dev is not None else 0, out.data_ptr(), **kw)
    raw = out.cpu().numpy().view(np.uint32)
    assert (raw[n:] == SENTINEL_WORD).all(), "guard words behind pixels_out[n)"
    assert info.kernel_ms >= 0.0 and info.reserved == 0
    return raw[:n].copy(), info_dict(info)


def check(ctx, w, h, kind, set_name, flags, src, order_dev, n, what, **kw):
    want, want_info = expected(w, h, kind, set_name, flags, n, **kw)
    got, got_info = pick(ctx, w, h, rect_sets(w, h)[set_name], src, order_dev, n, flags=flags, **kw)
    differing = int((got != want).sum())
    print(f"{w}x{h} {kind} {set_name} flags {flags} {what}: n {n} {kw} -> {got_info}; entries differing {differing}")
    assert got_info == want_info, what
    assert differing == 0, what
    return got


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def test_the_cases_are_not_vacuous():
    """(no device needed) From the restatement alone: the depth test keeps pixels out and leaves pixels in, for every reason the rule names; the shared
    lists are the restatement's."""
    w, h = 61, 37
    color, depth = frame(w, h)
    whole = rect_sets(w, h)["whole_frame"]
    plain = stale_ref.stale_mask(w, h, whole)
    deep = stale_ref.stale_mask(w, h, whole, color, depth, stale_ref.DEPTH_TEST).reshape(h, w)
    assert plain.all() and 0 < deep.sum() < w * h
    alpha = color[..., 3].view(np.float16).astype(np.float32)
    bits = depth.view(np.uint32)
    one = alpha == 1.0
    for what, where in [("UI depth", (bits >> 31 == 1) & (np.abs(depth) > 0)), ("-0.0", bits == 0x80000000), ("NaN depth", np.isnan(depth)),
                        ("marker", (color == rp.ref.MARKER).all(-1)), ("NaN alpha", np.isnan(alpha)), ("alpha just below 1", color[..., 3] == ALPHA_BELOW_ONE),
                        ("depth equal to dmin", one & (depth == DMIN))]:
        assert where.sum() >= 3, what
        assert deep[where].all(), what
    kept_out = one & (depth == np.nextafter(DMIN, np.float32(0.0)))
    assert kept_out.sum() >= 3 and not deep[kept_out].any()
    assert not rect_sets(w, h)["whole_frame_unknown_depth"]["dmin"][0] > -np.inf
    assert stale_ref.stale_mask(w, h, rect_sets(w, h)["whole_frame_unknown_depth"], color, depth, stale_ref.DEPTH_TEST).all()
    for size in SIZES:
        assert len(rect_sets(*size)["chunk_plus_one"]) == CHUNK + 1
        for name, rects in rect_sets(*size).items():
            assert ((rects["x0"] <= rects["x1"]) & (rects["x1"] <= size[0]) & (rects["y0"] <= rects["y1"]) & (rects["y1"] <= size[1])).all(), name
    a, ia = expected(w, h, "picker", "overlapping", 1, 300, max_stale=200, skip_stale=3, cursor=5)
    b, ib = stale_ref.pick_list(w, h, picker_order(w, h), 300, rect_sets(w, h)["overlapping"], color, depth, 1, max_stale=200, skip_stale=3, cursor=5)
    assert (a == b).all() and ia == ib


@gpu
@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_frames_equal_the_restatement(ctx, w, h, kind):
    color, depth = frame(w, h)
    src_bytes = rp.frame_bytes(color, depth)
    src = rp.to_device(src_bytes)
    order_dev = pk.to_device_words(picker_order(w, h)) if kind == "picker" else None
    large = w * h > 100000
    names = ["whole_frame", "overlapping", "chunk_plus_one"] if large else list(rect_sets(w, h))
    for set_name in names:
        for flags in (0, stale_ref.DEPTH_TEST):
            ns = len(ranks_of(w, h, kind, set_name, flags))
            # all of S, then seven picks; and the same call again
            n = ns + 7
            first = check(ctx, w, h, kind, set_name, flags, src, order_dev, n, "all of S and 7 picks", max_stale=n)
            again = check(ctx, w, h, kind, set_name, flags, src, order_dev, n, "the same call twice", max_stale=n)
            assert (first == again).all()
            if large and flags == 0:
                continue
            # n below n_stale; max_stale below n
            if ns >= 3:
                check(ctx, w, h, kind, set_name, flags, src, order_dev, ns - 1, "n < n_stale", max_stale=ns - 1)
                check(ctx, w, h, kind, set_name, flags, src, order_dev, ns - 1, "max_stale < n < n_stale", max_stale=(ns - 1) // 2, cursor=2**40 + 3)
            # stale pixels already handed out: inside the set and past it
            for skip in (1, ns - 1, ns, ns + 5):
                if skip >= 0:
                    check(ctx, w, h, kind, set_name, flags, src, order_dev, 70, "skip", max_stale=70, skip_stale=skip, cursor=9)
            # max_stale = 0: the picker alone
            check(ctx, w, h, kind, set_name, flags, src, order_dev, 70, "max_stale = 0", cursor=w * h // 2 - 1)
    # without the depth test the frame is not read: no frame will do
    check(ctx, w, h, kind, "overlapping", 0, None, order_dev, 50, "NULL src without the depth test", max_stale=50)
    assert (src.cpu().numpy() == src_bytes).all(), "src is only read"


@gpu
def test_an_order_entry_that_is_no_pixel_is_never_stale(ctx):
    w, h = 61, 37
    count = w * h
    color, depth = frame(w, h)
    src = rp.to_device(rp.frame_bytes(color, depth))
    order = picker_order(w, h).copy()
    order[[0, 5, 300, count - 1]] = [count, 0xFFFFFFFF, count + 7, 2**31]
    whole = rect_sets(w, h)["whole_frame"]
    for flags in (0, stale_ref.DEPTH_TEST):
        want, want_info = stale_ref.pick_list(w, h, order, count, whole, color, depth, flags, max_stale=count)
        got, info = pick(ctx, w, h, whole, src, pk.to_device_words(order), count, flags=flags, max_stale=count)
        assert info == want_info and (got == want).all()
        assert info["n_stale"] <= count - 4 and (flags or info["n_stale"] == count - 4)


def load_case(ctx, name, antialiasing):
    """Uploads space A of the case; returns (the Split frame's description, view_projection)."""
    sp, _, _, _ = S.case(name)
    inv, vp, zw = S.camera(name)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(S.options(antialiasing)))
    ctx.clear_space(abi.LAYER_UI)
    ctx.set_depth_transform(zw)
    return ctx.make_frame(S.W, S.HT, world_inv=inv, flags=abi.FRAME_OUT_SPLIT), vp


@gpu
@pytest.mark.parametrize("antialiasing", S.ANTIALIASING)
@pytest.mark.parametrize("name,flags", [("plaza", 0), ("terrace", 0), ("behind_wall", 0), ("behind_wall", stale_ref.DEPTH_TEST)])
def test_an_edit_is_complete_after_tracing_the_stale_pixels(ctx, name, flags, antialiasing):
    """A resident Split frame of A; aic_update_cubes to B; rectangles with expand = 1; every stale pixel picked and traced in place: the resident frame
    is a fresh Split render of B byte for byte, and n_stale is the value tests/test_stale_cpu.py checks against the oracle."""
    w, h = S.W, S.HT
    count = w * h
    try:
        f, vp = load_case(ctx, name, antialiasing)
        resident = rp.device_bytes(count * 12)
        ctx.render_submit(f, resident.data_ptr(), 0)
        ctx.render_wait(0)
        ctx.synchronize()
        before = resident.cpu().numpy().copy()
        _, edits, _, _ = S.case(name)
        ctx.update_cubes(abi.LAYER_WORLD, [cube for cube, _ in edits], [index for _, index in edits])
        rects = abi.stale_rects(vp, w, h, S.boxes(name), 1)
        s, want_rects = S.stale_set(name, antialiasing, flags)
        assert rects.tobytes() == want_rects.tobytes()
        order = picker_order(w, h)
        picks = pk.out_words(count)
        info = ctx.pick_stale(w, h, count, rects, resident.data_ptr(), pk.to_device_words(order).data_ptr(), picks.data_ptr(), max_stale=count, flags=flags)
        n_stale = int(s.sum())
        print(f"{name} aa {antialiasing} flags {flags}: n_stale {info.n_stale} (restated {n_stale}), {info.kernel_ms:.3f} ms")
        assert (info.n_stale, info.n_from_stale, info.n_from_order) == (n_stale, n_stale, count - n_stale)
        listed = picks.cpu().numpy().view(np.uint32)[:n_stale]
        assert (listed == stale_ref.rank_list(s, order)).all()
        tinfo = ctx.trace_pixels_device(f, n_stale, picks.data_ptr(), resident.data_ptr(), in_place=True)
        assert tinfo.rows_rendered == n_stale
        after = resident.cpu().numpy()
        fresh = ctx.render(f)
        want = rp.frame_bytes(fresh["color_f16"].view(np.uint16), fresh["depth"])
        changed = (before[:count * 8].view(np.uint64) != want[:count * 8].view(np.uint64)) | (before[count * 8:].view(np.uint32) != want[count * 8:].view(np.uint32))
        assert changed.sum() >= 20 and not (changed & ~s).any(), "the edit shows, and only inside S"
        assert (after == want).all()
    finally:
        ctx.set_depth_transform((1.0, 0.0, 0.0, 1.0))


@gpu
def test_host_mirror_refreshes_an_edit_from_its_own_dirty_set():
    """HipRtRenderer: draw_split of plaza's A, the edits through Space.set, update(), changed_boxes(), stale_rects(), pick_stale() frame by frame until no
    stale pixel is left, trace_pixels_into each list: the resident frame is draw_split of B byte for byte, every texel outside the lists is untouched,
    and at most half the frame was listed."""
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H

    w, h = 40, 24
    n = w * h
    sp, edits, eye, target = S.case("plaza")
    cams = H.StandardCameras()
    cams.graphics_options = H.GraphicsOptions()
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    space = A.space_from_flat(sp)
    cams.world_space = space
    cams.world_view_transform = H.look_at_y_up(eye, target)
    r = H.HipRtRenderer(cams)
    r.update()
    assert [list(b) for b in r.changed_boxes()] == [[*sp.lo, *sp.hi]], "a space uploaded whole"
    resident = rp.to_device(rp.split_bytes(r.draw_split()))
    before = resident.cpu().numpy().copy()
    r.update()
    assert r.changed_boxes() == []
    for cube, index in edits:
        space.set(*cube, index)
    r.update()
    boxes = r.changed_boxes()
    assert sorted(list(b) for b in boxes) == sorted([*cube, *(c + 1 for c in cube)] for cube, _ in edits)
    rects = r.stale_rects(boxes)
    assert len(rects) == len(edits) and r.pick_skip_stale == 0
    want_s = stale_ref.stale_mask(w, h, np.array(rects, stale_ref.RECT_DTYPE))
    assert 0 < want_s.sum() <= n // 2
    order = abi.pixel_order(w, h)[0]
    order_dev = pk.to_device_words(order)
    per_frame = 100
    listed = []
    for _ in range(n // per_frame + 2):
        picks = pk.out_words(per_frame)
        info = r.pick_stale(rects, resident.data_ptr(), order_dev.data_ptr(), picks.data_ptr(), per_frame, per_frame)
        if info["n_from_stale"] == 0:
            break
        listed.append(picks.cpu().numpy().view(np.uint32)[:info["n_from_stale"]].copy())
        r.trace_pixels_into(resident.data_ptr(), picks.data_ptr(), info["n_from_stale"])  # (the picker's picks behind them wait for their own frame)
    listed = np.concatenate(listed)
    assert (listed == stale_ref.rank_list(want_s, order)).all() and r.pick_skip_stale == len(listed) == info["n_stale"]
    after = resident.cpu().numpy()
    want = rp.split_bytes(r.draw_split())
    assert (after == want).all()
    rest = np.ones(n, bool)
    rest[listed] = False
    assert (after[:n * 8].view(np.uint64)[rest] == before[:n * 8].view(np.uint64)[rest]).all()
    assert (after[n * 8:].view(np.uint32)[rest] == before[n * 8:].view(np.uint32)[rest]).all()
    assert (before != want).any(), "the edit shows"
    # new rectangles start the count again; so does a reprojection
    r.restart_stale()
    assert r.pick_skip_stale == 0


@gpu
def test_rejections_leave_the_context_usable(ctx):
    import oracle
    import torch

    w, h = 61, 37
    color, depth = frame(w, h)
    src_bytes = rp.frame_bytes(color, depth)
    src = rp.to_device(src_bytes)
    order_dev = pk.to_device_words(picker_order(w, h))
    rects = rect_sets(w, h)["overlapping"]
    n = 40
    out = pk.out_words(n + 4)
    assert out.data_ptr() % 4 == 0 and order_dev.data_ptr() % 4 == 0 and src.data_ptr() % 8 == 0

    def good(what):
        check(ctx, w, h, "picker", "overlapping", 1, src, order_dev, n, what, max_stale=n, skip_stale=1, cursor=9)

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all(), what
        assert (src.cpu().numpy() == src_bytes).all(), what
        good(what)

    def call(width=w, height=h, n=n, r=rects, src_ptr=None, order_ptr=None, out_ptr=None, **kw):
        kw.setdefault("max_stale", n)
        kw.setdefault("flags", 1)
        return ctx.pick_stale(width, height, n, r, src.data_ptr() if src_ptr is None else src_ptr, order_dev.data_ptr() if order_ptr is None else order_ptr,
                              out.data_ptr() if out_ptr is None else out_ptr, **kw)

    def desc(r=rects, n_rects=None, width=w, height=h, n=n):
        d = abi.StaleDesc()
        d.width, d.height, d.n, d.max_stale, d.flags = width, height, n, n, 1
        d.n_rects = len(r) if n_rects is None else n_rects
        d.rects = r.ctypes.data if r is not None else None
        return d

    def raw_call(desc_ptr, src_ptr, order_ptr, out_ptr, info_ptr):
        ctx._check(ctx._lib.aic_pick_stale(ctx._h, desc_ptr, C.c_void_p(src_ptr), C.c_void_p(order_ptr), C.c_void_p(out_ptr), info_ptr))

    good("before")
    info = abi.StaleInfo()
    rejected(lambda: raw_call(None, src.data_ptr(), order_dev.data_ptr(), out.data_ptr(), C.byref(info)), "NULL desc")
    rejected(lambda: raw_call(C.byref(desc()), src.data_ptr(), order_dev.data_ptr(), out.data_ptr(), None), "NULL info")
    rejected(lambda: raw_call(C.byref(desc()), src.data_ptr(), order_dev.data_ptr(), None, C.byref(info)), "NULL pixels_out with n > 0")
    rejected(lambda: raw_call(C.byref(desc()), None, order_dev.data_ptr(), out.data_ptr(), C.byref(info)), "NULL src with the depth test")
    rejected(lambda: raw_call(C.byref(desc(r=None, n_rects=2)), src.data_ptr(), order_dev.data_ptr(), out.data_ptr(), C.byref(info)), "NULL rects with n_rects > 0")
    for off in (1, 2, 3):
        rejected(lambda: call(out_ptr=out.data_ptr() + off), f"pixels_out at {off} bytes")
        rejected(lambda: call(order_ptr=order_dev.data_ptr() + off), f"order at {off} bytes")
    for off in (1, 4, 7):
        rejected(lambda: call(src_ptr=src.data_ptr() + off), f"src at {off} bytes")
        rejected(lambda: call(src_ptr=src.data_ptr() + off, flags=0), f"src at {off} bytes, no depth test")
    for ww, hh in ((0, h), (w, 0), (0, 0)):
        rejected(lambda: call(width=ww, height=hh, r=rect_sets(w, h)["none"]), f"n > 0 in an empty frame {ww}x{hh}")
    rejected(lambda: call(width=65536, height=1, r=rect_sets(w, h)["none"]), "width above 65535")
    rejected(lambda: call(width=1, height=65536, r=rect_sets(w, h)["none"]), "height above 65535")
    rejected(lambda: call(n=MAX_PICKS + 1), "n above 2048 x 65535")
    for flags in (2, 3, 1 << 31):
        rejected(lambda: call(flags=flags), f"flags {flags}")
    rejected(lambda: call(r=recs([(0, 0, 1, 1, 0.5)] * (abi.STALE_MAX_RECTS + 1))), "n_rects above the cap")
    for what, bad in [("x0 > x1", (9, 2, 8, 5, 0.5)), ("y0 > y1", (2, 9, 5, 8, 0.5)), ("x1 > width", (2, 2, w + 1, 5, 0.5)), ("y1 > height", (2, 2, 5, h + 1, 0.5)),
                      ("NaN dmin", (2, 2, 5, 5, np.nan))]:
        rejected(lambda: call(r=recs([(1, 1, 4, 4, 0.5), bad])), what)
        rejected(lambda: call(r=recs([bad]), flags=0), what + ", no depth test")
    # a frame still occupying slot 0
    ctx.upload_space(abi.LAYER_WORLD, scenes.one_cube_space())
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    eye = (0.7, 0.9, 2.5)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, 40 / 24, oracle.look_at_y_up(eye, (0.5, 0.5, 0.5)), eye)
    busy = rp.device_bytes(40 * 24 * 4)
    ctx.render_submit(ctx.make_frame(40, 24, world_inv=inv), busy.data_ptr(), 0)
    with pytest.raises(abi.AicError) as err:
        call()
    assert err.value.code == AIC_ERR_INVALID, "slot 0 busy"
    ctx.render_wait(0)
    ctx.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all()
    good("after slot 0 busy")
    # the cap itself is fine
    full = recs([(1, 1, 4, 4, 0.5)] * abi.STALE_MAX_RECTS)
    got, got_info = pick(ctx, w, h, full, src, None, 12, max_stale=12, flags=0)
    assert got_info["n_stale"] == 9 and (got[:9] == [y * w + x for y in (1, 2, 3) for x in (1, 2, 3)]).all()
    # n = 0 and an empty frame: AIC_OK, nothing written, the info zeroed -- a NULL list and a NULL frame are then fine
    for ww, hh, out_ptr, src_ptr in ((w, h, out.data_ptr(), src.data_ptr()), (w, h, None, None), (0, h, out.data_ptr(), None), (0, 0, None, None)):
        d = desc(r=rect_sets(w, h)["none"], width=ww, height=hh, n=0)
        C.memset(C.byref(info), 0xFF, C.sizeof(info))
        raw_call(C.byref(d), src_ptr, order_dev.data_ptr(), out_ptr, C.byref(info))
        assert bytes(info) == bytes(C.sizeof(info))
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all()
    good("after the empty calls")
    torch.cuda.synchronize()
