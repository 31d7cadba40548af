"""GPU tests (-m gpu) of aic_pick_stale_cubes and aic_probe_stale_cube_rects: changed boxes and changed light cubes projected, marked and compacted on
the device.

Yardstick: tests/stale_cubes_ref.py, the restatement of DESIGN.md 4.19 in NumPy and Python numbers. Rectangles are compared bit for bit in all six
fields; whole uint32 lists, every info field and the guard words behind pixels_out[n) are compared; there is no tolerance anywhere. Sizes: 61 x 37 (rows
of two bitmap words, the second with 29 pixels; 9 scan blocks), 300 x 220 (rows of ten words, 258 scan blocks) and 523 x 503 (rows of 17 words, 1028
scan blocks: the scan's second round). Cameras, cube sets, frames and expected lists are made once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi
from tests import pick_ref, scenes, stale_ref
from tests import stale_cubes_ref as ref
from tests import test_gpu_pick as pk
from tests import test_gpu_reproject as rp
from tests import test_gpu_stale as gs
from tests import test_stale_cpu as sc

gpu = pytest.mark.gpu

SIZES = gs.SIZES
ORDERS = gs.ORDERS
SENTINEL_WORD = pk.SENTINEL_WORD
AIC_ERR_INVALID = 1
MAX_PICKS = 2048 * 65535
FLAGS = [0, ref.DEPTH_TEST, ref.DEPTH_BEHIND, ref.DEPTH_TEST | ref.DEPTH_BEHIND]
EYE, TARGET = (4.3, 4.0, 10.0), (4.0, 1.0, 4.0)
SETS = ["one", "257", "5000", "whole", "boxes_only"]


@functools.lru_cache(maxsize=None)
def view_projection(w, h):
    projection, world_to_eye, _ = oracle.camera_matrices(90.0, 200.0, w / h, oracle.look_at_y_up(EYE, TARGET), EYE)
    vp = (world_to_eye @ projection).reshape(16).copy()
    vp.setflags(write=False)
    return vp


@functools.lru_cache(maxsize=None)
def cube_set(name):
    """(boxes [n, 6] int32, light cubes [n, 3] int32). The cubes lie in a slab in front of the camera with neighbours and repeats among them (overlapping
    rectangles), some far to each side, above and below (rectangles that touch each frame edge, and dropped ones); "whole" adds the cube the eye is in
    and one behind the camera, whose grown boxes have corners behind the camera: the whole-frame rectangle."""
    rng = np.random.default_rng(11)
    n = {"one": 1, "257": 257, "5000": 5000, "whole": 258, "boxes_only": 0}[name]
    if name == "one":
        cubes = [[4, 1, 4]]
    else:
        m = 257 if name == "whole" else n
        cubes = [[int(v) for v in rng.integers((-6, -2, -12), (14, 6, 6))] for _ in range(m)]
        for i in range(0, m - 1, 5):  # a neighbour or a repeat of the cube before
            cubes[i + 1] = [c + int(d) for c, d in zip(cubes[i], rng.integers(0, 2, 3))]
        cubes[2:10] = [[-30, 1, 4], [40, 1, 4], [4, 14, -20], [4, -30, 2], [4, 0, 8], [4, 1, -150], [-3, 0, 7], [11, 3, 7]][:max(0, min(8, m - 2))]
        if name == "whole":
            cubes.insert(100, [4, 4, 10])
            cubes[200] = [4, 1, 30]  # behind the camera: the whole frame too
    boxes = [[2, 1, 2, 3, 2, 3], [4, 1, 4, 6, 2, 5], [3, 2, 5, 3, 3, 6]] if name in ("257", "boxes_only") else []  # (the last has no volume)
    b, q = np.array(boxes, np.int32).reshape(-1, 6), np.array(cubes, np.int32).reshape(-1, 3)
    assert len(q) == n
    b.setflags(write=False)
    q.setflags(write=False)
    return b, q


@functools.lru_cache(maxsize=None)
def rects_of(w, h, name):
    b, q = cube_set(name)
    r = ref.rects(view_projection(w, h), w, h, b, q, 1)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def frame(w, h):
    """tests/test_gpu_stale.py's synthetic frame (sign-bit depths, -0.0, NaN depths, marker texels, NaN alpha, alpha exactly 1 and just below), and in
    rectangles of the "257" set depths equal to their dmin and dmax and one f32 step either side of each, under alpha 1 and under alpha 0.5."""
    color, depth = (a.copy() for a in gs.frame(w, h))
    rng = np.random.default_rng(5 * w + h)
    planted = 0
    for r in rects_of(w, h, "257"):
        x0, y0, x1, y1 = int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])
        if (x1 - x0) * (y1 - y0) < 12 or not np.isfinite(r["dmin"]) or rng.random() < 0.5:
            continue
        cells = rng.choice((x1 - x0) * (y1 - y0), 12, replace=False)
        values = [v for d in (r["dmin"], r["dmax"]) for v in (d, np.nextafter(d, np.float32(-np.inf)), np.nextafter(d, np.float32(np.inf)))]
        for k, cell in enumerate(cells):
            y, x = y0 + int(cell) // (x1 - x0), x0 + int(cell) % (x1 - x0)
            depth[y, x] = values[k % 6]
            color[y, x, 3] = np.float16(1.0 if k < 6 else 0.5).view(np.uint16)
        planted += 1
    assert planted >= 20
    color.setflags(write=False)
    depth.setflags(write=False)
    return color, depth


@functools.lru_cache(maxsize=None)
def mask_of(w, h, name, flags):
    color, depth = frame(w, h)
    m = ref.stale_mask(w, h, rects_of(w, h, name), len(cube_set(name)[0]), color, depth, flags)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ranks_of(w, h, kind, name, flags):
    r = stale_ref.rank_list(mask_of(w, h, name, flags), gs.order_of(w, h, kind))
    r.setflags(write=False)
    return r


def expected(w, h, kind, name, flags, n, max_stale=0, skip_stale=0, cursor=0):
    """ref.pick_list, with the rank list and the picker part taken from the shared copies"""
    rl = rects_of(w, h, name)
    look = max_stale > 0 and len(rl) > 0
    ranks = ranks_of(w, h, kind, name, flags) if look else np.zeros(0, np.uint32)
    g = pick_ref.taken(n, max_stale, len(ranks), skip_stale)
    want = np.concatenate([ranks[skip_stale:skip_stale + g], gs.picker_list(w, h, kind, n - g, cursor)]).astype(np.uint32)
    info = {"n_stale": len(ranks), "next_cursor": (cursor + n - g) % 2**64, "n_from_stale": g, "n_from_order": n - g,
            "n_rects": int(((rl["x0"] < rl["x1"]) & (rl["y0"] < rl["y1"])).sum()) if look else 0,
            "whole_frame": int(ref.whole_frame(w, h, rl, len(cube_set(name)[0]), flags)) if look else 0}
    return want, info


def info_dict(info):
    return {k: getattr(info, k) for k in ("n_stale", "next_cursor", "n_from_stale", "n_from_order", "n_rects", "whole_frame")}


def pick(ctx, w, h, name, src, order_dev, n, **kw):
    """One call into a fresh list: (pixels_out [n] uint32, info fields); the guard words behind it are checked here."""
    out = pk.out_words(n)
    b, q = cube_set(name)
    info = ctx.pick_stale_cubes(view_projection(w, h), w, h, n, b, q, src.data_ptr() if src is not None else 0, order_dev.data_ptr() if order_dev is not None else 0,
                                out.data_ptr(), **kw)
    raw = out.cpu().numpy().view(np.uint32)
    assert (raw[n:] == SENTINEL_WORD).all(), "guard words behind pixels_out[n)"
    assert info.kernel_ms >= 0.0 and info.reserved == 0
    return raw[:n].copy(), info_dict(info)


def check(ctx, w, h, kind, name, flags, src, order_dev, n, what, **kw):
    want, want_info = expected(w, h, kind, name, flags, n, **kw)
    got, got_info = pick(ctx, w, h, name, src, order_dev, n, flags=flags, **kw)
    differing = int((got != want).sum())
    print(f"{w}x{h} {kind} {name} flags {flags} {what}: n {n} {kw} -> {got_info}; entries differing {differing}")
    assert got_info == want_info, what
    assert differing == 0, what
    return got


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def test_the_cases_are_not_vacuous():
    """(no device needed) From the restatement alone: rectangles touch each frame edge, overlap, are dropped; "whole" has the whole-frame rectangle; both
    depth tests keep pixels out and leave pixels in; depths exactly at a bound are stale and one step beyond it are kept out."""
    for w, h in SIZES:
        r = rects_of(w, h, "257")
        full = (r["x0"] < r["x1"]) & (r["y0"] < r["y1"])
        assert (r["x0"][full] == 0).any() and (r["y0"][full] == 0).any() and (r["x1"][full] == w).any() and (r["y1"][full] == h).any()
        assert 0 < (~full).sum() and full.sum() > 100
        assert not ref.whole_frame(w, h, r, 3, 0) and ref.whole_frame(w, h, rects_of(w, h, "whole"), 0, 3)
        area = ((r["x1"] - r["x0"]).astype(np.int64) * (r["y1"] - r["y0"])).sum()
        plain = mask_of(w, h, "257", 0)
        assert plain.sum() < area, "rectangles overlap"
        front, behind, both = (mask_of(w, h, "257", f) for f in FLAGS[1:])
        assert 0 < both.sum() < min(front.sum(), behind.sum()) and max(front.sum(), behind.sum()) < plain.sum() <= w * h
        assert mask_of(w, h, "whole", 3).all() and len(rects_of(w, h, "5000")) == 5000
    w, h = 61, 37
    color, depth = frame(w, h)
    one = rects_of(w, h, "one")
    assert len(one) == 1 and np.isfinite(one[0]["dmax"]) and one[0]["dmin"] < one[0]["dmax"]
    r = one[0]
    y, x = int(r["y0"]), int(r["x0"])
    for d, alpha, flags, stale in [(r["dmax"], 0.5, 2, True), (np.nextafter(r["dmax"], np.float32(np.inf)), 0.5, 2, False), (np.nextafter(r["dmax"], np.float32(np.inf)), np.nan, 2, True), (np.nextafter(r["dmax"], np.float32(np.inf)), -1.0, 2, True),
                                   (-np.nextafter(r["dmax"], np.float32(np.inf)), 0.5, 2, True), (r["dmin"], 1.0, 1, True), (np.nextafter(r["dmin"], np.float32(-np.inf)), 1.0, 1, False),
                                   (np.nextafter(r["dmin"], np.float32(-np.inf)), 0.5, 1, True), (np.nextafter(r["dmin"], np.float32(-np.inf)), 0.5, 3, True), (np.float32(np.nan), 1.0, 3, True)]:
        c2, d2 = color.copy(), depth.copy()
        d2[y, x] = d
        c2[y, x, 3] = np.float16(alpha).view(np.uint16)
        assert ref.stale_mask(w, h, one, 0, c2, d2, flags).reshape(h, w)[y, x] == stale, (d, alpha, flags)
    # a box never uses the behind test
    c2, d2 = color.copy(), depth.copy()
    d2[:] = 1.0
    c2[..., 3] = np.float16(0.5).view(np.uint16)
    assert ref.stale_mask(w, h, one, 1, c2, d2, 2).sum() == (int(r["x1"]) - x) * (int(r["y1"]) - y)
    assert ref.stale_mask(w, h, one, 0, c2, d2, 2).sum() == 0


@gpu
@pytest.mark.parametrize("w,h", [(61, 37), (523, 503)])
def test_probe_equals_the_restatement_bit_for_bit(ctx, w, h):
    """Six random perspective cameras and an orthographic one; boxes and cubes in front, straddling the camera plane, behind, off-screen, of no volume,
    at the i32 edges; expand 0, 1, 3."""
    rng = np.random.default_rng(w)
    cams = [sc.perspective(rng, w, h) for _ in range(6)] + [(sc.orthographic(), (3.0, 2.0, -10.0), (3.0, 2.0, 0.0))]
    kinds = {"whole": 0, "empty": 0, "proper": 0}
    for vp, eye, target in cams:
        b = sc.boxes_around(rng, eye, target)
        q = np.concatenate([b[:, :3], b[:, 3:] - 1, [[2**31 - 1] * 3, [-2**31] * 3, [2**31 - 1, 0, -2**31]]]).astype(np.int32)
        for expand in (0, 1, 3):
            got = ctx.probe_stale_cube_rects(vp, w, h, b, q, expand)
            want = ref.rects(vp, w, h, b, q, expand)
            assert got.tobytes() == want.tobytes(), (expand, got[got != want][:3], want[got != want][:3])
            # the boxes' first five fields are aic_stale_rects' own
            host = abi.stale_rects(vp, w, h, b, expand)
            for f in ("x0", "y0", "x1", "y1"):
                assert (got[f][:len(b)] == host[f]).all()
            assert got["dmin"][:len(b)].tobytes() == host["dmin"].tobytes()
            for r in want:
                whole = (r["x0"], r["y0"], r["x1"], r["y1"]) == (0, 0, w, h) and r["dmin"] == -np.inf and r["dmax"] == np.inf
                kinds["whole" if whole else ("empty" if r["x1"] == 0 else "proper")] += 1
        assert len(ctx.probe_stale_cube_rects(vp, w, h, b, None, 1)) == len(b) and len(ctx.probe_stale_cube_rects(vp, w, h, None, q, 1)) == len(q)
    print(kinds)
    assert all(v > 20 for v in kinds.values()), kinds
    assert len(ctx.probe_stale_cube_rects(sc.orthographic(), 5, 5, None, None)) == 0


@gpu
@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("w,h", SIZES)
def test_lists_equal_the_restatement(ctx, w, h, kind):
    color, depth = frame(w, h)
    src_bytes = rp.frame_bytes(color, depth)
    src = rp.to_device(src_bytes)
    order_dev = pk.to_device_words(gs.picker_order(w, h)) if kind == "picker" else None
    large = w * h > 100000
    for name in SETS:
        assert (ctx.probe_stale_cube_rects(view_projection(w, h), w, h, *cube_set(name)).tobytes() == rects_of(w, h, name).tobytes()), name
        for flags in FLAGS:
            ns = len(ranks_of(w, h, kind, name, flags))
            n = ns + 7
            first = check(ctx, w, h, kind, name, flags, src, order_dev, n, "all of S and 7 picks", max_stale=n)
            again = check(ctx, w, h, kind, name, flags, src, order_dev, n, "the same call twice", max_stale=n)
            assert (first == again).all()
            if large and name not in ("257", "whole"):
                continue
            if ns >= 3:
                check(ctx, w, h, kind, name, flags, src, order_dev, ns - 1, "n < n_stale", max_stale=ns - 1)
                check(ctx, w, h, kind, name, flags, src, order_dev, ns - 1, "max_stale < n < n_stale", max_stale=(ns - 1) // 2, cursor=2**40 + 3)
            for skip in (1, ns - 1, ns, ns + 5):
                if skip >= 0:
                    check(ctx, w, h, kind, name, flags, src, order_dev, 70, "skip", max_stale=70, skip_stale=skip, cursor=9)
            check(ctx, w, h, kind, name, flags, src, order_dev, 70, "max_stale = 0", cursor=w * h // 2 - 1)
    # no boxes and no cubes: nothing is looked at
    out = pk.out_words(50)
    info = ctx.pick_stale_cubes(view_projection(w, h), w, h, 50, None, None, src.data_ptr(), 0 if order_dev is None else order_dev.data_ptr(), out.data_ptr(), max_stale=50, flags=3, cursor=4)
    assert info_dict(info) == {"n_stale": 0, "next_cursor": 54, "n_from_stale": 0, "n_from_order": 50, "n_rects": 0, "whole_frame": 0}
    assert (out.cpu().numpy().view(np.uint32)[:50] == gs.picker_list(w, h, kind, 50, 4)).all()
    # without a depth flag the frame is not read, and the behind test is a light cube's alone: no frame will do
    check(ctx, w, h, kind, "257", 0, None, order_dev, 50, "NULL src without a depth flag", max_stale=50)
    check(ctx, w, h, kind, "boxes_only", 2, None, order_dev, 50, "NULL src, boxes under the behind flag", max_stale=50)
    assert (src.cpu().numpy() == src_bytes).all(), "src is only read"


@gpu
def test_an_order_entry_that_is_no_pixel_is_never_stale(ctx):
    w, h = 61, 37
    count = w * h
    color, depth = frame(w, h)
    src = rp.to_device(rp.frame_bytes(color, depth))
    order = gs.picker_order(w, h).copy()
    order[[0, 5, 300, count - 1]] = [count, 0xFFFFFFFF, count + 7, 2**31]
    for name, flags in [("whole", 0), ("whole", 3), ("257", 2)]:
        b, q = cube_set(name)
        want, want_info = ref.pick_list(view_projection(w, h), w, h, order, count, b, q, 1, color, depth, flags, max_stale=count, rect_list=rects_of(w, h, name))
        out = pk.out_words(count)
        info = ctx.pick_stale_cubes(view_projection(w, h), w, h, count, b, q, src.data_ptr(), pk.to_device_words(order).data_ptr(), out.data_ptr(), max_stale=count, flags=flags)
        assert info_dict(info) == want_info and (out.cpu().numpy().view(np.uint32)[:count] == want).all()
        assert name != "whole" or info.n_stale == count - 4


@gpu
def test_rejections_leave_the_context_usable(ctx):
    import torch

    w, h = 61, 37
    color, depth = frame(w, h)
    src_bytes = rp.frame_bytes(color, depth)
    src = rp.to_device(src_bytes)
    order_dev = pk.to_device_words(gs.picker_order(w, h))
    b, q = cube_set("257")
    vp = view_projection(w, h)
    n = 40
    out = pk.out_words(n + 4)
    rect_out = np.full(len(b) + len(q), 0xA5, np.uint8).repeat(24).view(ref.CUBE_RECT_DTYPE)
    assert out.data_ptr() % 4 == 0 and order_dev.data_ptr() % 4 == 0 and src.data_ptr() % 8 == 0

    def good(what):
        check(ctx, w, h, "picker", "257", 3, src, order_dev, n, what, max_stale=n, skip_stale=1, cursor=9)

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all(), what
        assert (src.cpu().numpy() == src_bytes).all(), what
        assert (rect_out.view(np.uint8) == 0xA5).all(), what
        good(what)

    def desc(m=vp, width=w, height=h, n=n, boxes=b, cubes=q, n_boxes=None, n_cubes=None, expand=1, flags=3):
        d = abi.StaleCubesDesc()
        d.width, d.height, d.n, d.max_stale, d.flags, d.expand = width, height, n, n, flags, expand
        d.view_projection = (C.c_double * 16)(*m)
        d.n_boxes = (len(boxes) if boxes is not None else 0) if n_boxes is None else n_boxes
        d.n_light_cubes = (len(cubes) if cubes is not None else 0) if n_cubes is None else n_cubes
        d.boxes = boxes.ctypes.data if boxes is not None and len(boxes) else None
        d.light_cubes = cubes.ctypes.data if cubes is not None and len(cubes) else None
        return d

    info = abi.StaleCubesInfo()

    def raw_call(d, src_ptr=-1, order_ptr=-1, out_ptr=-1, info_ptr=-1):
        ptr = lambda v, default: default if v == -1 else v
        ctx._check(ctx._lib.aic_pick_stale_cubes(ctx._h, None if d is None else C.byref(d), C.c_void_p(ptr(src_ptr, src.data_ptr())), C.c_void_p(ptr(order_ptr, order_dev.data_ptr())),
                                                 C.c_void_p(ptr(out_ptr, out.data_ptr())), ptr(info_ptr, C.byref(info))))

    def raw_probe(d, dst=-1):
        ctx._check(ctx._lib.aic_probe_stale_cube_rects(ctx._h, None if d is None else C.byref(d), C.c_void_p(rect_out.ctypes.data if dst == -1 else dst)))

    good("before")
    rejected(lambda: raw_call(None), "NULL desc")
    rejected(lambda: raw_call(desc(), info_ptr=None), "NULL info")
    rejected(lambda: raw_call(desc(), out_ptr=None), "NULL pixels_out with n > 0")
    rejected(lambda: raw_call(desc(flags=1), src_ptr=None), "NULL src with the front test")
    rejected(lambda: raw_call(desc(flags=2), src_ptr=None), "NULL src with the behind test and light cubes")
    rejected(lambda: raw_call(desc(boxes=None, n_boxes=2)), "NULL boxes with n_boxes > 0")
    rejected(lambda: raw_call(desc(cubes=None, n_cubes=2)), "NULL light_cubes with n_light_cubes > 0")
    rejected(lambda: raw_call(desc(n_boxes=2**32 - 1)), "n_boxes + n_light_cubes above 2^32 - 1")
    for off in (1, 2, 3):
        rejected(lambda: raw_call(desc(), out_ptr=out.data_ptr() + off), f"pixels_out at {off} bytes")
        rejected(lambda: raw_call(desc(), order_ptr=order_dev.data_ptr() + off), f"order at {off} bytes")
    for off in (1, 4, 7):
        rejected(lambda: raw_call(desc(), src_ptr=src.data_ptr() + off), f"src at {off} bytes")
        rejected(lambda: raw_call(desc(flags=0), src_ptr=src.data_ptr() + off), f"src at {off} bytes, no depth flag")
    for ww, hh in ((0, h), (w, 0), (0, 0)):
        rejected(lambda: raw_call(desc(width=ww, height=hh)), f"n > 0 in an empty frame {ww}x{hh}")
    rejected(lambda: raw_call(desc(width=65536, height=1)), "width above 65535")
    rejected(lambda: raw_call(desc(width=1, height=65536)), "height above 65535")
    rejected(lambda: raw_call(desc(n=MAX_PICKS + 1)), "n above 2048 x 65535")
    for flags in (4, 7, 1 << 31):
        rejected(lambda: raw_call(desc(flags=flags)), f"flags {flags}")
    rejected(lambda: raw_call(desc(expand=-1)), "negative expand")
    rejected(lambda: raw_probe(desc(expand=-1)), "negative expand, probe")
    for bad in (np.nan, np.inf, -np.inf):
        for i in (0, 7, 15):
            m = vp.copy()
            m[i] = bad
            rejected(lambda: raw_call(desc(m=m)), f"matrix component {i} = {bad}")
            rejected(lambda: raw_probe(desc(m=m)), f"matrix component {i} = {bad}, probe")
    rejected(lambda: raw_probe(None), "NULL desc, probe")
    rejected(lambda: raw_probe(desc(), dst=None), "NULL out, probe")
    rejected(lambda: raw_probe(desc(boxes=None, n_boxes=1)), "NULL boxes, probe")
    rejected(lambda: raw_probe(desc(cubes=None, n_cubes=1)), "NULL light cubes, probe")
    rejected(lambda: raw_probe(desc(width=65536)), "width above 65535, probe")
    # a frame still occupying slot 0
    ctx.upload_space(abi.LAYER_WORLD, scenes.one_cube_space())
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    eye = (0.7, 0.9, 2.5)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, 40 / 24, oracle.look_at_y_up(eye, (0.5, 0.5, 0.5)), eye)
    busy = rp.device_bytes(40 * 24 * 4)
    ctx.render_submit(ctx.make_frame(40, 24, world_inv=inv), busy.data_ptr(), 0)
    for fn in (lambda: raw_call(desc()), lambda: raw_probe(desc())):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, "slot 0 busy"
    ctx.render_wait(0)
    ctx.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all() and (rect_out.view(np.uint8) == 0xA5).all()
    good("after slot 0 busy")
    # n = 0 and an empty frame: AIC_OK, nothing written, the info zeroed -- a NULL list and a NULL frame are then fine
    for ww, hh, out_ptr, src_ptr in ((w, h, -1, -1), (w, h, None, None), (0, h, -1, None), (0, 0, None, None)):
        C.memset(C.byref(info), 0xFF, C.sizeof(info))
        raw_call(desc(width=ww, height=hh, n=0), src_ptr=src_ptr, out_ptr=out_ptr)
        assert bytes(info) == bytes(C.sizeof(info))
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all()
    good("after the empty calls")
    torch.cuda.synchronize()


# ---- the light report (aic_light_changed_count / _take) and the loop it closes ----------------------------------------------------------------------

from tests import stale_light_scenes as L  # noqa: E402
from tests.test_gpu_parity import to_abi_options  # noqa: E402

WORLD = abi.LAYER_WORLD


def volume_diff(sp, before, after):
    """the cubes whose texel differs, [n, 3] int32 ascending in the volume's cube index"""
    return (np.argwhere((before != after).any(-1)) + np.asarray(sp.lo)).astype(np.int32)


def edit_and_queue(ctx, name):
    """aic_update_cubes + aic_light_cubes_changed of the case's edits"""
    _, edits = L.case(name)
    cubes = [cube for cube, _ in edits]
    ctx.update_cubes(WORLD, cubes, [index for _, index in edits])
    ctx.light_cubes_changed(WORLD, cubes)


def drain(ctx, **kw):
    return ctx.evaluate_light(WORLD, L.MAXIMUM_DISTANCE, fast=False, queue=[], **kw)


def bounds_of(xyz):
    return np.concatenate([xyz.min(0), xyz.max(0) + 1]).astype(np.int32) if len(xyz) else np.zeros(6, np.int32)


@gpu
@pytest.mark.parametrize("name", L.CASES)
def test_the_light_report_is_the_volume_diff_and_the_oracles(ctx, name):
    sp, _ = L.case(name)
    ctx.upload_space(WORLD, sp)
    assert ctx.light_changed(WORLD, take=False)[0] == 0
    before = ctx.read_light_volume(WORLD, sp.size)
    edit_and_queue(ctx, name)
    info = drain(ctx)
    after = ctx.read_light_volume(WORLD, sp.size)
    want = volume_diff(sp, before, after)
    n, bounds = ctx.light_changed(WORLD, take=False)
    assert n == len(want) and (bounds == bounds_of(want)).all()
    assert ctx.light_changed(WORLD, take=False)[0] == n, "a count consumes nothing"
    xyz, bounds = ctx.light_changed(WORLD)
    print(f"{name}: {info.updates} updates, {len(xyz)} cubes reported, bounds {bounds.tolist()}")
    assert xyz.dtype == np.int32 and xyz.tolist() == want.tolist(), "exactly the diff, in cube index order"
    assert xyz.tolist() == L.relit(name)[1].tolist() and info.updates == L.relit(name)[2], "the oracle's relight"
    assert (after == L.relit(name)[0].light).all()
    again, bounds = ctx.light_changed(WORLD)
    assert len(again) == 0 and (bounds == 0).all() and ctx.light_changed(WORLD, take=False)[0] == 0


@gpu
def test_the_callers_own_texels_are_not_reported(ctx):
    name = "plaza"
    sp, _ = L.case(name)
    ctx.upload_space(WORLD, sp)
    ctx.read_light_cubes(WORLD, [(0, 0, 0)])  # (the updater's host mirrors exist from here on: the harder case)
    cubes = [(1, 1, 1), (2, 2, 2), (7, 3, 7)]
    ctx.update_cubes(WORLD, cubes, light=[[9, 8, 7, 1], [1, 2, 3, 1], [0, 0, 0, 1]])
    assert ctx.light_changed(WORLD, take=False)[0] == 0, "the light of aic_update_cubes"
    volume = ctx.read_light_volume(WORLD, sp.size)
    volume[3:6, 1:3, 2:5] = (40, 50, 60, 1)
    ctx.update_light_volume(WORLD, volume)
    assert ctx.light_changed(WORLD, take=False)[0] == 0, "aic_update_light_volume"
    # the updater's changes stay reported through both, except where the caller has written since
    before = ctx.read_light_volume(WORLD, sp.size)
    edit_and_queue(ctx, name)
    drain(ctx)
    after = ctx.read_light_volume(WORLD, sp.size)
    want = volume_diff(sp, before, after)
    assert len(want) >= 20 and ctx.light_changed(WORLD, take=False)[0] == len(want)
    ctx.update_cubes(WORLD, [want[0]], light=[[77, 77, 77, 1]])
    volume = after.copy()
    volume[tuple(want[0] - sp.lo)] = (77, 77, 77, 1)
    x, y, z = want[-1] - sp.lo
    volume[x, y, z] = (5, 5, 5, 1)
    ctx.update_light_volume(WORLD, volume)
    xyz, _ = ctx.light_changed(WORLD)
    assert xyz.tolist() == want[1:-1].tolist()


@gpu
def test_a_submitted_update_is_reported_when_it_is_published(ctx):
    name = "terrace"
    sp, _ = L.case(name)
    ctx.upload_space(WORLD, sp)
    edit_and_queue(ctx, name)
    stored = ctx.light_changed(WORLD, take=False)[0]  # the OPAQUE texels aic_light_cubes_changed stored at once: published already
    assert stored >= 1
    ctx.evaluate_light_submit(WORLD, L.MAXIMUM_DISTANCE, fast=False, queue=[])
    assert ctx.light_changed(WORLD, take=False)[0] == stored, "nothing of the update before it is published"
    while not ctx.evaluate_light_done(WORLD):
        pass
    assert ctx.light_changed(WORLD, take=False)[0] == stored, "finished is not published"
    info = ctx.evaluate_light_wait(WORLD)
    xyz, _ = ctx.light_changed(WORLD)
    assert info.updates == L.relit(name)[2] and xyz.tolist() == L.relit(name)[1].tolist()
    # a take ends and publishes an update that nobody has waited for yet; its outcome stays for the wait
    ctx.upload_space(WORLD, sp)
    edit_and_queue(ctx, name)
    ctx.evaluate_light_submit(WORLD, L.MAXIMUM_DISTANCE, fast=False, queue=[])
    xyz, _ = ctx.light_changed(WORLD)
    assert xyz.tolist() == L.relit(name)[1].tolist()
    assert ctx.evaluate_light_wait(WORLD).updates == L.relit(name)[2]
    assert (ctx.read_light_volume(WORLD, sp.size) == L.relit(name)[0].light).all()


@gpu
def test_budgets_accumulate_fast_reports_the_whole_diff_and_a_small_capacity_is_refused(ctx):
    name = "behind_wall"
    sp, _ = L.case(name)
    ctx.upload_space(WORLD, sp)
    before = ctx.read_light_volume(WORLD, sp.size)
    edit_and_queue(ctx, name)
    calls = 0
    while True:
        info = drain(ctx, max_updates=8, batch=4)
        calls += 1
        if info.queue_left == 0:
            break
    after = ctx.read_light_volume(WORLD, sp.size)
    want = volume_diff(sp, before, after)
    assert calls >= 3 and len(want) >= 20
    # capacity below the count: refused, nothing written, nothing consumed
    xyz = np.full((len(want), 3), 0x5A5A5A5A, np.int32)
    written = C.c_uint32(0xFFFF)
    rc = ctx._lib.aic_light_changed_take(ctx._h, WORLD, len(want) - 1, C.c_void_p(xyz.ctypes.data), C.byref(written))
    assert rc == AIC_ERR_INVALID and (xyz == 0x5A5A5A5A).all() and written.value == 0xFFFF
    assert ctx.light_changed(WORLD, take=False)[0] == len(want)
    got, _ = ctx.light_changed(WORLD)
    assert got.tolist() == want.tolist()
    # fast = 1: the diff against the volume as it was
    before = after
    ctx.evaluate_light(WORLD, L.MAXIMUM_DISTANCE, fast=True)
    after = ctx.read_light_volume(WORLD, sp.size)
    got, _ = ctx.light_changed(WORLD)
    assert got.tolist() == volume_diff(sp, before, after).tolist()
    for bad in (lambda: ctx._lib.aic_light_changed_count(ctx._h, WORLD, None, None), lambda: ctx._lib.aic_light_changed_count(ctx._h, 7, C.byref(C.c_uint64()), None),
                lambda: ctx._lib.aic_light_changed_take(ctx._h, WORLD, 4, None, C.byref(written)), lambda: ctx._lib.aic_light_changed_take(ctx._h, WORLD, 0, None, None)):
        assert bad() == AIC_ERR_INVALID


def load_relit_case(ctx, name, antialiasing):
    """Uploads space A of the case; returns (the Split frame's description, view_projection)."""
    sp, _ = L.case(name)
    inv, vp, zw = L.S.camera(L.base(name))
    ctx.upload_space(WORLD, sp)
    ctx.set_options(WORLD, to_abi_options(L.S.options(antialiasing)))
    ctx.clear_space(abi.LAYER_UI)
    ctx.set_depth_transform(zw)
    return ctx.make_frame(L.W, L.HT, world_inv=inv, flags=abi.FRAME_OUT_SPLIT), vp


@gpu
@pytest.mark.parametrize("antialiasing", L.ANTIALIASING)
@pytest.mark.parametrize("name", L.CASES)
def test_an_edit_and_its_relight_are_complete_after_tracing_the_stale_pixels(ctx, name, antialiasing):
    """A resident Split frame of A; the edits, the relight, the take; every stale pixel of aic_pick_stale_cubes (boxes + light cubes, the behind test)
    traced in place: the resident frame is a fresh Split render of B' byte for byte, and n_stale is the value tests/test_stale_cubes_cpu.py finds."""
    w, h = L.W, L.HT
    count = w * h
    try:
        f, vp = load_relit_case(ctx, name, antialiasing)
        resident = rp.device_bytes(count * 12)
        ctx.render_submit(f, resident.data_ptr(), 0)
        ctx.render_wait(0)
        ctx.synchronize()
        before = resident.cpu().numpy().copy()
        edit_and_queue(ctx, name)
        drain(ctx)
        cubes, _ = ctx.light_changed(WORLD)
        assert cubes.tolist() == L.relit(name)[1].tolist()
        s, want_rects = L.stale_set(name, antialiasing, ref.DEPTH_BEHIND, True)
        assert ctx.probe_stale_cube_rects(vp, w, h, L.boxes(name), cubes, 1).tobytes() == want_rects.tobytes()
        order = gs.picker_order(w, h)
        picks = pk.out_words(count)
        info = ctx.pick_stale_cubes(vp, w, h, count, L.boxes(name), cubes, resident.data_ptr(), pk.to_device_words(order).data_ptr(), picks.data_ptr(), max_stale=count,
                                    flags=ref.DEPTH_BEHIND)
        n_stale = int(s.sum())
        print(f"{name} aa {antialiasing}: {len(cubes)} light cubes, n_stale {info.n_stale} (restated {n_stale}) of {count}, {info.kernel_ms:.3f} ms")
        assert (info.n_stale, info.n_from_stale, info.n_from_order, info.whole_frame) == (n_stale, n_stale, count - n_stale, 0)
        listed = picks.cpu().numpy().view(np.uint32)[:n_stale]
        assert (listed == stale_ref.rank_list(s, order)).all()
        tinfo = ctx.trace_pixels_device(f, n_stale, picks.data_ptr(), resident.data_ptr(), in_place=True)
        assert tinfo.rows_rendered == n_stale
        after = resident.cpu().numpy()
        fresh = ctx.render(f)
        want = rp.frame_bytes(fresh["color_f16"].view(np.uint16), fresh["depth"])
        changed = (before[:count * 8].view(np.uint64) != want[:count * 8].view(np.uint64)) | (before[count * 8:].view(np.uint32) != want[count * 8:].view(np.uint32))
        assert changed.sum() >= 20 and not (changed & ~s).any(), "the edit and the relight show, and only inside S"
        assert (after == want).all()
    finally:
        ctx.set_depth_transform((1.0, 0.0, 0.0, 1.0))


@gpu
def test_host_mirror_refreshes_an_edit_and_its_relight_from_its_own_records():
    """HipRtRenderer with the light on the device: draw_split of plaza's A, the edits through Space.set, update(), evaluate_light() -- which takes the
    changed light cubes --, then pick_stale_cubes() 100 picks a frame until no stale pixel is left, trace_pixels_into each list: the resident frame is
    draw_split of B' byte for byte, every texel outside the lists is untouched, and the lists are the restatement's."""
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H

    w, h = 40, 24
    n = w * h
    name = "plaza"
    sp, edits = L.case(name)
    _, _, eye, target = L.S.case(name)
    cams = H.StandardCameras()
    cams.graphics_options = H.GraphicsOptions()
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    space = A.space_from_flat(sp)
    cams.world_space = space
    cams.world_view_transform = H.look_at_y_up(eye, target)
    r = H.HipRtRenderer(cams)
    r.device_light = True
    assert r.track_light_changes is False
    r.track_light_changes = True
    r.update()
    resident = rp.to_device(rp.split_bytes(r.draw_split()))
    before = resident.cpu().numpy().copy()
    r.update()
    assert r.changed_boxes() == [] and r.changed_light_cubes() == []
    for cube, index in edits:
        space.set(*cube, index)
    r.update()
    info = r.evaluate_light(L.MAXIMUM_DISTANCE, fast=False, continue_queue=True)
    cubes = r.changed_light_cubes()
    assert info["updates"] == L.relit(name)[2] and [list(q) for q in cubes] == L.relit(name)[1].tolist() and r.pick_skip_stale == 0
    projection, world_to_eye, _ = oracle.camera_matrices(90.0, 200.0, w / h, oracle.look_at_y_up(eye, target), eye)
    vp = (world_to_eye @ projection).reshape(16)
    boxes = np.array(r.changed_boxes(), np.int32)
    rects = ref.rects(vp, w, h, boxes, cubes, 1)
    color, depth = before[:n * 8].view(np.uint16).reshape(h, w, 4), before[n * 8:].view(np.float32).reshape(h, w)
    want_s = ref.stale_mask(w, h, rects, len(boxes), color, depth, ref.DEPTH_BEHIND)
    assert 0 < want_s.sum() < ref.stale_mask(w, h, rects, len(boxes)).sum() <= n
    order = abi.pixel_order(w, h)[0]
    order_dev = pk.to_device_words(order)
    per_frame = 100
    listed = []
    for _ in range(n // per_frame + 2):
        picks = pk.out_words(per_frame)
        got = r.pick_stale_cubes(resident.data_ptr(), order_dev.data_ptr(), picks.data_ptr(), per_frame, per_frame, ref.DEPTH_BEHIND)
        if got["n_from_stale"] == 0:
            break
        listed.append(picks.cpu().numpy().view(np.uint32)[:got["n_from_stale"]].copy())
        r.trace_pixels_into(resident.data_ptr(), picks.data_ptr(), got["n_from_stale"])
    listed = np.concatenate(listed)
    # (every call makes the set from the resident frame as it is by then: under the behind test alone it does not move while its pixels are traced -- a
    #  pixel inside a box's rectangle stays whatever its depth, and one inside light rectangles only keeps its geometry, so its depth)
    assert (listed == stale_ref.rank_list(want_s, order)).all() and r.pick_skip_stale == len(listed) == got["n_stale"]
    after = resident.cpu().numpy()
    want = rp.split_bytes(r.draw_split())
    assert (after == want).all()
    rest = np.ones(n, bool)
    rest[listed] = False
    assert (after[:n * 8].view(np.uint64)[rest] == before[:n * 8].view(np.uint64)[rest]).all()
    assert (after[n * 8:].view(np.uint32)[rest] == before[n * 8:].view(np.uint32)[rest]).all()
    assert (before != want).any(), "the edit and the relight show"
    r.clear_changed_light_cubes()
    r.restart_stale()
    assert r.changed_light_cubes() == [] and r.pick_skip_stale == 0
