"""GPU tests (-m gpu) of aic_present_split_lines: a line list drawn on the device into a presented Split frame, depth-tested against the frame's depth
plane, before bloom and tone mapping (all-is-cubes-gpu everything.rs:616-658, shaders/blocks-and-lines.wgsl:902-919, pipelines.rs:453-487).

Yardstick: tests/present_lines_ref.py, the NumPy restatement of DESIGN.md 4.13, on the frames and lists of tests/present_lines_cases.py
(tests/test_present_lines_cpu.py shows from the restatement alone that they hide some fragments, pass others and contest pixels). Without bloom the whole
output of both kinds and every count equal the restatement bit for bit; with bloom the bounds are the chain's own against its restatement (DESIGN.md
4.7, tests/test_gpu_bloom.py): f16 within 2 ulps, RGBA8 within 1 level. S, S' and B of a case are computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi
from tests import present_lines_cases as cases
from tests import present_lines_ref as ref
from tests import present_ref, scenes
from tests.test_gpu_bloom import f16_ulps
from tests.test_gpu_reproject import GUARD, SENTINEL, device_bytes, frame_bytes, to_device

pytestmark = pytest.mark.gpu

EXACT = [(0.0, 0, np.inf), (0.0, 1, 1.0)]  # (bloom_intensity, tone_mapping, maximum_intensity)
BLOOMED = (0.125, 0, np.inf)
KINDS = [(0, np.uint8), (abi.PRESENT_OUT_F16, np.uint16)]
AIC_ERR_INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def counts_of(lines_info):
    return {k: getattr(lines_info, k) for k in ref.COUNTS}


def present_to_device(ctx, src, src_size, out_size, case, flags, dtype, m, vertices, n_lines=None):
    """One call into a fresh sentinel-filled device buffer: (image, info, counts); the guard bytes behind the image are checked here."""
    n = out_size[0] * out_size[1]
    px = 4 * np.dtype(dtype).itemsize
    out = device_bytes(n * px + GUARD)
    none, info, lines_info = ctx.present_split_lines(src.data_ptr(), src_size, out_size, *case, m, vertices, n_lines, flags=flags, out_device=out.data_ptr())
    assert none is None
    raw = out.cpu().numpy()
    assert (raw[n * px:] == SENTINEL).all(), "guard bytes behind out"
    return raw[:n * px].view(dtype).reshape(out_size[1], out_size[0], 4), info, counts_of(lines_info)


def check_bloomed(got, want, flags, what):
    if flags:
        assert (got[..., 3] == present_ref.ONE_F16).all(), what
        assert f16_ulps(got[..., :3].view(np.float16), want[..., :3].view(np.float16)).max() <= 2, what
    else:
        assert (got[..., 3] == 255).all(), what
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, what


@pytest.mark.parametrize("src_size,out_size", cases.SIZES)
def test_synthetic_frames_and_lists_equal_the_restatement(ctx, src_size, out_size):
    for n in cases.N_LINES:
        color, depth, vertices, m, parts, _ = cases.restated(src_size, out_size, n)
        src_bytes = frame_bytes(color, depth)
        src = to_device(src_bytes)
        on_device = to_device(vertices)
        for case in EXACT + [BLOOMED]:
            bloom = cases.bloom_of(parts) if case[0] > 0 else None
            for flags, dtype in KINDS:
                want = present_ref.composite(parts["S'"], bloom, *case, out_f16=bool(flags))
                what = f"{src_size[0]}x{src_size[1]} -> {out_size[0]}x{out_size[1]}, {n} lines, case {case}, {'f16' if flags else 'rgba8'}"
                got, info, counts = present_to_device(ctx, src, src_size, out_size, case, flags, dtype, m, on_device.data_ptr(), n)
                print(f"{what}: exact {float((got == want).all(axis=-1).mean()):.4f}, {counts}")
                assert counts == parts["counts"], what
                assert info.bloomed == int(case[0] > 0), what
                if case[0] == 0:
                    assert (got == want).all(), what
                else:
                    check_bloomed(got, want, flags, what)
                again, _, counts_again = present_to_device(ctx, src, src_size, out_size, case, flags, dtype, m, on_device.data_ptr(), n)
                assert (again == got).all() and counts_again == counts, "the same call twice: " + what
                from_host, _, counts_host = present_to_device(ctx, src, src_size, out_size, case, flags, dtype, m, vertices)
                assert (from_host == got).all() and counts_host == counts, "host vertices: " + what
                to_host, _, lines_info = ctx.present_split_lines(src.data_ptr(), src_size, out_size, *case, m, vertices, flags=flags)
                assert to_host.dtype == dtype and (to_host == got).all() and counts_of(lines_info) == counts, "host target: " + what
        assert (src.cpu().numpy() == src_bytes).all(), "src changed"
        assert (on_device.cpu().numpy() == vertices.view(np.uint8).reshape(-1)).all(), "vertices changed"


def test_no_lines_is_present_split_and_the_keys_do_not_leak(ctx):
    src_size, out_size = (32, 24), (64, 48)
    color, depth, vertices, m, parts, _ = cases.restated(src_size, out_size, 1000)
    src = to_device(frame_bytes(color, depth))
    for case in EXACT + [BLOOMED]:
        for flags, dtype in KINDS:
            plain, plain_info = ctx.present_split(src.data_ptr(), src_size, out_size, *case, flags=flags)
            for kw in ({"vertices": None}, {"vertices": vertices, "n_lines": 0}):
                got, info, lines_info = ctx.present_split_lines(src.data_ptr(), src_size, out_size, *case, m, flags=flags, **kw)
                assert (got == plain).all() and (info.levels, info.bloomed) == (plain_info.levels, plain_info.bloomed)
                assert counts_of(lines_info) == dict.fromkeys(ref.COUNTS, 0)
            # a NULL lines desc
            d = abi.PresentDesc()
            d.src_width, d.src_height, d.out_width, d.out_height = *src_size, *out_size
            d.bloom_intensity, d.tone_mapping, d.maximum_intensity, d.flags = *case, flags
            image, lines_info = np.zeros_like(plain), abi.LinesInfo()
            C.memset(C.byref(lines_info), 0xFF, C.sizeof(lines_info))
            ctx._check(ctx._lib.aic_present_split_lines(ctx._h, C.byref(d), None, C.c_void_p(src.data_ptr()), image.ctypes.data_as(C.c_void_p), 0, None, C.byref(lines_info)))
            assert (image == plain).all() and bytes(lines_info) == bytes(C.sizeof(lines_info))
    # lines drawn, then the plain call and a smaller list at the same size: nothing of the first call's keys or scene shows
    case = EXACT[0]
    with_lines, _, _ = ctx.present_split_lines(src.data_ptr(), src_size, out_size, *case, m, vertices)
    assert (with_lines == present_ref.composite(parts["S'"], None, *case)).all()
    plain, _ = ctx.present_split(src.data_ptr(), src_size, out_size, *case)
    assert (plain == present_ref.composite(parts["S"], None, *case)).all()
    assert (plain != with_lines).any()
    _, _, few, m_few, parts_few, _ = cases.restated(src_size, out_size, 28)
    got, _, lines_info = ctx.present_split_lines(src.data_ptr(), src_size, out_size, *case, m_few, few)
    assert (got == present_ref.composite(parts_few["S'"], None, *case)).all() and counts_of(lines_info) == parts_few["counts"]
    # ... nor after a call at another size in between (the key image is laid out anew)
    small = (17, 9)
    color_s, depth_s, vertices_s, m_s, parts_s, _ = cases.restated(small, small, 65)
    src_s = to_device(frame_bytes(color_s, depth_s))
    got, _, lines_info = ctx.present_split_lines(src_s.data_ptr(), small, small, *case, m_s, vertices_s)
    assert (got == present_ref.composite(parts_s["S'"], None, *case)).all() and counts_of(lines_info) == parts_s["counts"]
    got, _, lines_info = ctx.present_split_lines(src.data_ptr(), src_size, out_size, *case, m, vertices)
    assert (got == with_lines).all() and counts_of(lines_info) == parts["counts"]


def test_clearing_the_keys_in_every_call_gives_the_same_bits(monkeypatch):
    """AIC_LINES_CLEAR_KEYS=1, read when the context is made: the whole key image is cleared at the start of every call and the resolve leaves its keys
    where they are -- the scheme tools/present_lines_timing.py measures against the kept one. Images and counts are the restatement's all the same, call
    after call, at changing sizes."""
    monkeypatch.setenv("AIC_LINES_CLEAR_KEYS", "1")
    c = abi.Context(0)
    monkeypatch.delenv("AIC_LINES_CLEAR_KEYS")
    try:
        for src_size, out_size, n in (((64, 48), (64, 48), 1000), ((64, 48), (17, 9), 65), ((64, 48), (64, 48), 1000), ((32, 24), (64, 48), 28), ((257, 129), (257, 129), 1000)):
            color, depth, vertices, m, parts, _ = cases.restated(src_size, out_size, n)
            src = to_device(frame_bytes(color, depth))
            for flags, dtype in KINDS:
                for _ in range(2):
                    got, _, counts = present_to_device(c, src, src_size, out_size, EXACT[0], flags, dtype, m, vertices)
                    assert counts == parts["counts"]
                    assert (got == present_ref.composite(parts["S'"], None, *EXACT[0], out_f16=bool(flags))).all()
    finally:
        c.close()


def test_scratch_report():
    assert abi.present_lines_scratch((1920, 1080), (1920, 1080), 28) == 1920 * 1080 * 16 + 32 + 28 * 56
    assert abi.present_lines_scratch((960, 540), (1920, 1080), 0) == 0 and abi.present_lines_scratch((960, 540), (0, 1080), 28) == 0
    for bad in (((65536, 1), (4, 4), 1), ((4, 4), (65535, 32769), 1), ((0, 0), (4, 4), 1), ((4, 4), (4, 4), abi.LINES_MAX + 1)):
        with pytest.raises(abi.AicError):
            abi.present_lines_scratch(*bad)


def test_rejections_leave_the_context_usable(ctx):
    src_size, out_size = (32, 24), (64, 48)
    n_out = 64 * 48
    color, depth, vertices, m, parts, _ = cases.restated(src_size, out_size, 28)
    case = EXACT[1]
    want = present_ref.composite(parts["S'"], None, *case)
    src_bytes = frame_bytes(color, depth)
    src = to_device(src_bytes)
    on_device = to_device(np.concatenate([vertices.view(np.uint8).reshape(-1), np.zeros(8, np.uint8)]))
    out = device_bytes(n_out * 8 + GUARD)

    def good(what):
        got, _, counts = present_to_device(ctx, src, src_size, out_size, case, 0, np.uint8, m, on_device.data_ptr(), 28)
        assert (got == want).all() and counts == parts["counts"], what

    def call(src_ptr=None, out_ptr=None, src_size=src_size, out_size=out_size, i=case[0], tm=case[1], mi=case[2], flags=0, m=m, vertices=vertices, n_lines=None,
             line_flags=None):
        d, ld = abi.PresentDesc(), abi.LinesDesc()
        d.src_width, d.src_height, d.out_width, d.out_height = *src_size, *out_size
        d.bloom_intensity, d.tone_mapping, d.maximum_intensity, d.flags = i, tm, mi, flags
        ld.view_projection[:] = [float(v) for v in m]
        if isinstance(vertices, int) or vertices is None:
            ld.vertices, ld.flags = vertices, abi.LINES_DEVICE
        else:
            ld.vertices, ld.flags = vertices.ctypes.data, 0
        ld.n_lines = 28 if n_lines is None else n_lines
        if line_flags is not None:
            ld.flags = line_flags
        info, lines_info = abi.PresentInfo(), abi.LinesInfo()
        ctx._check(ctx._lib.aic_present_split_lines(ctx._h, C.byref(d), C.byref(ld), C.c_void_p(src.data_ptr() if src_ptr is None else src_ptr),
                                                    C.c_void_p(out.data_ptr() if out_ptr is None else out_ptr), 1, C.byref(info), C.byref(lines_info)))

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert (out.cpu().numpy() == SENTINEL).all(), what
        good(what)

    good("before")
    # what this call adds
    rejected(lambda: call(vertices=None), "NULL vertices with lines")
    rejected(lambda: call(n_lines=abi.LINES_MAX + 1), "too many lines")
    for off in (1, 2, 3):
        rejected(lambda: call(vertices=on_device.data_ptr() + off), f"device vertices at {off} bytes")
    for bad in (2, 3, 1 << 31):
        rejected(lambda: call(line_flags=bad), f"line flags {bad}")
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 7, 15):
            other = np.array(m)
            other[at] = bad
            rejected(lambda: call(m=other), f"view_projection[{at}] = {bad}")
    # aic_present_split's own
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
    rejected(lambda: call(src_ptr=0), "NULL src")
    rejected(lambda: call(out_ptr=0), "NULL out")
    wide_src = to_device(np.concatenate([src_bytes, np.zeros(16, np.uint8)]))
    rejected(lambda: call(src_ptr=wide_src.data_ptr() + 4), "src at 4 bytes")
    rejected(lambda: call(out_ptr=out.data_ptr() + 2), "RGBA8 out at 2 bytes")
    rejected(lambda: call(out_ptr=out.data_ptr() + 4, flags=abi.PRESENT_OUT_F16), "f16 out at 4 bytes")
    both = device_bytes(32 * 24 * 12 + n_out * 8)
    rejected(lambda: call(src_ptr=both.data_ptr(), out_ptr=both.data_ptr()), "out == src")
    rejected(lambda: call(src_ptr=both.data_ptr(), out_ptr=both.data_ptr() + 32 * 24 * 12 - 4), "out starts in src's depth plane")
    rejected(lambda: call(src_ptr=both.data_ptr() + n_out * 4 - 8, out_ptr=both.data_ptr()), "src starts inside out")
    assert (both.cpu().numpy() == SENTINEL).all()
    rejected(lambda: call(src_size=(65536, 1)), "src width above 65535")
    rejected(lambda: call(out_size=(1, 65536)), "out height above 65535")
    rejected(lambda: call(out_size=(65535, 32769)), "more than 2^31 output pixels")
    rejected(lambda: call(src_size=(0, 9)), "an empty src with a non-empty output")
    for bad in (float("nan"), -0.125, float("inf")):
        rejected(lambda: call(i=bad), f"bloom_intensity {bad}")
    for bad in (float("nan"), -1.0):
        rejected(lambda: call(mi=bad), f"maximum_intensity {bad}")
    rejected(lambda: call(tm=2), "tone_mapping 2")
    rejected(lambda: call(flags=2), "flags 2")
    # an empty output with lines: AIC_OK, nothing written
    call(out_size=(0, 48))
    assert (out.cpu().numpy() == SENTINEL).all() and (src.cpu().numpy() == src_bytes).all()
    good("after the empty output")


def view_projection_of(camera):
    """the host mirror's matrix: view then projection in f64, the sums in Mat4::then's order, rounded to f32; [c*4+r]"""
    v, p = camera.view_matrix().tolist(), camera.projection_matrix().tolist()
    return np.array([v[r][0] * p[0][c] + v[r][1] * p[1][c] + v[r][2] * p[2][c] + v[r][3] * p[3][c] for r in range(4) for c in range(4)], np.float64).astype(np.float32)


def test_the_cursor_through_the_host_mirror():
    """One opaque cube with the cursor on the face towards the camera: draw_split, then the presentation draws the cursor from the resident frame alone.
    The box's front edges show, its back edges are hidden by the cube itself; after the camera moves, the reprojected frame hides and shows them as its
    own depth plane says."""
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H
    from tests.test_gpu_reproject import split_bytes

    w, h = 40, 24
    n = w * h
    cams = H.StandardCameras()
    o = H.GraphicsOptions()
    o.bloom_intensity = 0.0
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(scenes.one_cube_space())
    eye = (0.7, 0.9, 2.5)
    cams.world_view_transform = H.look_at_y_up(eye, (0.5, 0.5, 0.5))
    cursor = H.Cursor()
    cursor.cube, cursor.face_entered, cursor.face_selected = (0, 0, 0), 6, 6  # PZ
    cursor.point_entered = (0.5, 0.5, 1.0)
    cursor.distance_to_point = float(np.linalg.norm(np.subtract(eye, cursor.point_entered)))
    lines = cursor.wireframe()
    assert lines.shape == (56, 7)
    r = H.HipRtRenderer(cams)
    r.update(cursor)
    first = r.draw_split()
    traced_with = r.world_camera()
    src_bytes = split_bytes(first)
    src = to_device(src_bytes)

    def check(resident, size, explicit):
        raw = resident.cpu().numpy()
        color, depth = raw[:n * 8].view(np.uint16).reshape(h, w, 4), raw[n * 8:n * 12].view(np.uint32).reshape(h, w)
        m = view_projection_of(r.world_camera())
        parts = {}
        want, counts = ref.present(color, depth, size, lines, m, 0.0, int(o.tone_mapping), o.maximum_intensity, parts=parts)
        shown, got_counts = r.present_split_lines(resident.data_ptr(), *size, lines if explicit else None)
        print(f"cursor at {size[0]}x{size[1]}: {got_counts}")
        assert got_counts == counts
        assert counts["n_pixels"] > 0 and counts["n_passed"] < counts["n_fragments"]
        assert (shown.width, shown.height) == size and (shown.data == want).all()
        plain = r.present_split(resident.data_ptr(), *size)
        assert (plain.data == present_ref.composite(parts["S"], None, 0.0, int(o.tone_mapping), o.maximum_intensity)).all()
        assert int((shown.data != plain.data).any(-1).sum()) > 0
        # the device form, f16
        out = device_bytes(size[0] * size[1] * 8 + GUARD)
        info, device_counts = r.present_split_lines(resident.data_ptr(), *size, None, abi.PRESENT_OUT_F16, out.data_ptr())
        raw_out = out.cpu().numpy()
        assert (raw_out[size[0] * size[1] * 8:] == SENTINEL).all() and device_counts == counts and info["bloomed"] == 0
        want16, _ = ref.present(color, depth, size, lines, m, 0.0, int(o.tone_mapping), o.maximum_intensity, out_f16=True, parts=parts)
        assert (raw_out[:size[0] * size[1] * 8].view(np.uint16).reshape(size[1], size[0], 4) == want16).all()
        assert (resident.cpu().numpy() == raw).all(), "the frame changed"

    check(src, (w, h), explicit=False)
    check(src, (2 * w, 2 * h), explicit=True)
    # without a cursor the overload draws nothing
    r.update()
    shown, counts = r.present_split_lines(src.data_ptr(), w, h)
    assert counts == dict.fromkeys(ref.COUNTS, 0) and (shown.data == r.present_split(src.data_ptr(), w, h).data).all()
    # the camera moves: the cursor is drawn over the reprojected frame, under the new camera
    cams.world_view_transform = H.look_at_y_up((0.9, 1.0, 2.3), (0.45, 0.5, 0.5))
    r.update(cursor)
    resident = device_bytes(n * 12)
    r.reproject_split(src.data_ptr(), resident.data_ptr(), traced_with)
    check(resident, (w, h), explicit=False)
    check(resident, (2 * w, 2 * h), explicit=False)
