"""AIC_FRAME_BLOOM on the MI355X: the bloom chain and composite of aic_bloom.hip against the NumPy restatement (tests/bloom_ref.py),
the flagged frame paths (aic_render, streamed, batched) against aic_probe_bloom of the same frame's ColorBuf, the rejected combinations,
and the host mirror's opt-in. tests/golden/png_bloom-0.25-all.npy is the reference's bloom-0.25-all.png decoded as
tests/golden/make_golden.py decodes the others (Image.open(...).convert("RGBA"), then np.save)."""
from pathlib import Path

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi
from tests import bloom_ref, scenes
from tests.test_gpu_parity import to_abi_options
from tests.test_oracle_light import image_diff, spawn_camera

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (128, 256), (1920, 1080), (3840, 2160)]


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def bloom_scene_camera():
    return spawn_camera((128, 256), (1.5, 3.0, 8.0), (0.0, 0.0, -1.0), fov=45.0)


def to_abi(opt, bloom):
    o = to_abi_options(opt)
    o.bloom_intensity = bloom
    return o


def setup_bloom_scene(ctx, bloom):
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, scenes.bloom_test_space())
    ctx.set_options(abi.LAYER_WORLD, to_abi(oracle.unaltered_colors(lighting=3), bloom))
    return np.ctypeslib.as_array(bloom_scene_camera().inverse_projection_view).copy()


def random_colorbuf(w, h, seed):
    rng = np.random.default_rng(seed)
    cb = np.zeros((h, w, 4), np.float32)
    t = np.where(rng.random((h, w)) < 0.7, 0.0, rng.random((h, w))).astype(np.float32)  # mostly opaque, some a < 1
    t[rng.random((h, w)) < 0.05] = 1.0  # a = 0
    cb[..., 3] = t
    light = rng.exponential(2.0, (h, w, 3)).astype(np.float32) * (1 - t)[..., None]
    light[rng.random((h, w)) < 0.01] *= 40000.0  # past 65504 after exposure
    cb[..., :3] = light
    return cb


def f16_ulps(a, b):
    ia = np.asarray(a, np.float16).view(np.int16).astype(np.int64)
    ib = np.asarray(b, np.float16).view(np.int16).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("size", SIZES)
def test_probe_matches_restatement(ctx, size):
    w, h = size
    cb = random_colorbuf(w, h, seed=w * 7919 + h)
    cases = [(1.0, 0, np.inf, 0.125), (2.5, 1, 1.0, 0.25), (0.75, 0, 2.0, 0.5), (1.0, 1, np.inf, 1.0)]
    if w * h > 1 << 20:
        cases = cases[:2]
    for exposure, tm, mi, i in cases:
        opt = abi.make_options(tone_mapping=tm, maximum_intensity=mi, bloom_intensity=i)
        got, mip0 = ctx.probe_bloom(cb, exposure, opt, want_mip0=True)
        want, b = bloom_ref.bloom_frame(cb, exposure, i, tm, mi)
        assert mip0.shape == b.shape
        ulps = f16_ulps(mip0, b)
        exact = float((ulps == 0).mean())
        print(f"{w}x{h} e {exposure} tm {tm} max {mi} i {i}: mip 0 exact {exact:.4f}, RGBA8 exact {float((got == want).all(axis=-1).mean()):.4f}")
        assert ulps.max() <= 2, (size, exposure, tm, mi, ulps.max())
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, (size, exposure, tm, mi)


def test_probe_bloom_scene_and_golden(ctx):
    """The bloom scene's ColorBuf: probe = restatement. Against the golden the scene is clamped to [0, 1] first. That the reference renderer
    which made bloom-0.25-all.png held its linear scene texture as Rgba8UnormSrgb (all-is-cubes-gpu frame_texture.rs:509-520, the format taken
    where the backend cannot render to Rgba16Float), so that its bloom saw the emissive green 100 as 1, is inferred from the images, not known:
    tests/test_bloom_cpu.py gives the evidence."""
    inv = setup_bloom_scene(ctx, 0.25)
    cb = ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_OUT_COLORBUF))["rgba8"]
    opt = to_abi(oracle.unaltered_colors(lighting=3), 0.25)
    got = ctx.probe_bloom(cb, 1.0, opt)
    want, _ = bloom_ref.bloom_frame(cb, 1.0, 0.25)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    clamped = cb.copy()
    clamped[..., :3] = np.minimum(clamped[..., :3], 1.0)
    assert image_diff(GOLDEN, "bloom-0.25-all", ctx.probe_bloom(clamped, 1.0, opt)).max() <= 12


def atrium(ctx):
    import bench

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    return (w, h), inv, vd


def test_probe_at_zero_intensity_equals_the_trace(ctx):
    inv = setup_bloom_scene(ctx, 0.0)
    frames = [(128, 256, inv, (0, 0, 0, 0))]
    for w, h, fi, bd in frames:
        cb = ctx.render(ctx.make_frame(w, h, world_inv=fi, backdrop=bd, flags=abi.FRAME_OUT_COLORBUF))["rgba8"]
        plain = ctx.render(ctx.make_frame(w, h, world_inv=fi, backdrop=bd))["rgba8"]
        assert (ctx.probe_bloom(cb, 1.0, to_abi(oracle.unaltered_colors(lighting=3), 0.0)) == plain).all()
    # a backdrop over a transparent sky (the UI layer alone: pixels with a < 1 and a = 0)
    ctx.clear_space(abi.LAYER_WORLD)
    ui = scenes.ui_space()
    ctx.upload_space(abi.LAYER_UI, ui)
    opt = oracle.make_options(fog=0, lighting=0)
    ctx.set_options(abi.LAYER_UI, to_abi(opt, 0.0))
    _, _, ui_inv = oracle.camera_matrices(90.0, 20.0, 96 / 64, (0, 0, 0, 1), (0.5, 0.5, 2.0))
    for bd in ((0, 0, 0, 0), (0.2, 0.1, 0.4, 0.6)):
        f = dict(ui_inv=ui_inv, backdrop=bd)
        cb = ctx.render(ctx.make_frame(96, 64, flags=abi.FRAME_OUT_COLORBUF, **f))["rgba8"]
        plain = ctx.render(ctx.make_frame(96, 64, **f))["rgba8"]
        assert (ctx.probe_bloom(cb, 1.0, abi.make_options(bloom_intensity=0.0)) == plain).all(), bd
    # 64 rows of the 1080p atrium frame: rows 508-571 of the whole frame's ColorBuf through the probe equal those rows of the frame
    (w, h), inv_a, vd = atrium(ctx)
    o = abi.make_options(fog=3, view_distance=vd, bloom_intensity=0.0)
    ctx.set_options(abi.LAYER_WORLD, o)
    cb = ctx.render(ctx.make_frame(w, h, world_inv=inv_a, flags=abi.FRAME_OUT_COLORBUF))["rgba8"]
    plain = ctx.render(ctx.make_frame(w, h, world_inv=inv_a))["rgba8"]
    assert (ctx.probe_bloom(cb[508:572], 1.0, o) == plain[508:572]).all()


def test_render_with_flag_blooms_the_bloom_scene(ctx):
    inv = setup_bloom_scene(ctx, 0.25)
    got = ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_BLOOM))
    assert not got["info"].flaws & abi.FLAW_NO_BLOOM
    cb = ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_OUT_COLORBUF))["rgba8"]
    probe = ctx.probe_bloom(cb, 1.0, to_abi(oracle.unaltered_colors(lighting=3), 0.25))
    assert (got["rgba8"] == probe).all()
    plain = ctx.render(ctx.make_frame(128, 256, world_inv=inv))
    assert plain["info"].flaws & abi.FLAW_NO_BLOOM
    assert (plain["rgba8"] != got["rgba8"]).any()
    # (the HDR scene against the golden made from a [0, 1] scene: see test_probe_bloom_scene_and_golden)
    want, _ = bloom_ref.bloom_frame(cb, 1.0, 0.25)
    assert np.abs(got["rgba8"].astype(int) - want.astype(int)).max() <= 1


def test_old_behaviour_holds(ctx):
    inv = setup_bloom_scene(ctx, 0.0)
    plain = ctx.render(ctx.make_frame(128, 256, world_inv=inv))
    flagged = ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_BLOOM))
    assert not plain["info"].flaws & abi.FLAW_NO_BLOOM and not flagged["info"].flaws & abi.FLAW_NO_BLOOM
    assert (plain["rgba8"] == flagged["rgba8"]).all()
    ref = oracle.render(oracle.Space(scenes.bloom_test_space()), oracle.unaltered_colors(lighting=3), bloom_scene_camera())
    assert (plain["rgba8"] == ref["rgba8"]).all()
    setup_bloom_scene(ctx, 0.25)
    again = ctx.render(ctx.make_frame(128, 256, world_inv=inv))
    assert again["info"].flaws & abi.FLAW_NO_BLOOM and (again["rgba8"] == plain["rgba8"]).all()


def test_streamed_and_batched_frames(ctx):
    import torch

    inv0 = setup_bloom_scene(ctx, 0.25)
    w, h = 128, 256
    cams = []
    for j in range(8):
        c = spawn_camera((w, h), (1.5 - 0.2 * j, 3.0 + 0.1 * j, 8.0 + 0.3 * j), (0.05 * j, -0.02 * j, -1.0), fov=45.0)
        cams.append(np.ctypeslib.as_array(c.inverse_projection_view).copy())
    frames = [ctx.make_frame(w, h, world_inv=c, exposure=1.0 + 0.25 * (j % 3), flags=abi.FRAME_BLOOM) for j, c in enumerate(cams)]
    want = [ctx.render(f)["rgba8"] for f in frames]
    bufs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(8)]
    torch.cuda.synchronize()
    for j in range(6):  # six frames in flight on six slots
        ctx.render_submit(frames[j], bufs[j].data_ptr(), j)
    for j in range(6):
        assert not ctx.render_wait(j).flaws & abi.FLAW_NO_BLOOM
    torch.cuda.synchronize()
    for j in range(6):
        assert (bufs[j].cpu().numpy() == want[j]).all(), f"streamed frame {j}"
    for k in (2, 4, 8):
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        ctx.render_submit_batch(frames[:k], [b.data_ptr() for b in bufs[:k]], 1)
        infos = ctx.render_wait_batch(1, k)
        torch.cuda.synchronize()
        for j in range(k):
            assert not infos[j].flaws & abi.FLAW_NO_BLOOM
            assert (bufs[j].cpu().numpy() == want[j]).all(), f"batch of {k}, frame {j}"
    # a copy on a foreign stream ordered behind the frame by aic_stream_wait_frame sees the composited frame
    side = torch.cuda.Stream()
    dst = torch.zeros_like(bufs[0])
    bufs[0].zero_()
    torch.cuda.synchronize()
    ctx.render_submit(frames[0], bufs[0].data_ptr(), 2)
    ctx.stream_wait_frame(2, side.cuda_stream)
    with torch.cuda.stream(side):
        dst.copy_(bufs[0])
    side.synchronize()
    ctx.render_wait(2)
    assert (dst.cpu().numpy() == want[0]).all()
    assert inv0 is not None


def test_rejected_combinations_leave_the_context_usable(ctx):
    inv = setup_bloom_scene(ctx, 0.25)
    good = ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_BLOOM))["rgba8"]
    bad = [
        (abi.FRAME_BLOOM | abi.FRAME_OUT_LINEAR, None, 1),
        (abi.FRAME_BLOOM | abi.FRAME_OUT_COLORBUF, None, 1),
        (abi.FRAME_BLOOM, (8, 2, 0), 5),
    ]
    for flags, part, code in bad:
        with pytest.raises(abi.AicError) as e:
            ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=flags, partition=part))
        assert e.value.code == code, (flags, part, str(e.value))
        assert (ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_BLOOM))["rgba8"] == good).all()
    with pytest.raises(abi.AicError) as e:
        ctx.trace_patches(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_BLOOM), [[-0.1, -0.1, 0.1, 0.1]])
    assert e.value.code == 5
    assert (ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_BLOOM))["rgba8"] == good).all()
    m = abi.MultiContext([0])
    try:
        m.upload_space(abi.LAYER_WORLD, scenes.bloom_test_space())
        m.set_options(abi.LAYER_WORLD, to_abi(oracle.unaltered_colors(lighting=3), 0.25))
        with pytest.raises(abi.AicError) as e:
            m.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_BLOOM))
        assert e.value.code == 5
    finally:
        m.close()
    assert (ctx.render(ctx.make_frame(128, 256, world_inv=inv, flags=abi.FRAME_BLOOM))["rgba8"] == good).all()


def test_host_mirror_opt_in(ctx):
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H

    w, h = 128, 256
    cams = H.StandardCameras()
    o = H.GraphicsOptions()  # GraphicsOptions::default(): bloom 0.125
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    cams.world_space = A.space_from_flat(scenes.bloom_test_space())
    eye = (1.5, 3.0, 8.0)
    cams.world_view_transform = H.look_at_y_up(eye, (1.5, 3.0, 7.0))
    r = H.HipRtRenderer(cams)
    # the mirror draws with exactly the ABI frame's camera, so that the two frames can be required to be equal
    _, _, inv = oracle.camera_matrices(90.0, 200.0, w / h, oracle.look_at_y_up(eye, (1.5, 3.0, 7.0)), eye)
    r.set_world_camera_override([float(v) for v in np.asarray(inv, np.float64).reshape(16)], 1.0)
    assert r.bloom is False
    r.update()
    plain = r.draw_rgba("")
    assert plain.flaws & H.Flaws.NO_BLOOM == H.Flaws.NO_BLOOM
    r.set_bloom(True)
    bloomed = r.draw_rgba("")
    assert bloomed.flaws & H.Flaws.NO_BLOOM != H.Flaws.NO_BLOOM
    assert (bloomed.data != plain.data).any()
    # the same frames through the ABI: default options, the same camera
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, scenes.bloom_test_space())
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    abi_plain = ctx.render(ctx.make_frame(w, h, world_inv=inv))["rgba8"]
    abi_bloom = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_BLOOM))["rgba8"]
    assert (plain.data == abi_plain).all()
    assert (bloomed.data == abi_bloom).all()
    r.set_bloom(False)
    again = r.draw_rgba("")
    assert (again.data == plain.data).all() and again.flaws == plain.flaws


def test_full_1080p_frame(ctx):
    (w, h), inv, vd = atrium(ctx)
    o = abi.make_options(fog=3, view_distance=vd)  # GraphicsOptions::default(): bloom 0.125
    ctx.set_options(abi.LAYER_WORLD, o)
    got = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_BLOOM))
    assert not got["info"].flaws & abi.FLAW_NO_BLOOM
    cb = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_COLORBUF))["rgba8"]
    assert (got["rgba8"] == ctx.probe_bloom(cb, 1.0, o)).all()
