"""The trace kernel's colour against the CPU oracle bit for bit (run with -m gpu on an MI355X).

The kernel is built with -ffp-contract=off, does its colour arithmetic in f32 in the reference's order and restates the C
library's powf / expf (aic_colour.h powf_table, expf_table), as the oracle calls them. So the linear Rgba the frame hands
over before exposure and tone mapping (AIC_FRAME_OUT_LINEAR, Rgba::from(ColorBuf): raytracer_components.rs:141-163) must
carry the oracle's exact bits, and the encoded RGBA8 must equal the oracle's with no tolerance. A +-1 level bar lets relative
errors of up to about 1 % through; these tests do not. Every option of the colour path (fog, transparency, lighting, Bounce,
antialiasing, post-processing) goes through every kernel variant, and every other way a frame is traced (layers, partitions,
patches, batches, streamed slots, the BIG kernels, full-size frames) is compared with the single-frame image path."""
import os

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi, flat
from all_is_cubes_amd import workloads
from tests import scenes
from tests.test_gpu_parity import to_abi_options

pytestmark = pytest.mark.gpu

VARIANTS = (("recording", abi.VARIANT_RECORDING), ("plain", abi.VARIANT_PLAIN), ("exchanging", abi.VARIANT_EXCHANGING))
EYE = (10.5, 12.0, 24.0)
VD = 20.0  # short enough that the fog term (sr.rs:745-768) spans its whole range over the scene: see test_the_fog_term_covers_its_range
SIZE = (96, 64)


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def colour_space():
    """A small scene with every source of colour: voxel blocks (an emissive palette entry, translucent blocks), translucent and
    emissive atoms among the floating cubes (emission past 1, for the tone mappers), an octant sky and an interpolated light field."""
    sp = workloads.synthetic_space(n=20, resolution=8, n_blocks=8, seed=5, light="field")
    sp.set_sky_octants(np.random.default_rng(3).uniform(0.1, 1.4, (8, 3)))
    glow = [sp.add_block(flat.atom(rgba, emission=em)) for rgba, em in (
        ((0.9, 0.4, 0.1, 0.3), (0.6, 0.2, 0.0)), ((0.2, 0.3, 0.8, 1.0), (0.0, 0.5, 2.5)), ((0.7, 0.7, 0.7, 0.05), (0.0, 0.0, 0.0)),
        ((0.1, 0.9, 0.3, 0.6), (1.5, 1.5, 0.3)))]
    rng = np.random.default_rng(9)
    for _ in range(60):
        x, z = (int(v) for v in rng.integers(2, 18, 2))
        y = int(rng.integers(5, 14))
        sp.set((x, y, z), glow[int(rng.integers(0, len(glow)))])
    return sp


@pytest.fixture(scope="module")
def space():
    return colour_space()


def camera(size=SIZE, eye=EYE, target=(10.0, 4.0, 4.0), view_distance=VD, fov=90.0):
    w, h = size
    _, _, inv = oracle.camera_matrices(fov, view_distance, w / h, oracle.look_at_y_up(eye, target), eye)
    return inv


def assert_bits(got, want, what):
    """Float images equal bit for bit (+0.0 and -0.0 differ, so do NaN payloads)."""
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1))
    if len(bad):
        p = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ in their linear bits; first at {p}: "
                             f"got {got[p].tolist()} want {want[p].tolist()}")


def assert_rgba8_exact(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    if len(bad):
        p = tuple(bad[0])
        d = np.abs(got.astype(np.int16) - want.astype(np.int16)).max()
        raise AssertionError(f"{what}: {len(bad)} pixels differ in RGBA8 (max {d}); first at {p}: got {got[p].tolist()} want {want[p].tolist()}")


def colorbuf_to_rgba(cb):
    """Rgba::from(ColorBuf) (raytracer_components.rs:141-163) on the host, as tests/test_gpu_parity.py test_float_outputs does."""
    t = cb[..., 3]
    alpha = np.float32(1.0) - t
    with np.errstate(divide="ignore", invalid="ignore"):
        rgb = cb[..., 0:3] / alpha[..., None]
    rgb = np.where(rgb > 0, rgb, np.float32(0.0))
    back = np.concatenate([rgb, alpha[..., None]], -1).astype(np.float32)
    back[t >= 1.0] = 0.0
    return back


def check_all_variants(ctx, w, h, inv, ref, what, colorbuf=False, **frame_kw):
    """Linear bits and RGBA8 of the three kernel variants against the oracle's; Bounce has no exchanging variant (it runs the plain one)."""
    for name, variant in VARIANTS:
        tune = abi.tuning(variant=variant)
        lin = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_LINEAR, tuning=tune, **frame_kw), want_aux=variant == abi.VARIANT_RECORDING)
        assert lin["info"].variant == variant or (variant == abi.VARIANT_EXCHANGING and lin["info"].variant == abi.VARIANT_PLAIN), (what, name, lin["info"].variant)
        assert_bits(lin["rgba8"], ref["linear"], f"{what}, {name} variant")
        img = ctx.render(ctx.make_frame(w, h, world_inv=inv, tuning=tune, **frame_kw))
        assert_rgba8_exact(img["rgba8"], ref["rgba8"], f"{what}, {name} variant")
        if colorbuf:
            cb = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_COLORBUF, tuning=tune, **frame_kw))
            assert_bits(colorbuf_to_rgba(cb["rgba8"]), ref["linear"], f"{what}, {name} variant, ColorBuf")


def render_case(ctx, sp, opt, size=SIZE, inv=None, colorbuf=False, what=""):
    w, h = size
    inv = camera(size, view_distance=opt.view_distance) if inv is None else inv
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    ref = oracle.render(oracle.Space(sp), opt, oracle.make_camera(inv, w, h), want_linear=True)
    check_all_variants(ctx, w, h, inv, ref, what, colorbuf=colorbuf)
    return ref


# --- the options matrix: fog x transparency x lighting x antialiasing, every kernel variant ---------------------------------
# transparency 2 = Threshold, at three thresholds; under VD the fog term is evaluated over its whole range and clamped behind it
@pytest.mark.parametrize("transparency,threshold", [(0, 0.5), (1, 0.5), (2, 0.1), (2, 0.5), (2, 0.9)])
@pytest.mark.parametrize("fog", [0, 1, 2, 3])
def test_options_matrix_linear_bits(ctx, space, fog, transparency, threshold):
    for lighting in range(5):
        for aa in (0, 2):
            opt = oracle.make_options(fog=fog, transparency=transparency, threshold=threshold, lighting=lighting, antialiasing=aa, view_distance=VD)
            render_case(ctx, space, opt, colorbuf=(lighting in (1, 3) and transparency != 2),
                        what=f"fog {fog} transparency {transparency}@{threshold} lighting {lighting} aa {aa}")


@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("fog", [0, 2, 3])
def test_bounce_linear_bits(ctx, space, fog, samples):
    for transparency in (0, 1):
        for aa in (0, 2):
            opt = oracle.make_options(fog=fog, transparency=transparency, lighting=5, bounce_samples=samples, antialiasing=aa, view_distance=VD)
            render_case(ctx, space, opt, colorbuf=aa == 2, what=f"Bounce {samples} fog {fog} transparency {transparency} aa {aa}")


def test_the_fog_term_covers_its_range(space):
    """(the matrix above is only as strong as its scene) Sky and surfaces near and far: a ray's t runs in units of its direction,
    which spans the view distance, so first hits from t < 0.25 to t > 1 feed the fog term rel from below 0.25 to its clamp at 1."""
    opt = oracle.make_options(fog=3, view_distance=VD)
    w, h = SIZE
    ref = oracle.render(oracle.Space(space), opt, oracle.make_camera(camera(), w, h), want_aux=True)
    hit = ref["aux"]["hit"] == 1
    t = ref["aux"]["t_distance"][hit]
    assert hit.mean() > 0.5 and (~hit).any()
    assert t.min() < 0.25 and t.max() > 1.0


# --- post-processing: exposure and tone mapping come after the linear output, so RGBA8 is their only view ----------------
@pytest.mark.parametrize("tone_mapping", [0, 1])
@pytest.mark.parametrize("maximum_intensity", [np.inf, 1.0, 2.5])
def test_exposure_and_tone_mapping_rgba8_exact(ctx, space, tone_mapping, maximum_intensity):
    w, h = SIZE
    inv = camera()
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, space)
    for fog, lighting in ((3, 3), (0, 1)):
        opt = oracle.make_options(fog=fog, lighting=lighting, tone_mapping=tone_mapping, maximum_intensity=float(maximum_intensity), view_distance=VD)
        ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
        lin = None
        for exposure in (0.5, 1.0, 2.0):
            opt.exposure = exposure  # (Camera::exposure: the device takes it from the frame)
            ref = oracle.render(oracle.Space(space), opt, oracle.make_camera(inv, w, h), want_linear=True)
            if lin is None:
                lin = ref["linear"]
                assert float(lin[..., 0:3].max()) > 1.2  # values the clamp and Reinhard act on
            for name, variant in VARIANTS[1:]:
                img = ctx.render(ctx.make_frame(w, h, world_inv=inv, exposure=exposure, tuning=abi.tuning(variant=variant)))
                assert_rgba8_exact(img["rgba8"], ref["rgba8"], f"exposure {exposure} tone {tone_mapping} max {maximum_intensity} fog {fog} lighting {lighting}, {name}")


@pytest.mark.parametrize("workload", ["atrium"])
def test_full_size_post_processing_rgba8_exact(ctx, workload):
    """The same at full size: a last-bit deviation of the tone mapper (say, luminance summed in another order) changes the
    post-processed value of about one pixel in ten, and at 1080p some of those land across an sRGB8 threshold. The whole
    frame, linear bits and RGBA8 alike, under every exposure and both tone mappers."""
    import bench

    sp, (w, h), eye, target, vd, _ = bench.build_workload(workload)
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    osp, cam = oracle.Space(sp), oracle.make_camera(inv, w, h)
    threads = min(16, os.cpu_count() or 4)
    for tone_mapping, maximum_intensity in ((1, 1.0), (1, 2.5), (0, 1.0)):
        opt = oracle.make_options(fog=3, view_distance=vd, tone_mapping=tone_mapping, maximum_intensity=maximum_intensity)
        ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
        for exposure in (0.5, 1.0, 2.0):
            opt.exposure = exposure
            ref = oracle.render(osp, opt, cam, want_linear=exposure == 1.0, threads=threads)
            if exposure == 1.0:
                assert_bits(ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_LINEAR))["rgba8"], ref["linear"], f"{workload} linear")
            img = ctx.render(ctx.make_frame(w, h, world_inv=inv, exposure=exposure))
            assert_rgba8_exact(img["rgba8"], ref["rgba8"], f"{workload} exposure {exposure} tone {tone_mapping} max {maximum_intensity}")


@pytest.mark.parametrize("transparency", [1, 2])
@pytest.mark.parametrize("fog", [0, 3])
def test_debug_pixel_cost_linear_bits(ctx, space, fog, transparency):
    """debug_pixel_cost (accum.rs:228-234): the pixel is rgb(0.02 n, 0.002 n, luminance(colour) * 0.2), so the linear output shows
    the step count and the luminance of the accumulated colour unrounded."""
    for aa in (0, 2):
        opt = oracle.make_options(fog=fog, transparency=transparency, threshold=0.5, lighting=3, antialiasing=aa, debug_pixel_cost=True, view_distance=VD)
        ref = render_case(ctx, space, opt, what=f"debug_pixel_cost fog {fog} transparency {transparency} aa {aa}")
        assert len(np.unique(ref["linear"][..., 2])) > 100


# --- other ray paths against the single-frame image path -------------------------------------------------------------------
def test_ui_layer_and_backdrop_linear_bits(ctx, space):
    w, h = SIZE
    ui = scenes.ui_space()
    for opt in (oracle.make_options(fog=2, lighting=3, view_distance=VD), oracle.make_options(fog=3, transparency=2, threshold=0.3, lighting=1, antialiasing=2, view_distance=VD)):
        inv = camera(view_distance=opt.view_distance)
        _, _, ui_inv = oracle.camera_matrices(90.0, opt.view_distance, w / h, (0, 0, 0, 1), (0.5, 0.5, 2.0))
        backdrop = (0.2, 0.4, 0.6, 0.5)
        ctx.upload_space(abi.LAYER_WORLD, space)
        ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
        ctx.upload_space(abi.LAYER_UI, ui)
        ctx.set_options(abi.LAYER_UI, to_abi_options(opt))
        ref = oracle.render(oracle.Space(space), opt, oracle.make_camera(inv, w, h), ui=oracle.Space(ui), ui_opt=opt, ui_cam=oracle.make_camera(ui_inv, w, h),
                            backdrop=backdrop, want_linear=True)
        check_all_variants(ctx, w, h, inv, ref, f"UI layer + backdrop, fog {opt.fog}", colorbuf=True, ui_inv=ui_inv, backdrop=backdrop)
        # and a world with the backdrop alone (renderer.rs:474-477: the backdrop shows where the world is transparent)
        ctx.clear_space(abi.LAYER_UI)
        ref = oracle.render(oracle.Space(space), opt, oracle.make_camera(inv, w, h), backdrop=backdrop, want_linear=True)
        check_all_variants(ctx, w, h, inv, ref, f"backdrop, fog {opt.fog}", backdrop=backdrop)
    ctx.clear_space(abi.LAYER_UI)


@pytest.mark.parametrize("aa", [0, 2])
def test_row_partition_and_patches_linear_bits(ctx, space, aa):
    """ray_mode 1 (a strip partition) and ray_mode 2 (trace_patches) hand over the full frame's linear bits."""
    w, h = 100, 70
    opt = oracle.make_options(fog=2, transparency=1, lighting=4, antialiasing=aa, view_distance=VD)
    inv = camera((w, h))
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, space)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    backdrop = (0.2, 0.1, 0.3, 0.4)
    ref = oracle.render(oracle.Space(space), opt, oracle.make_camera(inv, w, h), backdrop=backdrop, want_linear=True)
    full = ctx.render(ctx.make_frame(w, h, world_inv=inv, backdrop=backdrop, flags=abi.FRAME_OUT_LINEAR))["rgba8"]
    assert_bits(full, ref["linear"], "full frame")
    strip, n = 16, 3
    for part in range(n):
        for name, variant in VARIANTS[1:]:
            got = ctx.render(ctx.make_frame(w, h, world_inv=inv, backdrop=backdrop, partition=(strip, n, part), flags=abi.FRAME_OUT_LINEAR,
                                            tuning=abi.tuning(variant=variant)))["rgba8"]
            rows = [y for y in range(h) if (y // strip) % n == part]
            assert_bits(got, full[rows], f"partition part {part}, {name}")
    # trace_patches: every pixel's rectangle (renderer.rs:537-550), scrambled, in two batches
    ex = np.arange(w + 1, dtype=np.float64) / np.float64(w) * 2.0 - 1.0
    ey = -(np.arange(h + 1, dtype=np.float64) / np.float64(h) * 2.0 - 1.0)
    X, Y = np.meshgrid(np.arange(w), np.arange(h))
    rects = np.stack([ex[X], ey[Y], ex[X + 1], ey[Y + 1]], -1).reshape(-1, 4)
    order = np.random.default_rng(2).permutation(len(rects))
    fr = ctx.make_frame(w, h, world_inv=inv, backdrop=backdrop, flags=abi.FRAME_OUT_LINEAR)
    got = np.zeros((len(rects), 4), np.float32)
    for part in (order[: len(order) // 3], order[len(order) // 3:]):
        got[part] = ctx.trace_patches(fr, rects[part])["rgba8"]
    assert_bits(got.reshape(h, w, 4), full, "trace_patches")
    enc = ctx.render(ctx.make_frame(w, h, world_inv=inv, backdrop=backdrop))["rgba8"]
    assert_rgba8_exact(enc, ref["rgba8"], "encoded full frame")


@pytest.mark.parametrize("flags", [abi.FRAME_OUT_LINEAR, 0])
def test_batched_and_streamed_frames_linear_bits(ctx, space, flags):
    """aic_render_submit_batch at k = 8 and streamed aic_render_submit / aic_render_wait deliver each frame's own linear bits (and,
    without the float flag, its own RGBA8 bytes), for both production variants, antialiased and not."""
    import torch

    w, h, k = 160, 96, 8
    ui = scenes.ui_space()
    cams = []
    for j in range(k):
        eye = (EYE[0] + 0.9 * j, EYE[1] - 0.6 * j, EYE[2] - 0.8 * j)
        inv = camera((w, h), eye=eye, view_distance=VD)
        _, _, ui_inv = oracle.camera_matrices(90.0, VD, w / h, (0, 0, 0, 1), (0.5 + 0.1 * j, 0.5, 2.0))
        cams.append((inv, ui_inv, (0.2, 0.1 * j, 0.4, 0.6) if j % 3 == 1 else (0, 0, 0, 0)))
    floats = bool(flags & abi.FRAME_OUT_LINEAR)
    dtype = torch.float32 if floats else torch.uint8
    for aa, with_ui in ((0, False), (2, True)):
        opt = oracle.make_options(fog=3, transparency=1, lighting=3, antialiasing=aa, view_distance=VD)
        ctx.upload_space(abi.LAYER_WORLD, space)
        ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
        if with_ui:
            ctx.upload_space(abi.LAYER_UI, ui)
            ctx.set_options(abi.LAYER_UI, to_abi_options(opt))
        else:
            ctx.clear_space(abi.LAYER_UI)
        refs = []
        for inv, ui_inv, bd in cams[:2]:  # (the first two against the oracle; all eight against the single-frame path)
            refs.append(oracle.render(oracle.Space(space), opt, oracle.make_camera(inv, w, h), ui=oracle.Space(ui) if with_ui else None,
                                      ui_opt=opt if with_ui else None, ui_cam=oracle.make_camera(ui_inv, w, h) if with_ui else None, backdrop=bd,
                                      want_linear=True))
        for name, variant in VARIANTS[1:]:
            frames = [ctx.make_frame(w, h, world_inv=c[0], ui_inv=c[1] if with_ui else None, backdrop=c[2], flags=flags, tuning=abi.tuning(variant=variant)) for c in cams]
            want = [ctx.render(f)["rgba8"] for f in frames]
            for j, r in enumerate(refs):
                if floats:
                    assert_bits(want[j], r["linear"], f"single frame {j}, aa {aa}, {name}")
                else:
                    assert_rgba8_exact(want[j], r["rgba8"], f"single frame {j}, aa {aa}, {name}")
            bufs = [torch.zeros((h, w, 4), dtype=dtype, device="cuda") for _ in range(k)]
            torch.cuda.synchronize()
            ctx.render_submit_batch(frames, [b.data_ptr() for b in bufs], 1)
            ctx.render_wait_batch(1, k)
            torch.cuda.synchronize()
            for j in range(k):
                got = bufs[j].cpu().numpy()
                if floats:
                    assert_bits(got, want[j], f"batch frame {j}, aa {aa}, {name}")
                else:
                    assert_rgba8_exact(got, want[j], f"batch frame {j}, aa {aa}, {name}")
            for b in bufs:
                b.zero_()
            torch.cuda.synchronize()
            for j in range(4):  # four frames in flight on four slots
                ctx.render_submit(frames[j], bufs[j].data_ptr(), j)
            for j in range(4):
                ctx.render_wait(j)
            torch.cuda.synchronize()
            for j in range(4):
                got = bufs[j].cpu().numpy()
                if floats:
                    assert_bits(got, want[j], f"streamed frame {j}, aa {aa}, {name}")
                else:
                    assert_rgba8_exact(got, want[j], f"streamed frame {j}, aa {aa}, {name}")
    ctx.clear_space(abi.LAYER_UI)


# --- the BIG kernels: a block table past 16384 entries (untagged cube grid, classes from the LDS table) ----------------------
def test_big_block_table_linear_bits(ctx):
    rng = np.random.default_rng(31)
    sp = flat.FlatSpace((0, 0, 0), (12, 10, 12))
    sp.set_sky_octants(np.random.default_rng(4).uniform(0.1, 1.2, (8, 3)))
    sp.add_block(flat.air())
    sp.add_block(flat.atom((0.5, 0.6, 0.9, 0.35), emission=(0.4, 0.1, 0.0)))
    [sp.add_block(b) for b in workloads.synthetic_blocks(8, 6, seed=5)]
    while len(sp.blocks) < 16385:  # one past the 14-bit limit
        c = rng.uniform(0.05, 0.95, 3)
        i = len(sp.blocks)
        sp.add_block(flat.atom((float(c[0]), float(c[1]), float(c[2]), 1.0 if i % 5 else 0.5)))
    grid = rng.integers(1, len(sp.blocks), sp.size).astype(np.uint16)
    grid[rng.random(sp.size) < 0.75] = 0
    grid[:, 0, :] = rng.integers(1, len(sp.blocks), (12, 12))
    grid[rng.random(sp.size) < 0.05] = rng.integers(1, 8)
    sp.block_index[...] = grid
    sp.light[..., 0:3] = rng.integers(40, 256, sp.size + (3,))
    sp.light[..., 3] = 255
    w, h = 112, 80
    eye = (6.0, 8.5, 17.0)
    inv = camera((w, h), eye=eye, target=(6, 2, 6), view_distance=30.0)
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    for transparency, lighting, fog in ((1, 3, 2), (1, 0, 3), (1, 1, 2), (0, 3, 3), (2, 0, 2), (0, 1, 3)):
        opt = oracle.make_options(fog=fog, transparency=transparency, lighting=lighting, view_distance=30.0)
        ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
        ref = oracle.render(oracle.Space(sp), opt, oracle.make_camera(inv, w, h), want_linear=True)
        check_all_variants(ctx, w, h, inv, ref, f"BIG <transparency {transparency}, lighting {lighting}> fog {fog}")


# --- full size: the benchmark scenes under Compromise and Physical fog, the auto-selected (exchanging) variant ---------------------------
@pytest.mark.parametrize("fog", [2, 3])
@pytest.mark.parametrize("workload", ["atrium", "s256"])
def test_full_size_linear_rows(ctx, workload, fog):
    import bench

    sp, (w, h), eye, target, vd, _ = bench.build_workload(workload)
    opt = oracle.make_options(fog=fog, view_distance=vd)
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))
    lin = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_LINEAR))
    assert lin["info"].variant == abi.VARIANT_EXCHANGING
    img = ctx.render(ctx.make_frame(w, h, world_inv=inv))
    assert img["info"].variant == abi.VARIANT_EXCHANGING
    osp, cam = oracle.Space(sp), oracle.make_camera(inv, w, h)
    for y in sorted({int(round(k * (h - 1) / 15.0)) for k in range(16)}):
        ref = oracle.render(osp, opt, cam, rows=(y, y + 1), want_linear=True, threads=min(16, os.cpu_count() or 4))
        assert_bits(lin["rgba8"][y:y + 1], ref["linear"][y:y + 1], f"{workload} fog {fog} row {y}")
        assert_rgba8_exact(img["rgba8"][y:y + 1], ref["rgba8"][y:y + 1], f"{workload} fog {fog} row {y}")


# --- the device's expf against the C library's, over everything the fog term can feed it -------------------------------------
def test_device_expf_equals_libm_expf_on_the_fog_domain(ctx):
    """distance_fog (sr.rs:745-768) takes exp(-1.6 * rel) with rel clamped to [0, 1]: every f32 in [-1.6, 0] (-0.0 included, about
    1.07e9 values), in chunks, against the oracle's std::exp(float) -- the C library's expf -- bit for bit."""
    lo = int(np.float32(-0.0).view(np.uint32))
    hi = int(np.float32(-1.6).view(np.uint32))
    chunk = 1 << 26
    n = 0
    for start in range(lo, hi + 1, chunk):
        x = np.arange(start, min(start + chunk, hi + 1), dtype=np.uint32).view(np.float32)
        got = ctx.probe_expf(x)
        want = oracle.expf(x)
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert len(bad) == 0, f"{len(bad)} of {len(x)} differ, e.g. x={x[bad[:3]].tolist()} got={got[bad[:3]].tolist()} want={want[bad[:3]].tolist()}"
        n += len(x)
    assert n == hi - lo + 1 and x[-1] == np.float32(-1.6)
    # the probe refuses what expf_table cannot evaluate (it has no overflow / underflow handling)
    for bad_x in (88.0, -88.0, np.inf, np.nan):
        with pytest.raises(abi.AicError):
            ctx.probe_expf(np.array([0.5, bad_x], np.float32))
