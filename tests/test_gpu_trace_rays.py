"""aic_trace_rays against the CPU oracle's trace_ray, ray by ray (run with -m gpu on an MI355X).

The call is SpaceRaytracer::trace_ray (sr.rs:113-120) for a batch of world-space rays against one layer's space: no camera, no
layering. The tolerance is the project's own for colour: float outputs carry the oracle's bits, RGBA8 has no tolerance, step
counts and first-hit records are equal, t_distance is equal as f64 bits."""
import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi, flat, workloads
from tests import scenes
from tests.test_gpu_linear_parity import VD, camera, colour_space
from tests.test_gpu_parity import to_abi_options

pytestmark = pytest.mark.gpu

PLAIN, EXCHANGING = abi.tuning(variant=abi.VARIANT_PLAIN), abi.tuning(variant=abi.VARIANT_EXCHANGING)
AUX_FIELDS = ("hit", "cube", "voxel", "resolution", "face", "block_index", "cubes_traced", "layer")


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def space():
    return colour_space()


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_bits(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.nonzero((bits32(got) != bits32(want)).any(axis=-1))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} rays differ in their float bits; first is ray {i}: got {got[i].tolist()} want {want[i].tolist()}")


def make_rays(n=4000, seed=77):
    """Origins uniform in [-6, 26)^3 around the 20^3 space; half the directions aimed at a uniform point inside it, half Gaussian; lengths
    times one of {1e-3, 1, 40}; a tenth with x = 0, a twentieth along x only."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-6.0, 26.0, (n, 3))
    aimed = rng.uniform(0.0, 20.0, (n, 3)) - o
    gauss = rng.normal(size=(n, 3))
    d = np.where((rng.random(n) < 0.5)[:, None], aimed, gauss)
    d = d * rng.choice([1e-3, 1.0, 40.0], n)[:, None]
    kind = rng.random(n)
    d[kind < 0.10, 0] = 0.0
    along_x = (kind >= 0.10) & (kind < 0.15)
    d[along_x, 1:] = 0.0
    return np.ascontiguousarray(np.concatenate([o, d], 1))


def oracle_rays(osp, opt, rays, sky):
    """(ColorBuf [n,4] f32, steps [n] u64, DepthBuf depth [n] f64) of oracle.trace_ray, ray by ray; sky[i] = include_sky of ray i."""
    n = len(rays)
    cb, steps, depth = np.zeros((n, 4), np.float32), np.zeros(n, np.uint64), np.zeros(n, np.float64)
    for i in range(n):
        steps[i], cb[i], depth[i] = oracle.trace_ray(osp, opt, rays[i, 0:3], rays[i, 3:6], include_sky=bool(sky[i]))
    return cb, steps, depth


def device_rays(ctx, layer, rays, sky, flags=abi.FRAME_OUT_COLORBUF, want_aux=False, exposure=1.0):
    """The batch in two calls -- the rays traced with the sky, then those without -- merged back into ray order: (out, aux, steps total, variants seen)."""
    floats = bool(flags & (abi.FRAME_OUT_LINEAR | abi.FRAME_OUT_COLORBUF))
    out = np.zeros((len(rays), 4), np.float32 if floats else np.uint8)
    aux = np.zeros(len(rays), abi.PIXEL_AUX_DTYPE) if want_aux else None
    total, variants = 0, set()
    for include_sky in (True, False):
        sel = np.nonzero(sky == include_sky)[0]
        if not len(sel):
            continue
        r = ctx.trace_rays(layer, rays[sel], include_sky=include_sky, flags=flags, exposure=exposure, want_aux=want_aux)
        assert r["info"].rows_rendered == len(sel)
        out[sel] = r["rgba8"]
        if want_aux:
            aux[sel] = r["aux"]
        total += r["info"].cubes_traced
        variants.add(r["info"].variant)
    return out, aux, total, variants


def check_against_oracle(ctx, layer, osp, opt, rays, sky, what, ref=None):
    """Every variant the batch can be asked for against the oracle: ColorBuf bits, steps per ray (the recording variant's records) and in total,
    aux.hit / aux.t_distance against the DepthBuf depth (inf <=> no hit)."""
    cb, steps, depth = oracle_rays(osp, opt, rays, sky) if ref is None else ref
    got, aux, total, variants = device_rays(ctx, layer, rays, sky, want_aux=True)
    assert variants == {abi.VARIANT_RECORDING}, (what, variants)
    assert_bits(got, cb, f"{what}, recording variant")
    assert (aux["cubes_traced"] == steps).all(), (what, np.nonzero(aux["cubes_traced"] != steps)[0][:5], aux["cubes_traced"][:8], steps[:8])
    assert total == int(steps.sum()), (what, total, int(steps.sum()))
    hit = np.isfinite(depth)
    assert ((aux["hit"] == 1) == hit).all(), (what, np.nonzero((aux["hit"] == 1) != hit)[0][:5])
    assert (bits64(aux["t_distance"][hit]) == bits64(depth[hit])).all(), what
    assert (aux["layer"][hit] == layer).all(), what
    for name, tune, allowed in (("plain", PLAIN, {abi.VARIANT_PLAIN}), ("exchanging", EXCHANGING, {abi.VARIANT_EXCHANGING, abi.VARIANT_PLAIN})):
        got, _, total, variants = device_rays(ctx, layer, rays, sky, flags=abi.FRAME_OUT_COLORBUF | tune)
        assert variants <= allowed, (what, name, variants)  # (Bounce lighting has no exchanging variant)
        assert_bits(got, cb, f"{what}, {name} variant")
        assert total == int(steps.sum()), (what, name, total, int(steps.sum()))
    return cb, steps, depth


def setup_world(ctx, sp, opt):
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt))


# --- 1. the oracle, ray by ray ------------------------------------------------------------------------------------------------
def test_the_ray_recipe_exercises_hits_and_misses(space):
    """A condition on the inputs, not on the device: at least a third of the rays hit something and at least a tenth end at transmittance 1."""
    rays = make_rays()
    sky = np.arange(len(rays)) % 2 == 0
    cb, steps, depth = oracle_rays(oracle.Space(space), oracle.make_options(fog=0, view_distance=VD), rays, sky)
    assert np.isfinite(depth).mean() >= 1 / 3, np.isfinite(depth).mean()
    assert (cb[:, 3] == 1.0).mean() >= 1 / 10, (cb[:, 3] == 1.0).mean()
    assert steps.mean() > 5


@pytest.mark.parametrize("fog", [0, 1, 2, 3])
def test_options_matrix_against_the_oracle(ctx, space, fog):
    rays = make_rays()
    sky = np.arange(len(rays)) % 2 == 0  # odd rays: AIC_RAYS_NO_SKY
    osp = oracle.Space(space)
    for transparency, threshold in ((0, 0.5), (1, 0.5), (2, 0.1), (2, 0.5), (2, 0.9)):
        for lighting in range(5):
            opt = oracle.make_options(fog=fog, transparency=transparency, threshold=threshold, lighting=lighting, view_distance=VD)
            setup_world(ctx, space, opt)
            ref = check_against_oracle(ctx, abi.LAYER_WORLD, osp, opt, rays, sky, f"fog {fog} transparency {transparency}@{threshold} lighting {lighting}")
            if lighting == 3 and transparency == 1:
                # antialiasing = Always changes nothing: one ray per result
                opt_aa = oracle.make_options(fog=fog, transparency=transparency, threshold=threshold, lighting=lighting, antialiasing=2, view_distance=VD)
                ctx.set_options(abi.LAYER_WORLD, to_abi_options(opt_aa))
                check_against_oracle(ctx, abi.LAYER_WORLD, osp, opt, rays, sky, f"fog {fog}, antialiasing Always", ref=ref)


@pytest.mark.parametrize("samples", [1, 3])
def test_bounce_against_the_oracle(ctx, space, samples):
    rays = make_rays()
    sky = np.arange(len(rays)) % 2 == 0
    osp = oracle.Space(space)
    for fog in (0, 3):
        for transparency in (0, 1):
            opt = oracle.make_options(fog=fog, transparency=transparency, lighting=5, bounce_samples=samples, view_distance=VD)
            setup_world(ctx, space, opt)
            check_against_oracle(ctx, abi.LAYER_WORLD, osp, opt, rays, sky, f"Bounce {samples} fog {fog} transparency {transparency}")


def test_linear_and_rgba8_outputs_follow_the_colorbuf(ctx, space):
    """AIC_FRAME_OUT_LINEAR is Rgba::from(ColorBuf) of the same batch; without a float flag the result is that colour encoded. Both are pinned to
    frames in test_camera_equivalence; here the three outputs of one batch are tied to each other on rays no camera makes."""
    from tests.test_gpu_linear_parity import colorbuf_to_rgba

    rays = make_rays(1500, seed=5)
    opt = oracle.make_options(fog=2, lighting=3, view_distance=VD)
    setup_world(ctx, space, opt)
    for include_sky in (True, False):
        sky = np.full(len(rays), include_sky)
        cb = device_rays(ctx, abi.LAYER_WORLD, rays, sky)[0]
        lin = device_rays(ctx, abi.LAYER_WORLD, rays, sky, flags=abi.FRAME_OUT_LINEAR)[0]
        assert_bits(lin, colorbuf_to_rgba(cb), f"linear output, include_sky {include_sky}")
        enc = device_rays(ctx, abi.LAYER_WORLD, rays, sky, flags=0)[0]
        assert (enc[:, 3] == np.round(lin[:, 3] * np.float32(255.0)).astype(np.uint8)).all()
        if not include_sky:
            assert (lin[:, 3] == 0).any() and (enc[lin[:, 3] == 0] == 0).all()  # a miss ends transparent


# --- 2. edge rays ----------------------------------------------------------------------------------------------------------------
def edge_rays(sp):
    opaque_index = len(sp.blocks) - 3  # colour_space's opaque emissive atom
    where = np.argwhere(sp.block_index == opaque_index)
    assert len(where), "colour_space lost its opaque atoms"
    inside = where[0] + np.asarray(sp.lo) + 0.5
    nan, inf = float("nan"), float("inf")
    return {
        "zero direction": [3.5, 7.5, 30.0, 0.0, 0.0, 0.0],
        "NaN in the origin": [nan, 7.5, 30.0, 0.1, -0.2, -1.0],
        "NaN in the direction": [3.5, 7.5, 30.0, 0.1, nan, -1.0],
        "an infinite direction component": [3.5, 7.5, 30.0, 0.1, -0.2, -inf],
        "origin at 1e9": [1e9, 7.5, 10.5, -1.0, 0.0, 0.0],
        "direction length 1e-200": [10.5, 12.0, 24.0, -0.5e-200, -8e-201, -2e-200],
        "direction length 1e120": [10.5, 12.0, 24.0, -0.5e120, -8e119, -2e120],
        "origin 1e300, direction -1e300": [1e300, 1e300, 1e300, -1e300, -1e300, -1e300],
        "origin inside an opaque block": [inside[0], inside[1], inside[2], 0.3, 0.2, -1.0],
        "origin on a cube boundary": [10.0, 6.0, 24.0, 0.0, -0.25, -1.0],
        "origin on a cube corner, diagonal": [0.0, 0.0, 0.0, 1.0, 1.0, 1.0],
    }


def test_edge_rays_alone_and_inside_a_batch(ctx, space):
    osp = oracle.Space(space)
    filler = make_rays(128, seed=11)
    for opt in (oracle.make_options(fog=3, transparency=1, lighting=3, view_distance=VD), oracle.make_options(fog=0, transparency=0, lighting=1, view_distance=VD)):
        setup_world(ctx, space, opt)
        for name, ray in edge_rays(space).items():
            ray = np.asarray(ray, np.float64)
            for include_sky in (True, False):
                alone = ray.reshape(1, 6)
                ref = check_against_oracle(ctx, abi.LAYER_WORLD, osp, opt, alone, np.array([include_sky]), f"{name}, alone, sky {include_sky}, fog {opt.fog}")
                batch = np.concatenate([filler[:64], alone, filler[64:]])
                sky = np.full(len(batch), include_sky)
                got = check_against_oracle(ctx, abi.LAYER_WORLD, osp, opt, batch, sky, f"{name}, in a batch, sky {include_sky}, fog {opt.fog}")
                assert (bits32(got[0][64]) == bits32(ref[0][0])).all() and got[1][64] == ref[1][0]
    # what the degenerate ones are, by the oracle: no steps and the sky sample (or nothing at all)
    opt = oracle.make_options(fog=0, view_distance=VD)
    for name in ("zero direction", "NaN in the origin", "NaN in the direction", "an infinite direction component", "direction length 1e120"):
        n, cb, depth = oracle.trace_ray(osp, opt, edge_rays(space)[name][0:3], edge_rays(space)[name][3:6])
        assert n == 0 and cb[3] == 0.0 and depth == np.inf, (name, n, cb, depth)


# --- 3. camera equivalence ------------------------------------------------------------------------------------------------------
def camera_rays(inv, w, h):
    """Camera::project_ndc_into_world (camera_struct.rs:238-257) at every pixel's patch centre, in the reference's own f64 operations: [h * w, 6]."""
    m = np.asarray(inv, np.float64).reshape(16)
    ex = np.arange(w + 1, dtype=np.float64) / np.float64(w) * 2.0 - 1.0
    ey = -(np.arange(h + 1, dtype=np.float64) / np.float64(h) * 2.0 - 1.0)
    X, Y = np.meshgrid((ex[:-1] + ex[1:]) / 2.0, (ey[:-1] + ey[1:]) / 2.0)

    def unproject(z):
        out = [X * m[k] + Y * m[4 + k] + z * m[8 + k] + m[12 + k] for k in range(4)]
        with np.errstate(divide="ignore", invalid="ignore"):
            return [np.where(out[3] > 0.0, out[k] / out[3], np.nan) for k in range(3)]

    near, far = unproject(0.0), unproject(1.0)
    rays = np.stack(near + [f - n for f, n in zip(far, near)], -1).reshape(-1, 6)
    # (the restatement is pinned to the oracle's on a sample of the pixels)
    for i in np.unique(np.linspace(0, w * h - 1, 257).astype(int)):
        o, d = oracle.project_ndc_into_world(inv, float(X.reshape(-1)[i]), float(Y.reshape(-1)[i]))
        assert (bits64(rays[i]) == bits64(np.concatenate([o, d]))).all(), i
    return np.ascontiguousarray(rays)


def check_frame_equivalence(ctx, w, h, inv, what, exposure=1.0):
    rays = camera_rays(inv, w, h)
    sky = np.ones(len(rays), bool)
    frame_cb = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_COLORBUF), want_aux=True)
    frame_lin = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_LINEAR))["rgba8"].reshape(-1, 4)
    frame_enc = ctx.render(ctx.make_frame(w, h, world_inv=inv, exposure=exposure))["rgba8"].reshape(-1, 4)
    want_cb, want_aux = frame_cb["rgba8"].reshape(-1, 4), frame_cb["aux"].reshape(-1)
    got, aux, total, variants = device_rays(ctx, abi.LAYER_WORLD, rays, sky, want_aux=True)
    assert variants == {abi.VARIANT_RECORDING}
    assert_bits(got, want_cb, f"{what}: ColorBuf, recording variant")
    assert total == frame_cb["info"].cubes_traced
    for k in AUX_FIELDS:
        assert (aux[k] == want_aux[k]).all(), (what, k)
    assert (bits64(aux["t_distance"]) == bits64(want_aux["t_distance"])).all(), what
    for name, tune in (("plain", PLAIN), ("exchanging", EXCHANGING)):
        got, _, total, variants = device_rays(ctx, abi.LAYER_WORLD, rays, sky, flags=abi.FRAME_OUT_COLORBUF | tune)
        assert variants <= {abi.VARIANT_PLAIN, abi.VARIANT_EXCHANGING}
        assert_bits(got, want_cb, f"{what}: ColorBuf, {name} variant")
        assert total == frame_cb["info"].cubes_traced
        assert_bits(device_rays(ctx, abi.LAYER_WORLD, rays, sky, flags=abi.FRAME_OUT_LINEAR | tune)[0], frame_lin, f"{what}: linear, {name} variant")
        enc = device_rays(ctx, abi.LAYER_WORLD, rays, sky, flags=tune, exposure=exposure)[0]
        assert (enc == frame_enc).all(), (what, name, int((enc != frame_enc).any(axis=-1).sum()))


def test_camera_equivalence_small_frames(ctx, space):
    w, h = 96, 64
    for opt, exposure in ((oracle.make_options(fog=3, transparency=1, lighting=3, view_distance=VD), 1.0),
                          (oracle.make_options(fog=2, transparency=0, lighting=1, tone_mapping=1, maximum_intensity=2.5, view_distance=VD), 2.0),
                          (oracle.make_options(fog=1, transparency=2, threshold=0.5, lighting=0, tone_mapping=0, maximum_intensity=1.0, view_distance=VD), 0.5)):
        setup_world(ctx, space, opt)
        inv = camera((w, h), view_distance=opt.view_distance)
        check_frame_equivalence(ctx, w, h, inv, f"96x64 fog {opt.fog} transparency {opt.transparency}", exposure=exposure)
    # and the frame is the oracle's, so the rays are: the chain is closed on the CPU side once
    opt = oracle.make_options(fog=3, transparency=1, lighting=3, view_distance=VD)
    inv = camera((48, 32), view_distance=VD)
    rays = camera_rays(inv, 48, 32)
    ref = oracle.render(oracle.Space(space), opt, oracle.make_camera(inv, 48, 32), want_aux=True)
    cb, steps, _ = oracle_rays(oracle.Space(space), opt, rays, np.ones(len(rays), bool))
    assert int(steps.sum()) == int(ref["info"]["cubes_traced"]) and (steps == ref["aux"]["cubes_traced"].reshape(-1)).all()
    setup_world(ctx, space, opt)
    assert_bits(device_rays(ctx, abi.LAYER_WORLD, rays, np.ones(len(rays), bool))[0], cb, "48x32 camera rays against the oracle")


def test_camera_equivalence_big_block_table(ctx):
    """The BIG kernels (a block table past 16384 entries), as tests/test_gpu_linear_parity.py test_big_block_table_linear_bits builds one."""
    rng = np.random.default_rng(31)
    sp = flat.FlatSpace((0, 0, 0), (12, 10, 12))
    sp.set_sky_octants(np.random.default_rng(4).uniform(0.1, 1.2, (8, 3)))
    sp.add_block(flat.air())
    sp.add_block(flat.atom((0.5, 0.6, 0.9, 0.35), emission=(0.4, 0.1, 0.0)))
    [sp.add_block(b) for b in workloads.synthetic_blocks(8, 6, seed=5)]
    while len(sp.blocks) < 16385:
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
    inv = camera((w, h), eye=(6.0, 8.5, 17.0), target=(6, 2, 6), view_distance=30.0)
    for transparency, lighting, fog in ((1, 3, 2), (0, 1, 3)):
        opt = oracle.make_options(fog=fog, transparency=transparency, lighting=lighting, view_distance=30.0)
        setup_world(ctx, sp, opt)
        check_frame_equivalence(ctx, w, h, inv, f"BIG <transparency {transparency}, lighting {lighting}>")
    # ... and against the oracle directly, rays no camera makes
    rays = make_rays(1000, seed=3)
    rays[:, 0:3] = rays[:, 0:3] * 0.6  # (the space is 12 x 10 x 12)
    sky = np.arange(len(rays)) % 2 == 0
    check_against_oracle(ctx, abi.LAYER_WORLD, oracle.Space(sp), opt, rays, sky, "BIG, free rays")


def test_camera_equivalence_full_size_on_the_device(ctx):
    """The 1920 x 1080 atrium frame's 2 073 600 camera rays through AIC_RAYS_DEVICE: rays, results and first-hit records stay in device memory."""
    import bench
    import torch

    sp, (w, h), eye, target, vd, _ = bench.build_workload("atrium")
    opt = oracle.make_options(fog=3, view_distance=vd, tone_mapping=1, maximum_intensity=2.5)
    _, _, inv = oracle.camera_matrices(90.0, vd, w / h, oracle.look_at_y_up(eye, target), eye)
    setup_world(ctx, sp, opt)
    n = w * h
    rays = torch.from_numpy(camera_rays(inv, w, h)).cuda()
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    aux = torch.zeros((n, abi.PIXEL_AUX_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    enc = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    frame = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_COLORBUF), want_aux=True)
    info = ctx.trace_rays_device(abi.LAYER_WORLD, n, rays.data_ptr(), out.data_ptr(), flags=abi.FRAME_OUT_COLORBUF)
    assert info.variant == abi.VARIANT_EXCHANGING and info.rows_rendered == n and info.tile_queues == 0
    assert info.cubes_traced == frame["info"].cubes_traced
    assert_bits(out.cpu().numpy(), frame["rgba8"].reshape(-1, 4), "1080p atrium, exchanging variant")
    out.zero_()
    torch.cuda.synchronize()
    info = ctx.trace_rays_device(abi.LAYER_WORLD, n, rays.data_ptr(), out.data_ptr(), aux_ptr=aux.data_ptr(), flags=abi.FRAME_OUT_COLORBUF)
    assert info.variant == abi.VARIANT_RECORDING and info.cubes_traced == frame["info"].cubes_traced
    assert_bits(out.cpu().numpy(), frame["rgba8"].reshape(-1, 4), "1080p atrium, recording variant")
    got_aux = aux.cpu().numpy().view(abi.PIXEL_AUX_DTYPE).reshape(-1)
    want_aux = frame["aux"].reshape(-1)
    for k in AUX_FIELDS:
        assert (got_aux[k] == want_aux[k]).all(), k
    assert (bits64(got_aux["t_distance"]) == bits64(want_aux["t_distance"])).all()
    ctx.trace_rays_device(abi.LAYER_WORLD, n, rays.data_ptr(), enc.data_ptr(), exposure=2.0)
    want = ctx.render(ctx.make_frame(w, h, world_inv=inv, exposure=2.0))["rgba8"].reshape(-1, 4)
    assert (enc.cpu().numpy() == want).all()
    # a few rows against the oracle itself
    osp = oracle.Space(sp)
    host_rays = rays.cpu().numpy()
    got = out.cpu().numpy()
    for y in (0, h // 3, h - 1):
        sel = slice(y * w, y * w + w, 16)
        cb, steps, _ = oracle_rays(osp, opt, host_rays[sel], np.ones(len(host_rays[sel]), bool))
        assert_bits(got[sel], cb, f"1080p atrium row {y} against the oracle")
        assert (got_aux["cubes_traced"][sel] == steps).all()


# --- 4. the UI layer as target -----------------------------------------------------------------------------------------------------
def test_ui_layer_without_sky(ctx, space):
    ui = scenes.ui_space()
    opt = oracle.make_options(fog=2, lighting=3, view_distance=VD)
    ctx.upload_space(abi.LAYER_WORLD, space)
    ctx.set_options(abi.LAYER_WORLD, to_abi_options(oracle.make_options(fog=0, lighting=0, view_distance=50.0)))  # (not the layer traced: must not matter)
    ctx.upload_space(abi.LAYER_UI, ui)
    ctx.set_options(abi.LAYER_UI, to_abi_options(opt))
    try:
        w, h = 64, 48
        _, _, ui_inv = oracle.camera_matrices(90.0, VD, w / h, (0, 0, 0, 1), (-2.5, -2.5, -1.0))
        rng = np.random.default_rng(8)
        free = np.concatenate([rng.uniform(-6.0, 0.0, (500, 3)), rng.normal(size=(500, 3))], 1)
        free[::2, 3:6] = np.array([-2.5, -2.5, -3.5]) - free[::2, 0:3]
        rays = np.concatenate([camera_rays(ui_inv, w, h), free])
        for include_sky in (False, True):
            ref = check_against_oracle(ctx, abi.LAYER_UI, oracle.Space(ui), opt, rays, np.full(len(rays), include_sky), f"UI layer, sky {include_sky}")
            assert np.isfinite(ref[2]).mean() > 0.1 and (~np.isfinite(ref[2])).mean() > 0.1
            if not include_sky:
                assert (ref[0][~np.isfinite(ref[2]), 3] == 1.0).all()
        # the world layer next to it is untouched by the swap
        world_rays = make_rays(500, seed=2)
        wopt = oracle.make_options(fog=0, lighting=0, view_distance=50.0)
        check_against_oracle(ctx, abi.LAYER_WORLD, oracle.Space(space), wopt, world_rays, np.ones(len(world_rays), bool), "world layer beside a UI layer")
    finally:
        ctx.clear_space(abi.LAYER_UI)


# --- 5. protocol -------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx, space):
    import torch

    opt = oracle.make_options(fog=3, lighting=3, view_distance=VD)
    setup_world(ctx, space, opt)
    rays = make_rays(300, seed=4)
    good = ctx.trace_rays(abi.LAYER_WORLD, rays, flags=abi.FRAME_OUT_COLORBUF, want_aux=True)

    def still_good():
        again = ctx.trace_rays(abi.LAYER_WORLD, rays, flags=abi.FRAME_OUT_COLORBUF, want_aux=True)
        assert (bits32(again["rgba8"]) == bits32(good["rgba8"])).all() and (again["aux"] == good["aux"]).all()
        assert again["info"].cubes_traced == good["info"].cubes_traced

    def refused(code, **kw):
        with pytest.raises(abi.AicError) as e:
            ctx.trace_rays(kw.pop("layer", abi.LAYER_WORLD), rays, **kw)
        assert e.value.code == code, (kw, str(e.value))
        still_good()

    refused(1, layer=abi.LAYER_UI)  # a layer without a space
    refused(1, exposure=float("nan"))
    refused(1, exposure=-1.0)
    refused(1, flags=abi.FRAME_OUT_LINEAR | abi.FRAME_OUT_COLORBUF)
    refused(5, flags=abi.FRAME_BLOOM)
    with pytest.raises(abi.AicError) as e:
        ctx.trace_rays(7, rays)
    assert e.value.code == 1
    # more than 2048 x 65535 rays: refused before anything is read (the buffers here are far smaller)
    dev_rays = torch.from_numpy(rays).cuda()
    dev_out = torch.zeros((len(rays), 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(abi.AicError) as e:
        ctx.trace_rays_device(abi.LAYER_WORLD, abi.MAX_RAYS + 1, dev_rays.data_ptr(), dev_out.data_ptr(), flags=abi.FRAME_OUT_COLORBUF)
    assert e.value.code == 1
    still_good()
    with pytest.raises(abi.AicError) as e:  # device rays off their 16-byte boundary
        ctx.trace_rays_device(abi.LAYER_WORLD, 10, dev_rays.data_ptr() + 8, dev_out.data_ptr(), flags=abi.FRAME_OUT_COLORBUF)
    assert e.value.code == 1
    still_good()
    # slot 0 busy
    w, h = 96, 64
    inv = camera((w, h))
    buf = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_submit(ctx.make_frame(w, h, world_inv=inv), buf.data_ptr(), 0)
    with pytest.raises(abi.AicError) as e:
        ctx.trace_rays(abi.LAYER_WORLD, rays)
    assert e.value.code == 1
    ctx.render_wait(0)
    still_good()
    # the device form of the good call: the same results, any whole number of rays into the buffers
    info = ctx.trace_rays_device(abi.LAYER_WORLD, len(rays) - 7, dev_rays.data_ptr() + 7 * 48, dev_out.data_ptr() + 7 * 16, flags=abi.FRAME_OUT_COLORBUF)
    assert info.rows_rendered == len(rays) - 7
    got = dev_out.cpu().numpy()
    assert (bits32(got[7:]) == bits32(good["rgba8"][7:])).all() and (got[:7] == 0).all()
    # n = 0
    empty = ctx.trace_rays(abi.LAYER_WORLD, np.zeros((0, 6)), want_aux=True)
    assert empty["rgba8"].shape == (0, 4) and empty["info"].rows_rendered == 0 and empty["info"].cubes_traced == 0


def test_batch_sizes_around_a_wave_and_a_row(ctx, space):
    opt = oracle.make_options(fog=3, lighting=3, view_distance=VD)
    setup_world(ctx, space, opt)
    osp = oracle.Space(space)
    rays = make_rays(2049, seed=6)
    ref = oracle_rays(osp, opt, rays, np.ones(len(rays), bool))
    for n in (1, 63, 64, 65, 2049):
        check_against_oracle(ctx, abi.LAYER_WORLD, osp, opt, rays[:n], np.ones(n, bool), f"n = {n}", ref=tuple(r[:n] for r in ref))


def test_a_batch_beside_streamed_frames(ctx, space):
    import torch

    opt = oracle.make_options(fog=3, lighting=3, view_distance=VD)
    setup_world(ctx, space, opt)
    rays = make_rays(3000, seed=9)
    sky = np.ones(len(rays), bool)
    want = device_rays(ctx, abi.LAYER_WORLD, rays, sky)[0]
    w, h = 320, 200
    frames = [ctx.make_frame(w, h, world_inv=camera((w, h), eye=(10.5 + j, 12.0, 24.0 - j))) for j in range(3)]
    want_frames = [ctx.render(f)["rgba8"] for f in frames]
    bufs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    for rounds in range(3):
        for j, f in enumerate(frames):
            ctx.render_submit(f, bufs[j].data_ptr(), j + 1)
        got = device_rays(ctx, abi.LAYER_WORLD, rays, sky)[0]
        for j in range(3):
            ctx.render_wait(j + 1)
        torch.cuda.synchronize()
        assert_bits(got, want, f"batch beside slots 1-3, round {rounds}")
        for j in range(3):
            assert (bufs[j].cpu().numpy() == want_frames[j]).all(), (rounds, j)
            bufs[j].zero_()
        torch.cuda.synchronize()


def test_rays_and_views_of_the_ui_layer_beside_a_light_update_of_the_world():
    """Rays and orthographic views of the UI layer's space are traced in the world's seat of the launch, and neither waits for a light update that
    runs on the context's worker thread (found by tests/test_gpu_session_fuzz.py: the two Layer objects used to be swapped around the submit, the
    worker found the UI layer's space under its reference to the world, and an update of 2553 cubes ended after 26). An update long enough to run
    beside twelve such calls -- a few cubes changed in a light field that is nobody's fixed point, no cap -- must come out as the blocking call
    makes it on a second context, and every batch as it is traced with nothing else going on."""
    world = workloads.synthetic_space(n=16, resolution=8, n_blocks=6, seed=165, light="field")
    ui = flat.FlatSpace((0, 0, 0), (3, 2, 1))
    ui.set_sky_uniform((1.0, 1.0, 0.5))
    ui.add_block(flat.air())
    ui.block_index[0, 0, 0] = ui.add_block(flat.atom((0.0, 1.0, 0.0, 1.0)))
    ui.block_index[2, 1, 0] = ui.add_block(flat.atom((0.9, 0.2, 0.1, 0.5)))
    rng = np.random.default_rng(11)
    rays = np.concatenate([rng.uniform(-1.0, 4.0, (700, 3)), rng.normal(size=(700, 3))], 1)
    xyz = np.array([[3, 9, 4], [8, 10, 8], [12, 9, 3], [5, 11, 12]], np.int32)
    kw = dict(maximum_distance=4, fast=False, queue=[], max_updates=0, batch=256)
    with abi.Context(0) as a, abi.Context(0) as b:
        for c in (a, b):
            c.upload_space(abi.LAYER_WORLD, world)
            c.upload_space(abi.LAYER_UI, ui)
            c.update_cubes(abi.LAYER_WORLD, xyz, np.array([1, 2, 6, 7], np.uint16))
            c.light_cubes_changed(abi.LAYER_WORLD, xyz)
        want_rays, want_view = b.trace_rays(abi.LAYER_UI, rays, want_aux=True), b.render_orthographic(abi.LAYER_UI, 4)
        a.evaluate_light_submit(abi.LAYER_WORLD, **kw)
        beside = 0
        for _ in range(6):
            beside += not a.evaluate_light_done(abi.LAYER_WORLD)
            got_rays, got_view = a.trace_rays(abi.LAYER_UI, rays, want_aux=True), a.render_orthographic(abi.LAYER_UI, 4)
            assert (got_rays["rgba8"] == want_rays["rgba8"]).all() and all((got_rays["aux"][k] == want_rays["aux"][k]).all() for k in AUX_FIELDS)
            assert (got_view["rgba8"] == want_view["rgba8"]).all() and got_view["info"].cubes_traced == want_view["info"].cubes_traced
        ia, ib = a.evaluate_light_wait(abi.LAYER_WORLD), b.evaluate_light(abi.LAYER_WORLD, **kw)
        print(f"{ia.updates} updates on the worker, {ib.updates} blocking; {beside} of 6 rounds began while the update ran")
        assert ib.updates > 100, "the update did not spread beyond the changed cubes: too short to run beside anything"
        assert (ia.updates, ia.queue_left) == (ib.updates, ib.queue_left)
        assert (a.read_light_volume(abi.LAYER_WORLD, world.size) == b.read_light_volume(abi.LAYER_WORLD, world.size)).all()


# --- 6. the host mirror --------------------------------------------------------------------------------------------------------------
def test_host_mirror_trace_rays(ctx, space):
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H

    cams = H.StandardCameras()
    cams.graphics_options = H.GraphicsOptions()
    cams.viewport = H.Viewport.with_scale(1.0, 64, 48)
    cams.world_space = A.space_from_flat(space)
    cams.world_view_transform = H.look_at_y_up((10.5, 12.0, 24.0), (10.0, 4.0, 4.0))
    r = H.HipRtRenderer(cams)
    r.update()
    ctx.clear_space(abi.LAYER_UI)
    ctx.upload_space(abi.LAYER_WORLD, space)
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())  # GraphicsOptions::default(), as the mirror's
    rays = make_rays(2000, seed=12)
    for include_sky in (True, False):
        want = ctx.trace_rays(abi.LAYER_WORLD, rays, include_sky=include_sky, flags=abi.FRAME_OUT_COLORBUF, want_aux=True)
        got = r.trace_rays(abi.LAYER_WORLD, rays, include_sky)
        assert_bits(got["colorbuf"], want["rgba8"], f"host mirror, sky {include_sky}")
        hits = np.ascontiguousarray(got["hits"]).view(abi.PIXEL_AUX_DTYPE).reshape(-1)
        assert (hits == want["aux"]).all()
        assert got["info"].rows_rendered == len(rays)
    with pytest.raises(Exception):
        r.trace_rays(abi.LAYER_UI, rays, True)  # no UI space
    assert_bits(r.trace_rays(abi.LAYER_WORLD, rays[:5], True)["colorbuf"], ctx.trace_rays(abi.LAYER_WORLD, rays[:5], flags=abi.FRAME_OUT_COLORBUF)["rgba8"], "after the error")
