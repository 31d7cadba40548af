"""The first lookup of a level, taken by the event that sets the level up (run with -m gpu on an MI355X).

The plain production kernels look up the first cube of a new ray (NEWRAY) and the first voxel of an entered block (ENTER) inside the
event: an invisible one is counted there and the lane goes on stepping; anything else is left to the stepping trip, as before. What
that may not change is everything a ray computes, so every case here is compared with the CPU oracle the way
tests/test_gpu_linear_parity.py and tests/test_gpu_trace_rays.py do: the float colour bits and the RGBA8 bytes with no tolerance, the
step count of every ray (the recording variant's record for ray batches; for frames a second frame with debug_pixel_cost, whose
linear output is 0.02 n per pixel, accum.rs:228-234) and of the frame, and the first-hit records of ray batches. The recording
variant compiles the early lookup out, so its per-ray record says nothing about the variants that take it: every ray batch is traced a
second time with debug_pixel_cost, which puts each ray's own step count into the colour bits of the plain and the exchanging variant. Every case runs
under VARIANT_PLAIN and VARIANT_EXCHANGING; frames are at most 96 x 64 and batches at most 4000 rays.

The cases are the ones in which the early lookup is taken, must not be taken, or sits at an edge of its conditions: the eye's cube
(air, solid, a recursive block), a block's first voxel and stored volume, the 1000-step cap, rays that start opaque, the
transparency / lighting / antialiasing options, and ray origins inside, outside and on the planes of the space's bounds."""
import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi, flat, workloads
from tests import scenes
from tests.test_gpu_linear_parity import assert_bits, assert_rgba8_exact
from tests.test_gpu_parity import to_abi_options
from tests.test_gpu_trace_rays import camera_rays, check_against_oracle, setup_world

pytestmark = pytest.mark.gpu

VARIANTS = (("plain", abi.VARIANT_PLAIN), ("exchanging", abi.VARIANT_EXCHANGING))
VD = 30.0
N = 12  # the scene is [0, 12)^3


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def shell_block(r, alpha=1.0, shell=True):
    """A full R`r` volume: an invisible outer shell (if `shell`) around voxels of two colours of the given alpha."""
    g = np.arange(r)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    vox = (1 + (X + Y + Z) % 2).astype(np.uint16)
    if shell:
        edge = (X == 0) | (Y == 0) | (Z == 0) | (X == r - 1) | (Y == r - 1) | (Z == r - 1)
        vox[edge] = 0
    pal = np.stack([flat.evoxel((0, 0, 0, 0)), flat.evoxel((0.9, 0.3, 0.2, alpha)), flat.evoxel((0.2, 0.5, 0.9, alpha), (0.0, 0.3, 0.1))])
    return flat.voxel_block(r, vox, pal)


def small_volume_block(r, vlo, shape, first_visible):
    """A block whose stored volume is smaller than the block: rays enter the cube and miss the volume, clip it, or cross it."""
    vox = np.ones(shape, np.uint16)
    if not first_visible:
        vox[0, :, :] = 0
        vox[:, :, -1] = 0
    pal = np.stack([flat.evoxel((0, 0, 0, 0)), flat.evoxel((0.8, 0.8, 0.1, 1.0))])
    return flat.voxel_block(r, vox, pal, vlo=vlo)


def scene():
    """The synthetic terrain of the parity tests at 12^3 plus, floating above it, one of each block this change treats differently: first voxel
    invisible / visible / translucent, and stored volumes smaller than the block (a 2 x 2 x 2 corner, a single voxel, a thin slab)."""
    sp = workloads.synthetic_space(n=N, resolution=8, n_blocks=8, seed=5, light="field")
    sp.set_sky_octants(np.random.default_rng(3).uniform(0.1, 1.4, (8, 3)))
    special = [shell_block(8), shell_block(8, shell=False), shell_block(4, alpha=0.5, shell=False), shell_block(4, alpha=0.5),
               small_volume_block(4, (1, 1, 1), (2, 2, 2), True), small_volume_block(8, (3, 3, 3), (1, 1, 1), True),
               small_volume_block(8, (0, 5, 0), (8, 1, 8), False), small_volume_block(4, (2, 0, 1), (2, 4, 2), False)]
    idx = [sp.add_block(b) for b in special]
    k = 0
    for x in range(1, N - 1, 2):
        for z in range(1, N - 1, 2):
            sp.set((x, 8 + (k % 2), z), idx[k % len(idx)])
            k += 1
    return sp, idx


@pytest.fixture(scope="module")
def world():
    return scene()


def air_index(sp):
    return next(i for i, b in enumerate(sp.blocks) if getattr(b, "is_air", False))


def camera(size, eye, target, fov=90.0, view_distance=VD):
    w, h = size
    _, _, inv = oracle.camera_matrices(fov, view_distance, w / h, oracle.look_at_y_up(eye, target), eye)
    return inv


def check_frame(ctx, sp, opt, size, inv, what, ui=None, ui_inv=None, backdrop=None):
    """Linear bits, RGBA8 and the frame's step total of both production variants against the oracle; then the same frame with
    debug_pixel_cost, which shows every pixel's step count in the linear output."""
    w, h = size
    osp, cam = oracle.Space(sp), oracle.make_camera(inv, w, h)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    kw, okw = {}, {}
    if ui is not None:
        ctx.upload_space(abi.LAYER_UI, ui)
        kw["ui_inv"] = ui_inv
        okw = dict(ui=oracle.Space(ui), ui_cam=oracle.make_camera(ui_inv, w, h))
    else:
        ctx.clear_space(abi.LAYER_UI)
    if backdrop is not None:
        kw["backdrop"] = backdrop
        okw["backdrop"] = backdrop
    try:
        for cost in (False, True):
            o = oracle.make_options(fog=opt.fog, transparency=opt.transparency, lighting=opt.lighting, antialiasing=opt.antialiasing,
                                    view_distance=opt.view_distance, debug_pixel_cost=cost)
            ctx.set_options(abi.LAYER_WORLD, to_abi_options(o))
            if ui is not None:  # (the UI layer without debug_pixel_cost, which would make every pixel opaque before the world pass)
                ctx.set_options(abi.LAYER_UI, to_abi_options(opt))
                okw["ui_opt"] = opt
            ref = oracle.render(osp, o, cam, want_linear=True, **okw)
            for name, variant in VARIANTS:
                tune = abi.tuning(variant=variant)
                tag = f"{what}, {name} variant" + (", debug_pixel_cost" if cost else "")
                lin = ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_LINEAR, tuning=tune, **kw))
                assert lin["info"].variant in (variant, abi.VARIANT_PLAIN), (tag, lin["info"].variant)
                assert lin["info"].cubes_traced == int(ref["info"]["cubes_traced"]), (tag, lin["info"].cubes_traced, int(ref["info"]["cubes_traced"]))
                assert_bits(lin["rgba8"], ref["linear"], tag)
                img = ctx.render(ctx.make_frame(w, h, world_inv=inv, tuning=tune, **kw))
                assert_rgba8_exact(img["rgba8"], ref["rgba8"], tag)
    finally:
        ctx.clear_space(abi.LAYER_UI)
    return ref


# --- the eye's cube, and the eye outside the space ------------------------------------------------------------------------------
EYE_CUBE = (6, 10, 6)


@pytest.mark.parametrize("eye_in", ["air", "solid", "recursive block", "translucent block", "outside"])
def test_the_eyes_cube(ctx, world, eye_in):
    idx = world[1]
    sp = scene()[0]  # (a copy of its own: the eye's cube is replaced)
    eye = (6.4, 10.3, 6.6)
    if eye_in == "air":
        sp.set(EYE_CUBE, air_index(sp))
    elif eye_in == "solid":
        sp.set(EYE_CUBE, sp.add_block(flat.atom((0.2, 0.7, 0.3, 1.0))))
    elif eye_in == "recursive block":
        sp.set(EYE_CUBE, idx[0])  # the eye's voxel is a visible one behind an invisible shell ... of the far side
    elif eye_in == "translucent block":
        sp.set(EYE_CUBE, idx[2])
    else:
        eye = (6.4, 10.3, 19.5)  # fast-forward taken
    size = (48, 32)
    inv = camera(size, eye, (5.0, 5.0, 1.0))
    for transparency in (0, 1):
        opt = oracle.make_options(fog=3, transparency=transparency, lighting=3, view_distance=VD)
        check_frame(ctx, sp, opt, size, inv, f"eye in {eye_in}, transparency {transparency}")


# --- options: Surface / Volumetric, Flat / Linear, antialiasing (NEWRAY without TAKE: four samples per pixel) ---------------------
@pytest.mark.parametrize("aa", [0, 2])
@pytest.mark.parametrize("lighting", [1, 3])
def test_options(ctx, world, lighting, aa):
    sp, _ = world
    size = (96, 64) if (lighting == 3 and aa == 0) else (48, 32)
    inv = camera(size, (6.5, 11.5, 13.5), (6.0, 7.0, 3.0))  # outside, looking down at the special blocks
    for transparency in (0, 1):
        opt = oracle.make_options(fog=2, transparency=transparency, lighting=lighting, antialiasing=aa, view_distance=VD)
        check_frame(ctx, sp, opt, size, inv, f"transparency {transparency} lighting {lighting} aa {aa}")


# --- opaque from the start: such rays count one step and end -----------------------------------------------------------------------
def test_rays_that_start_opaque(ctx, world):
    sp, _ = world
    size = (48, 32)
    w, h = size
    inv = camera(size, (6.4, 10.3, 11.5), (5.0, 6.0, 1.0))
    ui = scenes.ui_space()
    _, _, ui_inv = oracle.camera_matrices(90.0, VD, w / h, (0, 0, 0, 1), (-2.5, -2.5, -1.5))  # the UI cube covers the middle of the frame
    for transparency, aa in ((1, 0), (0, 2)):
        opt = oracle.make_options(fog=3, transparency=transparency, lighting=3, antialiasing=aa, view_distance=VD)
        ref = check_frame(ctx, sp, opt, size, inv, f"backdrop alpha 1, transparency {transparency} aa {aa}", backdrop=(0.2, 0.4, 0.6, 1.0))
        assert int(ref["info"]["cubes_traced"]) == w * h * (4 if aa else 1)  # (debug_pixel_cost frame: one step per ray)
        check_frame(ctx, sp, opt, size, inv, f"backdrop alpha 0.5, transparency {transparency} aa {aa}", backdrop=(0.2, 0.4, 0.6, 0.5))
        ref = check_frame(ctx, sp, opt, size, inv, f"UI layer (use_init), transparency {transparency} aa {aa}", ui=ui, ui_inv=ui_inv)
        steps = np.round(ref["linear"][..., 0] / np.float32(0.02))  # (the debug_pixel_cost frame) pixels the UI made opaque, and pixels it left to the world
        assert (steps <= 2 * (4 if aa else 1)).any() and (steps > 5 * (4 if aa else 1)).any()


def check_rays(ctx, sp, rays, sky, what, **options):
    """The batch against oracle.trace_ray under the given options, then again with debug_pixel_cost: the ColorBuf of that second run is
    (0.02 n, 0.002 n, ., 1) of the ray's own step count n, so the plain and the exchanging variant are pinned ray by ray, not only in the sum."""
    osp = oracle.Space(sp)
    out = None
    for cost in (False, True):
        opt = oracle.make_options(debug_pixel_cost=cost, **options)
        setup_world(ctx, sp, opt)
        res = check_against_oracle(ctx, abi.LAYER_WORLD, osp, opt, rays, sky, what + (", debug_pixel_cost" if cost else ""))
        if cost:
            n = res[1].astype(np.float32)
            assert (res[0][:, 0] == np.float32(0.02) * n).all(), what  # (the oracle's colour does carry the count: the run checks what it claims)
        else:
            out = res
    return out


# --- ray batches: a block's first voxel and stored volume, origins at the bounds, degenerate rays -------------------------------------
def block_rays(sp, idx, rng, n_per_cube=54):
    """Rays aimed at the special blocks from outside their cubes (hitting the stored volume, clipping it, missing it), rays starting inside
    their cubes, and zero-direction rays inside them (a level that emits its one cube and cannot go on)."""
    rays = []
    lo = np.asarray(sp.lo, np.float64)
    for c in np.argwhere(np.isin(sp.block_index, idx)):
        centre = c + lo + 0.5
        for k in range(n_per_cube):
            o = centre + rng.uniform(-3.0, 3.0, 3)
            if k % 6 == 4:
                o = centre + rng.uniform(-0.5, 0.5, 3)  # starts inside the block's cube
            target = centre + rng.uniform(-0.55, 0.55, 3)
            d = (target - o) * rng.choice([0.5, 1.0, 30.0])
            if k % 6 == 5:
                d = d * 0.0
                o = centre + rng.uniform(-0.5, 0.5, 3)
            if k % 9 == 7:
                d[int(rng.integers(0, 3))] = 0.0  # an axis the ray does not move along
            rays.append(np.concatenate([o, d]))
    return np.ascontiguousarray(np.asarray(rays, np.float64))


def test_a_blocks_first_voxel_and_stored_volume(ctx, world):
    sp, idx = world
    rays = block_rays(sp, idx, np.random.default_rng(21))
    assert 1000 < len(rays) <= 4000
    sky = np.arange(len(rays)) % 3 != 0
    for transparency, lighting in ((0, 1), (1, 3)):
        check_rays(ctx, sp, rays, sky, f"block rays, transparency {transparency} lighting {lighting}", fog=3, transparency=transparency, lighting=lighting, view_distance=VD)


def bounds_rays(rng):
    """One batch whose waves mix origins inside the space, outside it, exactly on its lo and hi planes (going in and going out), and
    NaN / infinite / 1e300 origins: 64 consecutive rays hold several kinds."""
    n = 2048
    o = rng.uniform(0.0, float(N), (n, 3))
    d = rng.normal(size=(n, 3)) * rng.choice([1e-2, 1.0, 25.0], n)[:, None]
    kind = np.arange(n) % 8
    outside = kind == 1
    o[outside] = rng.uniform(-8.0, float(N) + 8.0, (int(outside.sum()), 3))
    d[outside] = (rng.uniform(0.0, float(N), (int(outside.sum()), 3)) - o[outside]) * 1.5
    for k, plane in ((2, 0.0), (3, float(N))):
        sel = np.nonzero(kind == k)[0]
        axis = rng.integers(0, 3, len(sel))
        o[sel, axis] = plane
        d[sel, axis] = np.abs(d[sel, axis]) * np.where(np.arange(len(sel)) % 2 == 0, 1.0, -1.0)  # alternately up and down that axis
        d[sel[::5], (axis[::5] + 1) % 3] = 0.0
    corner = np.nonzero(kind == 4)[0]
    o[corner] = rng.choice([0.0, float(N)], (len(corner), 3))
    odd = np.nonzero(kind == 5)[0]
    bad = [np.nan, np.inf, -np.inf, 1e300, -1e300, 3e9, -3e9, 2147483647.5]
    for j, i in enumerate(odd):
        o[i, j % 3] = bad[(j // 3) % len(bad)]
    integral = kind == 6
    o[integral] = np.round(o[integral])  # origins on cube boundaries inside the space
    return np.ascontiguousarray(np.concatenate([o, d], 1))


def test_origins_inside_outside_and_on_the_bounds(ctx, world):
    sp, _ = world
    rays = bounds_rays(np.random.default_rng(33))
    sky = np.arange(len(rays)) % 2 == 0
    options = dict(fog=3, transparency=1, lighting=3, view_distance=VD)
    cb, steps, depth = check_rays(ctx, sp, rays, sky, "origins at the bounds", **options)
    assert (steps == 0).any() and (steps > 10).any() and np.isfinite(depth).mean() > 0.2
    # a wave of rays that all start inside, and one that all start outside
    inside = rays[(np.arange(len(rays)) % 8 == 0) | (np.arange(len(rays)) % 8 == 7)][:256]
    check_rays(ctx, sp, inside, np.ones(len(inside), bool), "all origins inside", **options)
    out = rays[np.arange(len(rays)) % 8 == 1][:256]
    check_rays(ctx, sp, out, np.ones(len(out), bool), "all origins outside", **options)


# --- the 1000-step cap (count_step_should_stop, sr.rs:639-651) ------------------------------------------------------------------------
CORRIDOR = 1030


def corridor_space():
    """A 5 x 5 corridor of air, 1030 cubes long, closed at z = 10 by a plane of recursive blocks (invisible shell first) in front of a solid plane."""
    sp = flat.FlatSpace((0, 0, 0), (5, 5, CORRIDOR))
    sp.set_sky_uniform((0.7, 0.8, 1.0))
    a = sp.add_block(flat.air())
    solid = sp.add_block(flat.atom((0.9, 0.2, 0.2, 1.0)))
    shell = sp.add_block(shell_block(4))
    full = sp.add_block(shell_block(4, alpha=0.5, shell=False))
    sp.block_index[...] = a
    sp.block_index[:, :, 9] = solid
    sp.block_index[:, :, 10] = shell
    sp.block_index[::2, :, 10] = full
    sp.light[..., 0:3] = 180
    sp.light[..., 3] = flat.STATUS_VISIBLE
    return sp


def test_the_step_cap_cuts_where_the_oracle_cuts(ctx):
    sp = corridor_space()
    rays = []
    # the block plane's cube is step number k of a ray that starts k - 1 cubes before it: its lookup, the entry into the block and the block's first
    # voxels fall on either side of the cap; rays from outside the far end have their first cube as step 1 and end in the corridor.
    # (A new ray's own first cube cannot fall at the cap: its count is zero at NEWRAY, so that lookup is always step 1. The cap meets the early
    # lookup only in ENTER -- a block entered at counts 998 .. 1001 -- and meets the cubes of the corridor in the stepping trip, as before.)
    for k in range(990, 1006):
        for x, y in ((2.5, 2.5), (1.5, 3.5), (0.25, 0.75)):
            z = 10.5 + (k - 1)
            rays.append([x, y, z, 0.0, 0.0, -1.0])
            rays.append([x, y, z, 0.0004, -0.0003, -1.0])     # a few steps sideways on the way
            rays.append([x, y, z + 0.4, 0.0, 0.0, -40.0])
    for dz in (0.5, 3.0):
        rays.append([2.5, 2.5, CORRIDOR + dz, 0.0, 0.0, -1.0])
        rays.append([2.2, 2.7, CORRIDOR + dz, 0.001, 0.0, -2.0])
    rays = np.ascontiguousarray(np.asarray(rays, np.float64))
    assert (rays[:, 2] < CORRIDOR).sum() > 100
    sky = np.ones(len(rays), bool)
    for transparency in (0, 1):
        cb, steps, depth = check_rays(ctx, sp, rays, sky, f"corridor, transparency {transparency}", fog=0, transparency=transparency, lighting=1, view_distance=2000.0)
        assert steps.max() >= 1000 and (steps < 1000).any()
        assert np.isfinite(depth).any() and (~np.isfinite(depth)).any()  # some reach the blocks, some are cut first
    # and as a frame from inside the corridor, 1000 cubes from its end
    size = (32, 24)
    inv = camera(size, (2.5, 2.5, 10.5 + 996.2), (2.5, 2.5, 0.0), fov=20.0, view_distance=2000.0)
    opt = oracle.make_options(fog=0, transparency=1, lighting=1, view_distance=2000.0)
    check_frame(ctx, sp, opt, size, inv, "corridor frame")
