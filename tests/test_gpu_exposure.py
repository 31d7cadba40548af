"""GPU tests (-m gpu) of aic_sample_luminance, the device's half of automatic exposure (all-is-cubes/src/character/exposure.rs:60-151).

Yardstick: tests/exposure_ref.py, the sampling loop restated over the CPU oracle's Raycaster. Every comparison is of f32 bit patterns: a sample is a
table entry or a sky colour through three multiplications and two additions, one rounding each (no sample is NaN: sky colours and table entries are
finite). Scenes are at most 30^3 cubes and lit once per process; tests/test_exposure_cpu.py checks that the case list reaches every outcome."""

import numpy as np
import pytest

import all_is_cubes_amd as A
import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi, flat
from tests import exposure_ref as ref
from tests import scenes

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
CASES = ref.cases()
W, HGT = 64, 48


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def sample_on_device(ctx, rays, max_steps) -> np.ndarray:
    """The AIC_RAYS_DEVICE form: rays and samples in tensors on the device, a guard element behind the samples"""
    import torch

    r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    d_rays = torch.from_numpy(r.copy()).to("cuda:0")
    d_out = torch.full((len(r) + 1,), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.sample_luminance_device(abi.LAYER_WORLD, len(r), d_rays.data_ptr(), max_steps, d_out.data_ptr())
    out = d_out.cpu().numpy()
    assert out[-1] == -7.0, "wrote past the samples"
    return out[:-1]


def check(ctx, scene: ref.Scene, rays, max_steps, what=""):
    want = scene.sample_all(rays, max_steps)
    got = ctx.sample_luminance(abi.LAYER_WORLD, rays, max_steps)
    assert (bits(got) == bits(want)).all(), (what, np.flatnonzero(bits(got) != bits(want))[:8], got[:4], want[:4])
    got_d = sample_on_device(ctx, rays, max_steps)
    assert (bits(got_d) == bits(want)).all(), (what, "device pointers")
    return want


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_device_equals_the_restatement(ctx, case):
    name, key, rays, max_steps = CASES[case]
    scene = ref.scene(key)
    ctx.upload_space(abi.LAYER_WORLD, scene.sp)
    check(ctx, scene, rays, max_steps, name)


def test_ray_counts_and_step_limits(ctx):
    scene = ref.scene("spread")
    ctx.upload_space(abi.LAYER_WORLD, scene.sp)
    rays = np.concatenate([ref.grid_rays((0.0, 0.0, 0.0, 1.0), (0.5, 0.5, 3.5)), ref.ODD_RAYS])
    whole = {ms: scene.sample_all(rays[:100], ms) for ms in (0, 1, 3, 60, 510)}
    for n in (1, 10, 64, 65, 100):  # (65: a second wave with one live lane)
        for ms, want in whole.items():
            got = ctx.sample_luminance(abi.LAYER_WORLD, rays[:n], ms)
            assert (bits(got) == bits(want[:n])).all(), (n, ms)
        assert (bits(sample_on_device(ctx, rays[:n], 60)) == bits(whole[60][:n])).all(), n
    check(ctx, scene, rays[91:], 60, "the grid's last rays, then a zero direction, NaN and infinite components")
    assert ctx.sample_luminance(abi.LAYER_WORLD, np.zeros((0, 6)), 60).shape == (0,)


def test_the_references_end_to_end_test(ctx):
    """exposure.rs:181-241 through the mirror: an empty 10^3 space under a uniform sky of luminance 3, the eye at its centre, 100 steps of 0.1 s"""
    luminance = 3.0
    sp = flat.FlatSpace((0, 0, 0), (10, 10, 10))
    sp.set_sky_uniform((luminance, luminance, luminance))
    sp.add_block(flat.air())
    cams = H.StandardCameras()
    o = H.GraphicsOptions()
    e = H.ExposureOption()
    e.automatic = True
    o.exposure = e
    cams.graphics_options = o
    cams.viewport = H.Viewport.with_scale(1.0, 16, 16)
    cams.world_space = A.space_from_flat(sp)
    vt = H.ViewTransform.identity()
    vt.translation = (5.0, 5.0, 5.0)
    cams.world_view_transform = vt
    r = H.HipRtRenderer(cams)
    r.update()
    state = H.ExposureState()
    assert state.exposure() == 1.0
    state.step(r, vt, 30, 0.0)
    assert state.sample_index == 0 and state.exposure_log == 0.0  # dt == 0: nothing
    for _ in range(100):
        state.step(r, vt, 30, 0.1)
        cams.measured_exposure = state.exposure()
    assert (state.samples() == np.float32(luminance)).all()
    assert state.luminance_average() == np.float32(luminance)
    expected = H.ExposureState.compute_target_exposure(luminance)
    assert abs(state.exposure() / expected - 1.0) < 0.001, (state.exposure(), expected)
    # ... and the loop's last line reaches the camera: an Automatic camera renders at the measured exposure
    r.update()
    assert r.world_camera().exposure() == state.exposure()
    # the same steps through the C boundary: the same bits
    s2 = abi.ExposureState()
    with abi.Context(0) as c2:
        c2.upload_space(abi.LAYER_WORLD, sp)
        for _ in range(100):
            s2.advance(c2.sample_luminance(abi.LAYER_WORLD, s2.rays(vt.rotation, vt.translation), 60), 0.1)
    assert bits(s2.exposure()) == bits(state.exposure()) and bits(s2.exposure_log) == bits(state.exposure_log)


def test_scene_changes_are_seen(ctx):
    import copy

    rays = np.concatenate([ref.ODD_RAYS[:3], ref.grid_rays((0.0, 0.0, 0.0, 1.0), (0.5, 0.5, 4.5), 64, first=37)])
    sp = copy.deepcopy(ref.scene("ghost").sp)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    before = check(ctx, ref.Scene(sp), rays, 60, "as uploaded")
    ghost, wall = int(sp.block_index[0, 0, 2]), int(sp.block_index[0, 0, 0])
    # a visible block in the rays' way ...
    for cube in ((0, 0, 3), (1, 0, 3)):
        sp.set(cube, wall)
    ctx.update_cubes(abi.LAYER_WORLD, [(0, 0, 3), (1, 0, 3)], [wall, wall])
    blocked = check(ctx, ref.Scene(sp), rays, 60, "a wall block put in the way")
    assert (bits(blocked) != bits(before)).any()
    # ... then an all-invisible voxel block in its place: the rays go through again
    for cube in ((0, 0, 3), (1, 0, 3)):
        sp.set(cube, ghost)
    ctx.update_cubes(abi.LAYER_WORLD, [(0, 0, 3), (1, 0, 3)], [ghost, ghost])
    through = check(ctx, ref.Scene(sp), rays, 60, "an invisible voxel block in its place")
    assert (bits(through) == bits(before)).all()
    # a block redefined: the ghost gets a voxel that emits, and stops the rays
    lit = ref.invisible_voxel_block()
    lit.palette[1, 4:7] = (0.5, 0.5, 0.5)
    sp.blocks[ghost] = lit
    ctx.replace_block(abi.LAYER_WORLD, ghost, lit)
    stopped = check(ctx, ref.Scene(sp), rays, 60, "the block redefined with an emitting voxel")
    assert (bits(stopped) != bits(through)).any()


def test_light_evaluated_on_the_device_is_seen(ctx):
    sp = scenes.light_spread_space()  # (unlit)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    rays = ref.grid_rays((0.0, 0.0, 0.0, 1.0), (0.5, 0.5, 3.5))
    dark = check(ctx, ref.Scene(sp), rays, 60, "unlit")
    ctx.evaluate_light(abi.LAYER_WORLD, 30)
    sp.light = ctx.read_light_volume(abi.LAYER_WORLD, sp.size)
    lit = check(ctx, ref.Scene(sp), rays, 60, "lit on the device")
    assert (bits(lit) != bits(dark)).any()
    # a submitted update is finished and published by the sample itself
    ctx.upload_space(abi.LAYER_WORLD, scenes.light_spread_space())
    ctx.evaluate_light_submit(abi.LAYER_WORLD, 30)
    got = ctx.sample_luminance(abi.LAYER_WORLD, rays, 60)
    ctx.evaluate_light_wait(abi.LAYER_WORLD)
    assert (bits(got) == bits(lit)).all()


def test_with_frames_in_flight(ctx):
    import torch

    scene = ref.scene("spread")
    ctx.upload_space(abi.LAYER_WORLD, scene.sp)
    ctx.set_options(abi.LAYER_WORLD, abi.make_options())
    frames = []
    for eye in ((0.5, 0.5, 8.0), (3.0, -2.0, 6.0)):
        q = oracle.look_at_y_up(eye, (0.0, 0.0, 0.0))
        _, _, inv = oracle.camera_matrices(45.0, 200.0, W / HGT, q, eye)
        frames.append(ctx.make_frame(W, HGT, world_inv=inv))
    alone = [ctx.render(f)["rgba8"] for f in frames]
    rays = ref.grid_rays((0.0, 0.0, 0.0, 1.0), (0.5, 0.5, 3.5))
    quiet = ctx.sample_luminance(abi.LAYER_WORLD, rays, 60)
    assert (bits(quiet) == bits(scene.sample_all(rays, 60))).all()
    outs = [torch.zeros((HGT, W, 4), dtype=torch.uint8, device="cuda:0") for _ in frames]
    torch.cuda.synchronize()
    for slot, (f, o) in enumerate(zip(frames, outs)):
        ctx.render_submit(f, o.data_ptr(), slot)
    busy = ctx.sample_luminance(abi.LAYER_WORLD, rays, 60)
    busy_d = sample_on_device(ctx, rays, 60)
    for slot in range(len(frames)):
        ctx.render_wait(slot)
    assert (bits(busy) == bits(quiet)).all() and (bits(busy_d) == bits(quiet)).all()
    for o, want in zip(outs, alone):
        assert (o.cpu().numpy() == want).all()


def test_errors_leave_the_context_usable():
    lib = abi.load()
    scene = ref.scene("spread")
    rays = ref.grid_rays((0.0, 0.0, 0.0, 1.0), (0.5, 0.5, 3.5), 10)
    out = np.zeros(10, np.float32)
    with abi.Context(0) as c:
        call = lambda layer, n, r, flags, o: lib.aic_sample_luminance(c._h, layer, n, r, 60, flags, o)
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, 0, out.ctypes.data) == ERR_INVALID  # no space yet
        c.upload_space(abi.LAYER_WORLD, scene.sp)
        assert call(abi.LAYER_UI, 10, rays.ctypes.data, 0, out.ctypes.data) == ERR_INVALID      # a layer without a space
        assert call(2, 10, rays.ctypes.data, 0, out.ctypes.data) == ERR_INVALID
        assert call(abi.LAYER_WORLD, (1 << 20) + 1, rays.ctypes.data, 0, out.ctypes.data) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, 1, out.ctypes.data) == ERR_INVALID    # unknown flag bits
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, abi.RAYS_DEVICE | 128, out.ctypes.data) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 10, None, 0, out.ctypes.data) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 10, rays.ctypes.data, 0, None) == ERR_INVALID
        assert call(abi.LAYER_WORLD, 0, None, 0, None) == abi.AIC_OK
        assert (out == 0).all()
        with pytest.raises(abi.AicError):
            c.sample_luminance(abi.LAYER_UI, rays, 60)
        # the context still samples and renders what it should
        got = c.sample_luminance(abi.LAYER_WORLD, rays, 60)
        assert (bits(got) == bits(scene.sample_all(rays, 60))).all()
        c.set_options(abi.LAYER_WORLD, abi.make_options())
        eye = (0.5, 0.5, 8.0)
        _, _, inv = oracle.camera_matrices(45.0, 200.0, W / HGT, oracle.look_at_y_up(eye, (0.0, 0.0, 0.0)), eye)
        frame = c.render(c.make_frame(W, HGT, world_inv=inv))["rgba8"]
        want = oracle.render(oracle.Space(scene.sp), oracle.make_options(), oracle.make_camera(inv, W, HGT), threads=4)["rgba8"]
        assert np.abs(frame.astype(int) - want.astype(int)).max() <= 1
