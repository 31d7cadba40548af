"""Automatic exposure without a GPU: the reference's known answers, the host-only entry points (aic_exposure_init / _rays / _advance) against the
restatement in tests/exposure_ref.py bit for bit, the four names in every layer, and that the case list the GPU test runs reaches every outcome of the
sampler. The sampler itself runs in tests/test_gpu_exposure.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import exposure_ref as ref

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("aic_exposure_init", "aic_exposure_rays", "aic_sample_luminance", "aic_exposure_advance")
f32 = np.float32
ERR_INVALID = 1  # AIC_ERR_INVALID


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the reference's known answers (exposure.rs:169-174) -------------------------------------------------------------

LUMINANCES = [0.0, 0.01, 0.5, 1.0, 2.0, 100.0, 1000.0]
TARGETS = np.array([2.125, 2.125, 1.3, 0.9625, 0.79375, 0.6625, 0.6625], np.float32)


def test_target_exposure_known_answers():
    assert (bits([ref.compute_target_exposure(l) for l in LUMINANCES]) == bits(TARGETS)).all()
    assert (bits([H.ExposureState.compute_target_exposure(l) for l in LUMINANCES]) == bits(TARGETS)).all()
    # ... and through the boundary: with the ring full of one luminance a step of dt = 0.5 (dt * rate = 1) takes the log from 0 to ln(target) exactly
    for l, t in zip(LUMINANCES, TARGETS):
        s = abi.ExposureState()
        s.advance(np.full(100, l, np.float32), 0.5)
        if l in (0.0, 0.5, 1.0, 2.0):  # (sums of 100 equal samples that come out exact, so that the average is l itself)
            assert bits(s.exposure_log) == bits(f32(np.log(np.float64(t)))), (l, t)
        assert abs(float(s.exposure()) / float(t) - 1.0) < 1e-5, (l, t)


def test_luminance_known_answer():
    assert ref.luminance(3, 3, 3) == f32(3.0)
    assert ref.luminance(1, 0, 0) == f32(0.2126) and ref.luminance(0, 1, 0) == f32(0.7152) and ref.luminance(0, 0, 1) == f32(0.0722)


# ---- aic_exposure_advance --------------------------------------------------------------------------------------------

def same_state(got: abi.ExposureState, want: ref.State):
    assert (bits(got.samples) == bits(want.samples)).all()
    assert got.index == want.index
    assert bits(got.exposure_log) == bits(want.exposure_log)


def test_advance_matches_the_restatement_bit_for_bit():
    rng = np.random.default_rng(11)
    got, want = abi.ExposureState(), ref.State()
    same_state(got, want)
    assert got.exposure() == f32(1.0)
    specials = [np.zeros(10, np.float32), np.full(100, 0.0, np.float32), np.array([np.inf], np.float32), np.array([np.nan, 1.0], np.float32),
                np.full(100, 1e-30, np.float32), np.full(100, 3e38, np.float32)]
    for step in range(400):
        n = int(rng.choice([0, 1, 10, 10, 10, 37, 100]))
        smp = (rng.uniform(0.0, 4.0, n) ** 3).astype(np.float32)
        if step % 23 == 5:
            smp = specials[(step // 23) % len(specials)]
        dt = float(rng.choice([0.0, 0.1, 1.0 / 60.0, 0.25, float(rng.uniform(0.0, 0.4))]))
        e_got, e_want = got.advance(smp, dt), want.advance(smp, dt)
        same_state(got, want)
        assert bits(e_got) == bits(e_want), (step, n, dt)
        if step % 23 == 16:  # (flush what a special left in the ring)
            flush = rng.uniform(0.1, 2.0, 100).astype(np.float32)
            got.advance(flush, 0.1), want.advance(flush, 0.1)
    assert np.isfinite(got.exposure_log)


def test_advance_dt_zero_changes_nothing():
    s = abi.ExposureState()
    s.advance(np.linspace(0.1, 2.0, 10), 0.1)
    before = (s.samples.copy(), s.index, s.exposure_log)
    e = s.advance(np.full(10, 7.0, np.float32), 0.0)
    assert (bits(s.samples) == bits(before[0])).all() and s.index == before[1] and bits(s.exposure_log) == bits(before[2])
    assert bits(e) == bits(s.exposure())


def test_advance_zero_luminance_clamps_to_four():
    s = abi.ExposureState()
    s.advance(np.zeros(100, np.float32), 0.5)  # (dt * rate = 1: the log lands on ln(target))
    assert bits(s.exposure_log) == bits(f32(np.log(np.float64(f32(4.0) * f32(0.375) + f32(0.625)))))
    assert s.exposure() == f32(np.exp(np.float64(s.exposure_log)))


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_advance_non_finite_samples_leave_the_log_alone(bad):
    s = abi.ExposureState()
    s.advance(np.full(10, 0.2, np.float32), 0.1)
    log_before = s.exposure_log
    if np.isinf(bad):
        # inf in the ring: the average is inf, 0.9 / inf = 0 clamps to 0.1 -- a finite target. A non-finite one needs the sum to be NaN
        s.advance(np.array([np.inf, -np.inf], np.float32), 0.1)
    else:
        s.advance(np.array([np.nan], np.float32), 0.1)
    assert not np.isfinite(ref.compute_target_exposure(ref_state_of(s).luminance_average()))
    assert bits(s.exposure_log) == bits(log_before)
    assert s.index == (12 if np.isinf(bad) else 11)


def ref_state_of(s: abi.ExposureState) -> ref.State:
    r = ref.State()
    r.samples, r.index, r.exposure_log = s.samples.copy(), s.index, s.exposure_log
    return r


def test_advance_ring_wraps_and_ends_on_the_last_sample_written():
    s = abi.ExposureState()
    s.advance(np.arange(1, 96, dtype=np.float32), 0.1)
    assert s.index == 95
    s.advance(np.arange(200, 210, dtype=np.float32), 0.1)
    assert s.index == 5
    assert (s.samples[96:100] == [200, 201, 202, 203]).all() and (s.samples[0:6] == [204, 205, 206, 207, 208, 209]).all()
    assert s.samples[6] == 6.0
    s.advance(np.arange(300, 400, dtype=np.float32), 0.1)  # n = 100: the whole ring, starting behind the index
    assert s.index == 5 and s.samples[6] == 300.0 and s.samples[5] == 399.0
    s.advance([], 0.1)
    assert s.index == 5


def test_advance_and_rays_reject_bad_arguments():
    lib = abi.load()
    s = abi.ExposureState()
    smp = np.zeros(101, np.float32)
    assert lib.aic_exposure_advance(C.byref(s.c), 101, smp.ctypes.data, 0.1, None) == ERR_INVALID
    assert lib.aic_exposure_advance(None, 0, None, 0.1, None) == ERR_INVALID
    assert lib.aic_exposure_advance(C.byref(s.c), 3, None, 0.1, None) == ERR_INVALID
    assert lib.aic_exposure_advance(C.byref(s.c), 0, None, 0.1, None) == abi.AIC_OK
    assert lib.aic_exposure_init(None) == ERR_INVALID
    abi.exposure_rays((0, 0, 0, 1), (0, 0, 0), 0, 0)
    q = (C.c_double * 4)(0, 0, 0, 1)
    assert lib.aic_exposure_rays(q, None, 0, 0, None) == ERR_INVALID
    assert lib.aic_exposure_rays(q, (C.c_double * 3)(), 0, 1, None) == ERR_INVALID


# ---- aic_exposure_rays -----------------------------------------------------------------------------------------------

def unit_quaternions(n: int, seed: int):
    q = np.random.default_rng(seed).normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def test_rays_match_the_restatement_bit_for_bit():
    rng = np.random.default_rng(3)
    views = [((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, 0.0, 1.0), (5.0, 5.0, 5.0)), (ref.HALF_TURN_Y, (0.5, 0.5, -6.0))]
    for eye, target in (((6.0, 7.0, 3.2), (-2.0, 2.0, 0.0)), ((0.0, 10.0, 0.0), (0.4, 10.0, -1.0)), ((-3.5, 2.25, 9.0), (100.0, -50.0, 0.125))):
        views.append((tuple(oracle.look_at_y_up(eye, target)), eye))
    for q in unit_quaternions(12, 4):
        views.append((tuple(q), tuple(rng.uniform(-1e3, 1e3, 3))))
    views.append(((0.3, -0.2, 0.9, 0.1), (-0.0, 1e-300, 1e300)))  # not a unit quaternion: the arithmetic is the same
    for q, t in views:
        for first, n in ((0, 100), (95, 10), (99, 1), (7, 10), (250, 30), (2 ** 32 - 3, 10)):
            got, want = abi.exposure_rays(q, t, first, n), ref.exposure_rays(q, t, first, n)
            assert got.shape == (n, 6)
            assert (bits64(got) == bits64(want)).all(), (q, t, first, n)


def test_rays_of_the_identity():
    r = abi.exposure_rays((0, 0, 0, 1), (1.5, -2.0, 3.0), 0, 100)
    assert (r[:, :3] == (1.5, -2.0, 3.0)).all() and (r[:, 5] == -1.0).all()
    assert bits64(r[5, 3]) == bits64(0.0)  # index 5: 5 / 10 * 2 - 1 is exactly +0.0
    assert r[0, 3] == -1.0 and r[0, 4] == -1.0 and r[99, 3] == 0.8 and r[99, 4] == 0.8
    assert (r[10:20, 4] == r[10, 4]).all() and r[10, 4] == 0.1 * 2 - 1
    wrapped = abi.exposure_rays((0, 0, 0, 1), (1.5, -2.0, 3.0), 95, 10)
    assert (bits64(wrapped) == bits64(np.concatenate([r[95:], r[:5]]))).all()


# ---- every layer -----------------------------------------------------------------------------------------------------

def test_the_entry_points_exist_in_every_layer():
    header = (ROOT / "include" / "aic_hip.h").read_text()
    ffi = (ROOT / "rust" / "all-is-cubes-hip" / "src" / "ffi.rs").read_text()
    shim = (ROOT / "rust" / "all-is-cubes-hip" / "src" / "lib.rs").read_text()
    lib = abi.load()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
        assert f"pub fn {name}(" in ffi, name
    assert "typedef struct aic_exposure_state" in header and "pub struct aic_exposure_state" in ffi
    assert "#define AIC_EXPOSURE_SAMPLES 100" in header and "#define AIC_EXPOSURE_RAYS 10" in header
    assert C.sizeof(abi.ExposureStateC) == 408
    assert "pub fn sample_luminance(" in shim and "pub struct ExposureState" in shim
    for attr in ("step", "exposure", "luminance_average", "samples", "compute_target_exposure"):
        assert hasattr(H.ExposureState, attr), attr
    assert hasattr(H.HipRtRenderer, "sample_luminance") and hasattr(abi.Context, "sample_luminance") and hasattr(abi.Context, "sample_luminance_device")
    s = H.ExposureState()
    assert s.exposure() == 1.0 and s.luminance_average() == 1.0 and (s.samples() == 1.0).all() and s.sample_index == 0


def test_sampling_without_a_gpu_fails_loudly():
    """No device, no samples: nothing falls back to the CPU."""
    import torch

    lib = abi.load()
    rays = np.zeros((1, 6))
    out = np.zeros(1, np.float32)
    assert lib.aic_sample_luminance(None, 0, 1, rays.ctypes.data, 60, 0, out.ctypes.data) == ERR_INVALID
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(abi.AicError):
        abi.Context(0).sample_luminance(abi.LAYER_WORLD, rays, 60)
    with pytest.raises(Exception):
        H.ExposureState().step(H.HipRtRenderer(H.StandardCameras()), H.ViewTransform.identity(), 30, 0.1)


# ---- the case list of the GPU test -----------------------------------------------------------------------------------

def test_case_list_reaches_every_outcome():
    seen = {}
    for name, key, rays, max_steps in ref.cases():
        o = set()
        ref.scene(key).sample_all(rays, max_steps, o)
        seen[name] = o
    everything = set().union(*seen.values())
    for outcome in (ref.SKY_NO_STEPS, ref.SKY_STEP_LIMIT, ref.SKY_LEFT_BOUNDS, ref.LIT_INSIDE, ref.LIT_OUTSIDE, ref.PASSED):
        assert outcome in everything, outcome
    # the cases the issue names reach what it says they reach
    assert seen["spread eye(0.5,0.5,3.5) steps 0"] == {ref.SKY_NO_STEPS}
    assert seen["spread eye(0.5,0.5,3.5) steps 3"] == {ref.SKY_STEP_LIMIT}
    assert ref.LIT_INSIDE in seen["spread eye(0.5,0.5,3.5) steps 60"]
    assert {ref.PASSED, ref.SKY_LEFT_BOUNDS} <= seen["spread inside a pillar"]
    assert ref.LIT_OUTSIDE in seen["spread from outside, along +Z"]
    both = seen["cornell from its centre"] | seen["cornell from 30 cubes in front"]
    assert {ref.LIT_INSIDE, ref.PASSED, ref.SKY_LEFT_BOUNDS} <= both


def test_an_invisible_voxel_block_is_passed_through():
    sc = ref.scene("ghost")
    sp = sc.sp
    ghost, lamp = int(sp.block_index[0, 0, 2]), int(sp.block_index[0, 0, 1])
    assert sp.blocks[ghost].resolution == 2 and not sc.visible[ghost] and sc.visible[lamp]  # recursive by class, invisible by evaluation
    down = [0.5, 0.5, 4.5, 0.0, 0.0, -1.0]
    behind_lamp, behind_ghost = sp.light[0, 0, 2], sp.light[0, 0, 3]
    want = ref.luminance(*[sc.lut[int(v)] for v in behind_lamp[:3]])
    stop_at_class_bits = ref.luminance(*[sc.lut[int(v)] for v in behind_ghost[:3]])
    assert want != stop_at_class_bits
    assert sc.sample(down, 60) == want
    # through the other ghost, at (1, 1, 2), to the wall: the texel in front of the wall
    assert sc.sample([1.5, 1.5, 4.5, 0.0, 0.0, -1.0], 60) == ref.luminance(*[sc.lut[int(v)] for v in sp.light[1, 1, 1][:3]])


def test_an_empty_space_samples_its_octant_sky():
    sc = ref.scene("empty")
    for d in ((1.0, 1.0, 1.0), (-1.0, 2.0, -3.0), (-0.0, -0.0, -0.0), (np.nan, 1.0, -1.0), (0.0, 0.0, 0.0)):
        o = (int(d[0] >= 0) << 2) + (int(d[1] >= 0) << 1) + int(d[2] >= 0)
        c = sc.sp.sky[o]
        for ms in (0, 60):
            assert sc.sample([0.1, 0.2, 0.3, *d], ms) == ref.luminance(c[0], c[1], c[2]), (d, ms)
    assert bits(sc.sample([0, 0, 0, np.nan, np.nan, np.nan], 60)) == bits(ref.luminance(*sc.sp.sky[0]))


def test_host_half_under_sanitizers_as_a_stand_alone_program(tmp_path):
    """csrc/aic_exposure_state.cpp and tests/native/exposure_state_check.cpp (its own main) built with AddressSanitizer and UBSan and run on the CPU:
    exact-size heap buffers for the state, the rays and the samples, every n, wrapping first indices. Nothing is loaded into Python."""
    import subprocess

    exe = tmp_path / "exposure_state_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    str(ROOT / "tests" / "native" / "exposure_state_check.cpp"), str(ROOT / "all_is_cubes_amd" / "csrc" / "aic_exposure_state.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("exposure state ok"), run.stdout + run.stderr
