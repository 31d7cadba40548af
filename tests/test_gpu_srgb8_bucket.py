"""The trace kernels encode sRGB8 from the context's bucket table (aic_encode.h srgb8_bucket_channel, read with global loads in FINISH): whole frames whose
channels are spread over the table by the exposure -- dark (0.25), plain (1) and mostly clamped at 1.0 (8) -- under both tone-mapping operators must be the
oracle's RGBA8 byte for byte, on the recording and the production variants. tests/test_srgb8_bucket_host.py checks the table itself for every bit pattern."""
import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi
from all_is_cubes_amd import workloads as scenes

pytestmark = pytest.mark.gpu

W, H = 96, 64
EYE = (12.5, 20.5, 40.0)


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene():
    space = scenes.synthetic_space(n=24, resolution=8, n_blocks=8, seed=3)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, W / H, oracle.look_at_y_up(EYE, (12.0, 8.0, 12.0)), EYE)
    return space, oracle.Space(space), inv


@pytest.mark.parametrize("tone_mapping", [0, 1], ids=["clamp", "reinhard"])
@pytest.mark.parametrize("exposure", [0.25, 1.0, 8.0])
def test_frame_equals_oracle_rgba8(ctx, scene, exposure, tone_mapping):
    space, ospace, inv = scene
    ctx.upload_space(abi.LAYER_WORLD, space)
    ctx.clear_space(abi.LAYER_UI)
    ctx.set_options(abi.LAYER_WORLD, abi.make_options(tone_mapping=tone_mapping, maximum_intensity=2.0, bloom_intensity=0.0))
    frame = ctx.make_frame(W, H, world_inv=inv, exposure=exposure)
    recorded = ctx.render(frame, want_aux=True)["rgba8"]
    plain = ctx.render(frame)["rgba8"]
    frame.tuning |= abi.tuning(variant=abi.VARIANT_EXCHANGING)
    exchanging = ctx.render(frame)["rgba8"]
    opt = oracle.make_options(tone_mapping=tone_mapping, maximum_intensity=2.0, exposure=exposure)
    ref = oracle.render(ospace, opt, oracle.make_camera(inv, W, H))["rgba8"]
    for name, got in (("recording", recorded), ("plain", plain), ("exchanging", exchanging)):
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        print(f"exposure {exposure} tone mapping {tone_mapping} {name}: max difference {int(d.max())}, pixels that differ {int(d.any(axis=-1).sum())}")
        assert (got == ref).all(), name
    assert len(np.unique(ref[..., :3])) > (20 if exposure == 8.0 else 60)  # the frame really spreads over the table
