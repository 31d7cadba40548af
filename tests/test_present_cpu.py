"""aic_present_split without a device: aic_present_geometry (host-only) against tests/bloom_ref.py's geometry, the ABI structs' sizes, and
tests/present_ref.py -- the NumPy restatement of DESIGN.md 4.11 -- on cases whose answer is known without it and against tests/bloom_ref.py on
opaque ColorBufs."""
import ctypes as C

import numpy as np
import pytest

from all_is_cubes_amd import abi
from tests import bloom_ref
from tests import present_ref as ref

F = np.float32
AIC_ERR_INVALID = 1


def bits(values):
    return np.asarray(values, np.float16).view(np.uint16)


def split_of(colorbuf, exposure):
    """The Split colour plane of an opaque ColorBuf: the f16 texels bloom_ref.scene makes, as bit patterns."""
    return bloom_ref.scene(colorbuf, exposure).astype(np.float16).view(np.uint16)


def random_opaque_colorbuf(w, h, seed):
    rng = np.random.default_rng(seed)
    cb = np.zeros((h, w, 4), F)
    light = rng.exponential(2.0, (h, w, 3)).astype(F)
    light[rng.random((h, w)) < 0.01] *= 1000.0  # bright, but below 65504 after the exposures used here: see the test
    cb[..., :3] = np.minimum(light, F(20000.0))
    return cb


@pytest.mark.parametrize("out", [(1, 1), (2, 2), (3, 5), (17, 9), (33, 20), (128, 256), (1920, 1080), (3840, 2160), (65535, 3), (65535, 32768)])
def test_geometry_is_the_bloom_chains_on_the_output_size(out):
    levels, t0 = bloom_ref.geometry(*out)
    n = out[0] * out[1]
    texels = sum((t0[0] >> k) * (t0[1] >> k) for k in range(levels))
    assert abi.present_geometry(out, out) == (levels, t0, texels * 8)
    assert abi.present_geometry((7, 3), out) == (levels, t0, (texels + n) * 8)  # a stretched frame: S is stored too
    assert abi.present_geometry((out[0], out[1] + 1 if out[1] < 65535 else 1), out) == (levels, t0, (texels + n) * 8)


def test_geometry_documented_figures_empty_outputs_and_rejections():
    assert abi.present_geometry((1920, 1080), (1920, 1080)) == (6, (960, 576), 5_896_800)
    assert abi.present_geometry((960, 540), (1920, 1080)) == (6, (960, 576), 22_485_600)
    assert abi.present_geometry((1, 1), (1, 1)) == (1, (2, 2), 32)
    for out in ((0, 5), (5, 0), (0, 0)):
        assert abi.present_geometry((4, 4), out) == (0, (0, 0), 0)
        assert abi.present_geometry((0, 0), out) == (0, (0, 0), 0)
    assert abi.present_geometry((65535, 65535), (32768, 65535))[0] == 6  # 2^31 - 32768 pixels
    bad = [((65536, 1), (4, 4)), ((1, 65536), (4, 4)), ((4, 4), (65536, 1)), ((4, 4), (1, 65536)),  # a dimension above 65535
           ((4, 4), (65535, 32769)), ((4, 4), (65535, 65535)),                                       # more than 2^31 output pixels
           ((0, 4), (4, 4)), ((4, 0), (4, 4)), ((0, 0), (1, 1))]                                     # nothing to fill the output from
    for src, out in bad:
        with pytest.raises(abi.AicError) as e:
            abi.present_geometry(src, out)
        assert e.value.code == AIC_ERR_INVALID, (src, out)
    lib = abi.load()  # any of the three may be NULL
    assert lib.aic_present_geometry(4, 4, 8, 8, None, None, None) == 0


def test_struct_sizes():
    assert C.sizeof(abi.PresentDesc) == 32
    assert C.sizeof(abi.PresentInfo) == 32
    assert abi.PRESENT_OUT_F16 == 1 and abi.PRESENT_MAX_PIXELS == 2 ** 31


@pytest.mark.parametrize("src,out", [((5, 4), (5, 4)), ((5, 4), (13, 9)), ((16, 12), (7, 5)), ((1, 1), (6, 3)), ((3, 7), (3, 8))])
def test_a_constant_frame_presents_as_that_constant(src, out):
    """Any size ratio, any intensity: bilinear weights sum to 1 and so do the chain's within an f32 rounding, far inside half an f16 ulp."""
    colour = np.array([0.3, 1.7, 12.25], np.float16)
    frame = np.zeros((src[1], src[0], 4), np.uint16)
    frame[..., :3] = colour.view(np.uint16)
    frame[..., 3] = np.random.default_rng(1).integers(0, 0x10000, (src[1], src[0]))  # alpha: anything
    for i in (0.0, 0.125, 0.5, 1.0):
        got = ref.present(frame, out, i, out_f16=True)
        assert got.shape == (out[1], out[0], 4)
        assert (got[..., :3] == colour.view(np.uint16)).all() and (got[..., 3] == ref.ONE_F16).all(), (src, out, i)
        rgba = ref.present(frame, out, i)
        want = bloom_ref.encode(colour.astype(F)[None, None, :], np.ones((1, 1), F))[0, 0]
        assert (rgba == want).all() and want[3] == 255


def test_equal_size_without_bloom_is_the_source_texel():
    rng = np.random.default_rng(7)
    w, h = 19, 11
    frame = np.abs(rng.standard_normal((h, w, 4)) * 30).astype(np.float16).view(np.uint16)
    frame[2, 3] = (0x7C00, 0x7BFF, 0x0001, 0xBC00)   # inf, 65504, the least subnormal; alpha -1
    frame[5, 0] = (0, 0, 0, 0xBC00)                  # the marker of an unfilled reprojection: black
    got = ref.present(frame, (w, h), 0.0, 0, np.inf, out_f16=True)
    want = frame.copy()
    want[..., 3] = ref.ONE_F16
    want[2, 3, 0] = 0x7BFF
    assert (got == want).all()
    assert (ref.present(frame, (w, h), 0.0)[5, 0] == (0, 0, 0, 255)).all()


def test_two_texels_stretched_to_four_by_hand():
    frame = np.zeros((1, 2, 4), np.uint16)
    frame[0, 0, :3] = bits([4.0, 0.0, 100.0])
    frame[0, 1, :3] = bits([0.0, 8.0, 100.0])
    got = ref.present(frame, (4, 1), 0.0, out_f16=True)[0].view(np.float16).astype(F)
    # sample points at -1/4, 1/4, 3/4, 5/4 texels from the first centre: the edge texel, 3/4 : 1/4, 1/4 : 3/4, the other edge texel
    assert (got == np.array([[4.0, 0.0, 100.0, 1.0], [3.0, 2.0, 100.0, 1.0], [1.0, 6.0, 100.0, 1.0], [0.0, 8.0, 100.0, 1.0]], F)).all()
    s = ref.scene(frame, 4, 1)
    assert s.shape == (1, 4, 4) and (s[0, 1, :2] == (F(4.0) * F(0.75), F(8.0) * F(0.25))).all()


@pytest.mark.parametrize("size", [(2, 2), (3, 5), (17, 9), (128, 96)])
def test_opaque_colorbufs_against_the_colorbuf_restatement(size):
    """t = 0 everywhere: S of the ColorBuf path is the Split texel, so B is bloom_ref.chain's bit for bit. The RGBA8 images differ only by the f16
    rounding of the scene term, which the ColorBuf composite takes in f32: at most 2^-12 relative, under 0.03 of an sRGB8 level, so at most one
    threshold is crossed. That holds below 65504 only -- above it a Split texel is saturated and the ColorBuf composite's scene term is not, which is
    a difference of the two formats, not of the arithmetic --, so the light here stays below it."""
    w, h = size
    cb = random_opaque_colorbuf(w, h, seed=31 * w + h)
    for exposure, tm, mi, i in [(1.0, 0, np.inf, 0.125), (2.5, 1, 1.0, 0.25), (0.75, 0, 2.0, 1.0)]:
        parts = {}
        got = ref.present(split_of(cb, exposure), size, i, tm, mi, parts=parts)
        want, b = bloom_ref.bloom_frame(cb, exposure, i, tm, mi)
        assert (parts["B"].view(np.uint32) == bloom_ref.chain(cb, exposure).view(np.uint32)).all() and (parts["B"] == b).all()
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"{w}x{h} e {exposure} tm {tm} max {mi} i {i}: RGBA8 exact {float((diff == 0).all(-1).mean()):.4f}")
        assert diff.max() <= 1, (size, exposure, tm, mi, i)
