"""NumPy restatement of the presentation post-process (aic_present_split; DESIGN.md "Presentation"), for the tests.

A resident Split frame's colour plane -- [h][w][4] f16 bit patterns, premultiplied light times exposure and an alpha this pass never uses -- shown in a
window: the reference's frame copy with a linear ClampToEdge sampler (all-is-cubes-gpu raytrace_to_texture.rs:546-568, shaders/rt-copy.wgsl:41-71)
into the scene texture S, the dual-filter bloom chain on S (bloom.rs:41-60, mip_ping.rs:301-420: tests/bloom_ref.py's stages, from S instead of a
ColorBuf), and postprocess_fragment's mix, tone map and output conversion (shaders/postprocess.wgsl:140-158, 251-276). Every step is float32 in the
order DESIGN.md writes it; texels are rounded to float16 (nearest even, saturating at 65504) wherever the reference stores them.
"""
from __future__ import annotations

import numpy as np

from tests import bloom_ref

F = np.float32
ONE_F16 = 0x3C00


def texels(color_bits):
    """c: the three colour halves of every source texel as float32, saturated at 65504 (a Split frame stores overflow as infinity)."""
    bits = np.ascontiguousarray(color_bits, np.uint16)
    return np.minimum(bits[..., :3].view(np.float16).astype(F), F(65504.0))


def scene(color_bits, out_w: int, out_h: int):
    """S [out_h][out_w][4], float32 values of f16 texels, alpha 1.0: the texel itself at equal size, else the ClampToEdge bilinear read of c at the output
    pixel's centre, rounded to f16."""
    c = texels(color_bits)
    h, w = c.shape[:2]
    if (w, h) == (out_w, out_h):
        rgb = c
    else:
        u, v = bloom_ref._centres(out_w, out_h)
        rgb = bloom_ref.f16(bloom_ref.sample(c, u, v, mirror=False))
    return np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), F)], axis=-1)


def chain(s):
    """B = mip 0 after the whole bloom chain run on the scene texture `s`: bloom_ref.chain's stages, S given instead of made from a ColorBuf."""
    h, w = s.shape[:2]
    levels, (tx, ty) = bloom_ref.geometry(w, h)
    dims = [(tx >> k, ty >> k) for k in range(levels)]
    mips = [None] * levels
    for rep in range(bloom_ref.REPETITIONS):
        for k in range(levels):
            if rep and k == 0:
                continue
            mips[k] = bloom_ref.downsample(s if k == 0 else mips[k - 1], *dims[k])
        for k in range(levels - 2, -1, -1):
            mips[k] = bloom_ref.upsample(mips[k + 1], mips[k - 1] if k >= 1 else mips[1], k, *dims[k])
    return mips[0]


def composite(s, bloom, intensity, tone_mapping=0, maximum_intensity=np.inf, out_f16=False):
    """The image from S and (intensity > 0) B: x = s (1 - i) + b i with b the ClampToEdge read of B at the pixel's centre, the tone map, then sRGB8 with
    alpha byte 255 -- [h][w][4] uint8 -- or the saturating f16 of x with alpha 1.0 -- [h][w][4] uint16 bit patterns."""
    h, w = s.shape[:2]
    x = s[..., :3]
    i = F(intensity)
    if i > 0:
        u, v = bloom_ref._centres(w, h)
        b = bloom_ref.sample(bloom, u, v, mirror=False)[..., :3]
        x = x * (F(1.0) - i) + b * i
    x = bloom_ref.tone_map(x.astype(F), tone_mapping, maximum_intensity)
    if out_f16:
        out = np.empty((h, w, 4), np.uint16)
        out[..., :3] = bloom_ref.f16(x).astype(np.float16).view(np.uint16)
        out[..., 3] = ONE_F16
        return out
    return bloom_ref.encode(x, np.ones((h, w), F))


def present(color_bits, out_size, intensity, tone_mapping=0, maximum_intensity=np.inf, out_f16=False, parts=None):
    """aic_present_split of a frame's colour plane into an out_size = (width, height) window. `parts`, a dict, receives S and B (None at intensity 0)
    and supplies them when it already holds them: they depend on the frame and the sizes only."""
    parts = {} if parts is None else parts
    if "S" not in parts:
        parts["S"] = scene(color_bits, *out_size)
    if F(intensity) > 0 and parts.get("B") is None:
        parts["B"] = chain(parts["S"])
    return composite(parts["S"], parts.get("B"), intensity, tone_mapping, maximum_intensity, out_f16)
