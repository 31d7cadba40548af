"""NumPy restatement of the bloom post-process (AIC_FRAME_BLOOM; DESIGN.md "Bloom"), for the tests.

It follows the reference GPU renderer's dual-filter chain (all-is-cubes-gpu bloom.rs:41-60, mip_ping.rs:301-420 and :460-481,
shaders/resampling.wgsl:40-115) and the composite decided for this project: x = ps_mul(c, e) (1 - i) + (B / a) i in straight alpha, then the
raytracer's tone map and sRGB8 encode. Every step is float32 in the shaders' operation order; texels are rounded to float16 (nearest even,
saturating at 65504) wherever the reference stores them.
"""
from __future__ import annotations

import numpy as np

import oracle

F = np.float32
MAX_LEVELS, REPETITIONS = 6, 3


def geometry(width: int, height: int):
    """(L, (T0x, T0y)): R = (ceil(W/2), ceil(H/2)), L = min(6, ilog2(min(R)) + 1), T0 = R rounded up to a multiple of 2^L."""
    rx, ry = -(-width // 2), -(-height // 2)
    levels = min(MAX_LEVELS, int(np.floor(np.log2(min(rx, ry)))) + 1)
    d = 2 ** levels
    return levels, (-(-rx // d) * d, -(-ry // d) * d)


def f16(x):
    """f32 -> f16 -> f32: round to nearest even, saturating at 65504."""
    return np.minimum(np.asarray(x, F), F(65504.0)).astype(np.float16).astype(F)


def _mirror(i, n):
    p = 2 * n
    m = i % p
    return np.where(m >= n, p - 1 - m, m)


def _clamp(i, n):
    return np.clip(i, 0, n - 1)


def sample(tex, u, v, mirror=True):
    """Bilinear read of tex [h][w][4] at normalised (u, v) (texel centres at (i + 1/2) / size), exact float32 weights."""
    h, w = tex.shape[:2]
    x = u * F(w) - F(0.5)
    y = v * F(h) - F(0.5)
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = (x - fx)[..., None], (y - fy)[..., None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    wrap = _mirror if mirror else _clamp
    xa, xb, ya, yb = wrap(x0, w), wrap(x0 + 1, w), wrap(y0, h), wrap(y0 + 1, h)
    bx, by = F(1.0) - ax, F(1.0) - ay
    return (tex[ya, xa] * bx + tex[ya, xb] * ax) * by + (tex[yb, xa] * bx + tex[yb, xb] * ax) * ay


def _centres(ow, oh):
    u = (np.arange(ow, dtype=F) + F(0.5)) / F(ow)
    v = (np.arange(oh, dtype=F) + F(0.5)) / F(oh)
    return np.broadcast_to(u[None, :], (oh, ow)), np.broadcast_to(v[:, None], (oh, ow))


def downsample(inp, ow, oh):
    """bloom_downsample into an ow x oh mip: step = 2 / dims(input)."""
    ih, iw = inp.shape[:2]
    u, v = _centres(ow, oh)
    hx, hy = F(0.5) * (F(2.0) / F(iw)), F(0.5) * (F(2.0) / F(ih))
    r = (F(0.5) * sample(inp, u, v) + F(0.125) * sample(inp, u + hx, v + hy) + F(0.125) * sample(inp, u + hx, v - hy)
         + F(0.125) * sample(inp, u - hx, v + hy) + F(0.125) * sample(inp, u - hx, v - hy))
    return f16(r)


def higher_weight(k: int):
    q = F(1.0)
    for _ in range(k):
        q = F(q / F(1.5))
    return F(F(5.0) * q)


def upsample(lower, higher, k, ow, oh):
    """bloom_upsample into mip k (ow x oh) from mip k+1 (`lower`) and its "higher" input; step = 1 / dims(higher)."""
    hh, hw = higher.shape[:2]
    u, v = _centres(ow, oh)
    sx, sy = F(1.0) / F(hw), F(1.0) / F(hh)
    hx, hy = F(0.5) * sx, F(0.5) * sy
    wt = higher_weight(k)
    r = (F(2.0) * sample(lower, u + hx, v + hy) + F(2.0) * sample(lower, u + hx, v - hy) + F(2.0) * sample(lower, u - hx, v + hy)
         + F(2.0) * sample(lower, u - hx, v - hy) + sample(lower, u, v + sy) + sample(lower, u, v - sy) + sample(lower, u - sx, v)
         + sample(lower, u + sx, v) + wt * sample(higher, u, v))
    return f16(r / (F(12.0) + wt))


def scene(colorbuf, exposure):
    """S: ColorBuf::into_premultiplied_rgba times exposure, as f16 texels."""
    cb = np.asarray(colorbuf, F)
    e = F(exposure)
    a = np.minimum(np.maximum(F(1.0) - cb[..., 3], F(0.0)), F(1.0))
    return f16(np.concatenate([cb[..., :3] * e, a[..., None]], axis=-1))


def chain(colorbuf, exposure, stages=None):
    """The bloom image B = mip 0 after the whole chain, float32 values of f16 texels [T0y][T0x][4]. `stages`, a list, receives
    (name, mip index, copy of the mip) after every stage."""
    h, w = colorbuf.shape[:2]
    levels, (tx, ty) = geometry(w, h)
    dims = [(tx >> k, ty >> k) for k in range(levels)]
    s = scene(colorbuf, exposure)
    mips = [None] * levels
    for rep in range(REPETITIONS):
        for k in range(levels):
            if rep and k == 0:
                continue
            mips[k] = downsample(s if k == 0 else mips[k - 1], *dims[k])
            if stages is not None:
                stages.append(("down", k, mips[k].copy()))
        for k in range(levels - 2, -1, -1):
            mips[k] = upsample(mips[k + 1], mips[k - 1] if k >= 1 else mips[1], k, *dims[k])
            if stages is not None:
                stages.append(("up", k, mips[k].copy()))
    return mips[0]


def cb_to_rgba(colorbuf):
    """Rgba::from(ColorBuf) (raytracer_components.rs:122-147)."""
    cb = np.asarray(colorbuf, F)
    t = cb[..., 3]
    alpha = F(1.0) - t
    with np.errstate(divide="ignore", invalid="ignore"):
        c = cb[..., :3] / alpha[..., None]
    ok = (c >= 0).all(axis=-1)
    rgb = np.where(ok[..., None], np.maximum(c, F(0.0)), np.array([1.0, 0.0, 0.0], F))
    a = np.where((alpha > 0) & (alpha <= 1), alpha, np.where(alpha == 0, F(0.0), F(1.0)))
    out = np.concatenate([rgb, a[..., None]], axis=-1).astype(F)
    out[t >= 1.0] = 0.0
    return out


def ps_mul(a, b):
    with np.errstate(invalid="ignore"):
        return np.fmax(np.asarray(a, F) * F(b) if np.isscalar(b) else np.asarray(a, F) * b, F(0.0))


_THR = None


def srgb_thresholds():
    """thr[k] = the smallest f32 whose Rgba::to_srgb8 channel is >= k (k = 1..255), found with the oracle's encoder."""
    global _THR
    if _THR is None:
        def enc(x):
            return int(oracle.to_srgb8([x, 0.0, 0.0, 1.0])[0])
        thr = np.zeros(256, F)
        for k in range(1, 256):
            lo, hi = 0, 0x3F800000  # bit patterns of 0.0 and 1.0
            while lo < hi:
                mid = (lo + hi) // 2
                if enc(np.array(mid, np.uint32).view(F)) >= k:
                    hi = mid
                else:
                    lo = mid + 1
            thr[k] = np.array(lo, np.uint32).view(F)
        _THR = thr
    return _THR


def encode(rgb, a):
    """The raytracer's encoder after the tone map: sRGB8 channels by threshold count, alpha = (a * 255).round()."""
    thr = srgb_thresholds()[1:]
    with np.errstate(invalid="ignore"):
        pos = rgb > 0
    ch = np.where(pos, np.searchsorted(thr, np.where(pos, rgb, F(0.0)), side="right"), 0)
    ab = np.floor((a * F(255.0)).astype(np.float64) + 0.5)
    ab = np.clip(np.nan_to_num(ab, nan=0.0), 0, 255)
    return np.concatenate([ch, ab[..., None]], axis=-1).astype(np.uint8)


def tone_map(rgb, tone_mapping, m):
    """ToneMappingOperator::apply (graphics_options.rs:352-368) as the trace kernels apply it."""
    m = F(m)
    if not np.isfinite(m):
        return rgb
    if tone_mapping == 0:
        return np.clip(rgb, F(0.0), m)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    lum = g * F(0.7152) + (r * F(0.2126) + b * F(0.0722))
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = F(1.0) / (F(1.0) + lum / m)
    scale = np.where(scale > 0, scale, F(0.0)).astype(F)
    return ps_mul(rgb, scale[..., None])


def composite(colorbuf, bloom, exposure, intensity, tone_mapping=0, maximum_intensity=np.inf):
    """RGBA8 of the frame with B mixed in: x = ps_mul(c, e) (1 - i) + (B / a) i, a = 0 unchanged; then tone map and encode."""
    h, w = colorbuf.shape[:2]
    c = cb_to_rgba(colorbuf)
    rgb = ps_mul(c[..., :3], F(exposure))
    a = c[..., 3]
    u = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    v = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    B = sample(bloom, np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w)), mirror=False)
    i = F(intensity)
    with np.errstate(divide="ignore", invalid="ignore"):
        mixed = rgb * (F(1.0) - i) + (B[..., :3] / a[..., None]) * i
    rgb = np.where((a > 0)[..., None], mixed, rgb).astype(F)
    return encode(tone_map(rgb, tone_mapping, maximum_intensity), a)


def bloom_frame(colorbuf, exposure, intensity, tone_mapping=0, maximum_intensity=np.inf):
    """(RGBA8, mip 0) of the whole post-process."""
    b = chain(colorbuf, exposure)
    return composite(colorbuf, b, exposure, intensity, tone_mapping, maximum_intensity), b
