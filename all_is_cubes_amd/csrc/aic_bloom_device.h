// aic_bloom_device.h -- what the kernels of the bloom chain (aic_bloom.hip) and of the presentation (aic_present.hip) share on the device: the f16
// texel, the address modes, the bilinear read with exact f32 weights and the two stages' texel functions. The bodies are aic_bloom.hip's own, moved
// here unchanged. Texel sources are types with `float4 at(int x, int y, int w) const`, so that every load names its address space.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_encode.h"

namespace aic {

AIC_DEV float f16_value(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
AIC_DEV uint32_t f16_bits(float x) {  // round to nearest even; saturating: at most 65504
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)fminf(x, 65504.0f));
}
AIC_DEV float4 unpack_texel(uint2 v) {
    return make_float4(f16_value(v.x & 0xffffu), f16_value(v.x >> 16), f16_value(v.y & 0xffffu), f16_value(v.y >> 16));
}
AIC_DEV uint2 pack_texel(float4 c) {
    return make_uint2(f16_bits(c.x) | (f16_bits(c.y) << 16), f16_bits(c.z) | (f16_bits(c.w) << 16));
}

AIC_DEV int wrap_mirror(int i, int n) {  // AddressMode::MirrorRepeat on texel indices: period 2n, reflected
    if ((uint32_t)i < (uint32_t)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m >= n ? p - 1 - m : m;
}
AIC_DEV int wrap_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }  // AddressMode::ClampToEdge

// The texel sources a stage reads. Each is a distinct type so that every load names its address space.
struct SrcScene {  // S, formed from the ColorBuf
    const float4 *__restrict__ cb;
    float e;
    AIC_DEV float4 at(int x, int y, int w) const {
        const float4 b = cb[(size_t)y * (uint32_t)w + (uint32_t)x];
        const float a = fminf(fmaxf(1.0f - b.w, 0.0f), 1.0f);
        return make_float4(f16_value(f16_bits(b.x * e)), f16_value(f16_bits(b.y * e)), f16_value(f16_bits(b.z * e)), f16_value(f16_bits(a)));
    }
};
struct SrcGlobal {
    const uint2 *__restrict__ p;
    AIC_DEV float4 at(int x, int y, int w) const { return unpack_texel(p[(uint32_t)y * (uint32_t)w + (uint32_t)x]); }
};

AIC_DEV float4 lerp2(float4 t00, float4 t10, float4 t01, float4 t11, float ax, float ay) {
    const float bx = 1.0f - ax, by = 1.0f - ay;
    float4 r;
    r.x = (t00.x * bx + t10.x * ax) * by + (t01.x * bx + t11.x * ax) * ay;
    r.y = (t00.y * bx + t10.y * ax) * by + (t01.y * bx + t11.y * ax) * ay;
    r.z = (t00.z * bx + t10.z * ax) * by + (t01.z * bx + t11.z * ax) * ay;
    r.w = (t00.w * bx + t10.w * ax) * by + (t01.w * bx + t11.w * ax) * ay;
    return r;
}

// textureSampleLevel(t, linear sampler, (u, v), 0) over a w x h texture, exact weights
template <bool MIRROR, class Src>
AIC_DEV float4 sample(const Src &s, int w, int h, float u, float v) {
    const float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    const float ax = x - fx, ay = y - fy;
    const int x0 = (int)fx, y0 = (int)fy;
    const int xa = MIRROR ? wrap_mirror(x0, w) : wrap_clamp(x0, w), xb = MIRROR ? wrap_mirror(x0 + 1, w) : wrap_clamp(x0 + 1, w);
    const int ya = MIRROR ? wrap_mirror(y0, h) : wrap_clamp(y0, h), yb = MIRROR ? wrap_mirror(y0 + 1, h) : wrap_clamp(y0 + 1, h);
    return lerp2(s.at(xa, ya, w), s.at(xb, ya, w), s.at(xa, yb, w), s.at(xb, yb, w), ax, ay);
}

AIC_DEV float4 f4_scale(float k, float4 a) { return make_float4(k * a.x, k * a.y, k * a.z, k * a.w); }
AIC_DEV float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// bloom_downsample (resampling.wgsl:90-98) at output texel (i, j) of an ow x oh mip, reading an iw x ih input: step = 2 / dims(input)
template <class Src>
AIC_DEV uint2 downsample_texel(const Src &s, int iw, int ih, int ow, int oh, int i, int j) {
    const float u = ((float)i + 0.5f) / (float)ow, v = ((float)j + 0.5f) / (float)oh;
    const float hx = 0.5f * (2.0f / (float)iw), hy = 0.5f * (2.0f / (float)ih);
    float4 r = f4_scale(0.50f, sample<true>(s, iw, ih, u, v));
    r = f4_add(r, f4_scale(0.125f, sample<true>(s, iw, ih, u + hx, v + hy)));
    r = f4_add(r, f4_scale(0.125f, sample<true>(s, iw, ih, u + hx, v - hy)));
    r = f4_add(r, f4_scale(0.125f, sample<true>(s, iw, ih, u - hx, v + hy)));
    r = f4_add(r, f4_scale(0.125f, sample<true>(s, iw, ih, u - hx, v - hy)));
    return pack_texel(r);
}

// bloom_upsample (resampling.wgsl:100-115) at output texel (i, j) of an ow x oh mip: I (iw x ih) is the mip below, H (hw x hh) the "higher" one;
// the step is 1 / dims(H) (resampling.wgsl:55-62), the weight of H is hwt = 5 * 1.5^-k
template <class SrcI, class SrcH>
AIC_DEV uint2 upsample_texel(const SrcI &I, int iw, int ih, const SrcH &H, int hw, int hh, float hwt, int ow, int oh, int i, int j) {
    const float u = ((float)i + 0.5f) / (float)ow, v = ((float)j + 0.5f) / (float)oh;
    const float sx = 1.0f / (float)hw, sy = 1.0f / (float)hh;
    const float hx = 0.5f * sx, hy = 0.5f * sy;
    float4 r = f4_scale(2.0f, sample<true>(I, iw, ih, u + hx, v + hy));
    r = f4_add(r, f4_scale(2.0f, sample<true>(I, iw, ih, u + hx, v - hy)));
    r = f4_add(r, f4_scale(2.0f, sample<true>(I, iw, ih, u - hx, v + hy)));
    r = f4_add(r, f4_scale(2.0f, sample<true>(I, iw, ih, u - hx, v - hy)));
    r = f4_add(r, sample<true>(I, iw, ih, u, v + sy));
    r = f4_add(r, sample<true>(I, iw, ih, u, v - sy));
    r = f4_add(r, sample<true>(I, iw, ih, u - sx, v));
    r = f4_add(r, sample<true>(I, iw, ih, u + sx, v));
    r = f4_add(r, f4_scale(hwt, sample<true>(H, hw, hh, u, v)));
    const float d = 12.0f + hwt;
    return pack_texel(make_float4(r.x / d, r.y / d, r.z / d, r.w / d));
}

inline uint32_t bloom_blocks_of(uint32_t n) { return (n + 255u) / 256u; }

}  // namespace aic
