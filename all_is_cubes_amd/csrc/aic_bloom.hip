// aic_bloom.hip -- the bloom post-process on gfx950: the reference GPU renderer's dual-filter mip chain and its mix into the scene, applied to a
// traced frame's ColorBuf (aic_bloom.h; DESIGN.md "Bloom").
//
//  * S, the scene texture (the reference's Rgba16Float, raytrace_to_texture.rs:644-661), is never stored: downsample 0 reads the ColorBuf and
//    forms S's texels, (l0 e, l1 e, l2 e, clamp(1 - t, 0, 1)) rounded to f16 (ColorBuf::into_premultiplied_rgba times exposure), where it samples them.
//  * Every mip is f16 x 4 (8 bytes a texel). f32 -> f16 rounds to nearest even and saturates at 65504 (the reference would store inf and its
//    Reinhard step would make NaN of it); the round-toward-zero pack instruction is not used.
//  * Sampling: normalised coordinates over the texture read, texel centres at (i + 1/2) / size, bilinear with exact f32 weights; MirrorRepeat in
//    the chain, ClampToEdge for the composite's read of mip 0. f32 arithmetic in the shaders' operation order, under -ffp-contract=off.
//  * Launches: one grid per stage of the chain, a texel per thread, in the reference's stage order; then the composite. (A single workgroup that kept
//    the small mips in LDS and ran their stages behind barriers was measured slower than the launches it saved: DESIGN.md §4.7.)
//  * Composite, in straight alpha: x = ps_mul(c, e) (1 - i) + (B / a) i per channel, with c, a = Rgba::from(ColorBuf) (cb_to_rgba), then the
//    trace kernels' own tone map, sRGB8 encode and alpha byte (aic_encode.h). A pixel with a = 0 is left as the trace encodes it.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_bloom.h"
#include "aic_encode.h"

namespace aic {

namespace {

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

// One stage over a whole mip, a texel per thread.
__global__ void __launch_bounds__(256) bloom_down0_kernel(const float4 *__restrict__ cb, float e, int sw, int sh, uint2 *__restrict__ out, int ow, int oh) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)(ow * oh)) return;
    const SrcScene s{cb, e};
    out[t] = downsample_texel(s, sw, sh, ow, oh, (int)(t % (uint32_t)ow), (int)(t / (uint32_t)ow));
}
__global__ void __launch_bounds__(256) bloom_down_kernel(const uint2 *__restrict__ in, uint2 *__restrict__ out, int ow, int oh) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)(ow * oh)) return;
    const SrcGlobal s{in};
    out[t] = downsample_texel(s, 2 * ow, 2 * oh, ow, oh, (int)(t % (uint32_t)ow), (int)(t / (uint32_t)ow));
}
__global__ void __launch_bounds__(256) bloom_up_kernel(const uint2 *__restrict__ lower, const uint2 *__restrict__ higher, int hw, int hh, float hwt,
                                                       uint2 *__restrict__ out, int ow, int oh) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)(ow * oh)) return;
    const SrcGlobal I{lower}, H{higher};
    out[t] = upsample_texel(I, ow / 2, oh / 2, H, hw, hh, hwt, ow, oh, (int)(t % (uint32_t)ow), (int)(t / (uint32_t)ow));
}

// mix(scene, B, i) in straight alpha, then the trace's encoder (aic_trace.hip, the end of a pixel's last sample)
__global__ void __launch_bounds__(256) bloom_composite_kernel(const float4 *__restrict__ cb, const uint2 *__restrict__ mip0, int w, int h, int t0x, int t0y,
                                                              float ex, float intensity, int32_t tone_mapping, float m, const float *__restrict__ thr,
                                                              uint32_t *__restrict__ out) {
    __shared__ float s_thr[kSrgbWindowWords];
    srgb_window_to_lds(s_thr, thr, threadIdx.x, 256u);
    __syncthreads();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    const uint32_t pix = t < npix ? t : npix - 1u;  // (every lane of the wave runs cb_to_rgba's ballot; only the real pixels store)
    const float4 b4 = cb[pix];
    ColorBuf pixel;
    pixel.l0 = b4.x; pixel.l1 = b4.y; pixel.l2 = b4.z; pixel.t = b4.w;
    float c[4];
    cb_to_rgba(pixel, c);
    float r = ps_mul(c[0], ex), g = ps_mul(c[1], ex), bl = ps_mul(c[2], ex);
    const float a = c[3];
    if (a > 0.f) {
        const int x = (int)(pix % (uint32_t)w), y = (int)(pix / (uint32_t)w);
        const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)h;
        const float4 B = sample<false>(SrcGlobal{mip0}, t0x, t0y, u, v);
        const float keep = 1.0f - intensity;
        r = r * keep + (B.x / a) * intensity;
        g = g * keep + (B.y / a) * intensity;
        bl = bl * keep + (B.z / a) * intensity;
    }
    if (isfinite(m)) {  // ToneMappingOperator::apply (graphics_options.rs:352-368), as the trace kernels apply it
        if (tone_mapping == 0) {
            r = r < 0.f ? 0.f : (r > m ? m : r);
            g = g < 0.f ? 0.f : (g > m ? m : g);
            bl = bl < 0.f ? 0.f : (bl > m ? m : bl);
        } else {
            const float scale = ps_clamped(1.0f / (1.0f + luminance(r, g, bl) / m));
            r = ps_mul(r, scale); g = ps_mul(g, scale); bl = ps_mul(bl, scale);
        }
    }
    uint32_t R, G, B;
    srgb8_rgb(r, g, bl, s_thr, R, G, B);
    const uint32_t A = round_sat_u8(c[3] * 255.0f);
    if (t < npix) out[t] = R | (G << 8) | (B << 16) | (A << 24);
}

uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }

}  // namespace

void launch_bloom(const BloomGeom &g, const BloomParams &p, hipStream_t stream) {
    const uint32_t L = g.levels;
    if (!g.width || !g.height || !L) return;
    uint2 *const M = p.mips;
    auto mip = [&](uint32_t k) { return M + g.off[k]; };
    float hwt[kBloomMaxLevels];
    for (uint32_t k = 0; k < kBloomMaxLevels; k++) {  // resampling.wgsl:103: 5 * pow(1.5, -k)
        float q = 1.0f;
        for (uint32_t j = 0; j < k; j++) q = q / 1.5f;
        hwt[k] = 5.0f * q;
    }
    for (uint32_t rep = 0; rep < kBloomRepetitions; rep++) {
        // mip_ping.rs:301-420: downsample 0 .. L-1 (repetitions after the first keep mip 0), then upsample L-2 .. 0
        for (uint32_t k = rep == 0 ? 0u : 1u; k < L; k++) {
            const int ow = (int)g.mw[k], oh = (int)g.mh[k];
            if (k == 0) bloom_down0_kernel<<<blocks_of(g.mw[0] * g.mh[0]), 256, 0, stream>>>(p.colorbuf, p.exposure, (int)g.width, (int)g.height, mip(0), ow, oh);
            else bloom_down_kernel<<<blocks_of(g.mw[k] * g.mh[k]), 256, 0, stream>>>(mip(k - 1), mip(k), ow, oh);
        }
        for (int k = (int)L - 2; k >= 0; k--) {
            const uint32_t hk = k >= 1 ? (uint32_t)k - 1u : 1u;  // mip_ping.rs:353: upsample 0 takes mip 1 as its "higher" input
            bloom_up_kernel<<<blocks_of(g.mw[k] * g.mh[k]), 256, 0, stream>>>(mip((uint32_t)k + 1u), mip(hk), (int)g.mw[hk], (int)g.mh[hk], hwt[k], mip((uint32_t)k),
                                                                                (int)g.mw[k], (int)g.mh[k]);
        }
    }
    bloom_composite_kernel<<<blocks_of(g.width * g.height), 256, 0, stream>>>(p.colorbuf, mip(0), (int)g.width, (int)g.height, (int)g.mw[0], (int)g.mh[0], p.exposure,
                                                                           p.intensity, p.tone_mapping, p.maximum_intensity, p.srgb_thr, p.out);
}

}  // namespace aic
