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
#include "aic_bloom_device.h"
#include "aic_encode.h"

namespace aic {

namespace {

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

void launch_bloom_stages(const BloomGeom &g, uint2 *M, hipStream_t stream) {
    const uint32_t L = g.levels;
    auto mip = [&](uint32_t k) { return M + g.off[k]; };
    float hwt[kBloomMaxLevels];
    for (uint32_t k = 0; k < kBloomMaxLevels; k++) {  // resampling.wgsl:103: 5 * pow(1.5, -k)
        float q = 1.0f;
        for (uint32_t j = 0; j < k; j++) q = q / 1.5f;
        hwt[k] = 5.0f * q;
    }
    for (uint32_t rep = 0; rep < kBloomRepetitions; rep++) {
        // mip_ping.rs:301-420: downsample 0 .. L-1 (downsample 0 is the caller's: repetitions after the first keep mip 0), then upsample L-2 .. 0
        for (uint32_t k = 1u; k < L; k++)
            bloom_down_kernel<<<blocks_of(g.mw[k] * g.mh[k]), 256, 0, stream>>>(mip(k - 1), mip(k), (int)g.mw[k], (int)g.mh[k]);
        for (int k = (int)L - 2; k >= 0; k--) {
            const uint32_t hk = k >= 1 ? (uint32_t)k - 1u : 1u;  // mip_ping.rs:353: upsample 0 takes mip 1 as its "higher" input
            bloom_up_kernel<<<blocks_of(g.mw[k] * g.mh[k]), 256, 0, stream>>>(mip((uint32_t)k + 1u), mip(hk), (int)g.mw[hk], (int)g.mh[hk], hwt[k], mip((uint32_t)k),
                                                                                (int)g.mw[k], (int)g.mh[k]);
        }
    }
}

void launch_bloom(const BloomGeom &g, const BloomParams &p, hipStream_t stream) {
    if (!g.width || !g.height || !g.levels) return;
    bloom_down0_kernel<<<blocks_of(g.mw[0] * g.mh[0]), 256, 0, stream>>>(p.colorbuf, p.exposure, (int)g.width, (int)g.height, p.mips + g.off[0], (int)g.mw[0], (int)g.mh[0]);
    launch_bloom_stages(g, p.mips, stream);
    bloom_composite_kernel<<<blocks_of(g.width * g.height), 256, 0, stream>>>(p.colorbuf, p.mips + g.off[0], (int)g.width, (int)g.height, (int)g.mw[0], (int)g.mh[0], p.exposure,
                                                                           p.intensity, p.tone_mapping, p.maximum_intensity, p.srgb_thr, p.out);
}

}  // namespace aic
