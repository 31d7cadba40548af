// aic_present.hip -- presentation of a resident Split frame on gfx950 (aic_present_split; aic_bloom.h, DESIGN.md "Presentation"): what the reference's
// incremental raytracer does with its resident textures every displayed frame.
//
//  * The frame's f16 colour texels, saturated at 65504 and with alpha 1, ARE the scene texture S when the window has the frame's size, and the
//    ClampToEdge bilinear stretch of them, rounded to f16, when it has not (raytrace_to_texture.rs:546-568, shaders/rt-copy.wgsl:41-71).
//  * The bloom chain runs from that S: downsample 0 through SrcSplit here, every later stage by the chain's own kernels. The composite
//    x = s (1 - i) + B i needs no division: alpha is 1 everywhere (postprocess.wgsl:140-158).
//  * S is stored only for a stretched AND bloomed frame (downsample 0 reads each of its texels five times over); otherwise the composite forms it
//    where it reads it. The bits are the same either way.
//  * The info text (aic_present_split_text; postprocess.wgsl:160-276, DESIGN.md "The info text in a presentation") is a variant of the composite: the
//    four nearest cells of a grid of character codes are looked up in the resident font atlas and their maximum is laid over the tone-mapped scene.
//    Codes are byte loads, atlas texels dword loads; lanes outside the rectangle the host found in the text's reach skip the lookups.
//  * Everything else -- the f16 texel, the sampler, the chain's stages from mip 1 on, the tone map and the encoder -- is the bloom post-process's own
//    (aic_bloom_device.h, launch_bloom_stages, aic_encode.h). A texel per lane, 256-thread workgroups, one 8-byte load or store per colour texel.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_bloom.h"
#include "aic_bloom_device.h"
#include "aic_encode.h"
#include "aic_split_texel.h"

namespace aic {

namespace {

// A resident Split frame's colour plane as the scene texture reads it (rt_frame_copy_fragment, rt-copy.wgsl:56-71: alpha discarded, 1.0 written):
// colour saturated at 65504 (a Split frame stores overflow as infinity; the chain's convention is saturation, and inf x 0 weights would make NaN).
// The alpha half travels in the 8-byte load and is dropped; the depth plane is never addressed.
struct SrcSplit {
    const uint2 *__restrict__ p;
    AIC_DEV float4 at(int x, int y, int w) const {
        const uint2 v = p[(uint32_t)y * (uint32_t)w + (uint32_t)x];
        return make_float4(fminf(f16_value(v.x & 0xffffu), 65504.0f), fminf(f16_value(v.x >> 16), 65504.0f), fminf(f16_value(v.y & 0xffffu), 65504.0f), 1.0f);
    }
};

// S(x, y) of an ow x oh window stretched from an sw x sh Split frame: the linear ClampToEdge sampler of the frame-copy pipeline at the window pixel's
// centre, stored as the Rgba16Float scene texture stores it
AIC_DEV uint2 stretch_texel(const SrcSplit &s, int sw, int sh, int ow, int oh, int x, int y) {
    const float u = ((float)x + 0.5f) / (float)ow, v = ((float)y + 0.5f) / (float)oh;
    float4 r = sample<false>(s, sw, sh, u, v);
    r.w = 1.0f;
    return pack_texel(r);
}
// the scene texel a composite or an export reads at (x, y) of a w x h window: formed from an sw x sh frame (STRETCH), or the frame's own texel
template <bool STRETCH>
AIC_DEV float4 scene_at(const SrcSplit &s, int sw, int sh, int w, int h, int x, int y) {
    return STRETCH ? unpack_texel(stretch_texel(s, sw, sh, w, h, x, y)) : s.at(x, y, w);
}
__global__ void __launch_bounds__(256) present_stretch_kernel(const uint2 *__restrict__ src, int sw, int sh, uint2 *__restrict__ out, int ow, int oh) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)ow * (uint32_t)oh) return;
    out[t] = stretch_texel(SrcSplit{src}, sw, sh, ow, oh, (int)(t % (uint32_t)ow), (int)(t / (uint32_t)ow));
}
// S of a window of the frame's own size, stored: the source texel itself, saturated, alpha 1 (what SrcSplit reads, as the scene texture holds it)
__global__ void __launch_bounds__(256) present_copy_kernel(const uint2 *__restrict__ src, uint2 *__restrict__ out, uint32_t npix, int w) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= npix) return;
    out[t] = pack_texel(SrcSplit{src}.at((int)(t % (uint32_t)w), (int)(t / (uint32_t)w), w));
}
// downsample 0 of a presented frame: `scene` is the Split frame itself (window of the frame's size) or the stored S; sw x sh is S's size either way
__global__ void __launch_bounds__(256) present_down0_kernel(const uint2 *__restrict__ scene, int sw, int sh, uint2 *__restrict__ out, int ow, int oh) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)(ow * oh)) return;
    out[t] = downsample_texel(SrcSplit{scene}, sw, sh, ow, oh, (int)(t % (uint32_t)ow), (int)(t / (uint32_t)ow));
}

// render_character_cell (postprocess.wgsl:202-246): the atlas texel that the cell (cx, cy) -- whole numbers held in f32, tested against the grid before
// any conversion -- shows at the position (px, py) measured in cells from its top left corner; 0 where the cell is outside the grid or the position
// outside the atlas cell. DESIGN.md 4.14.
AIC_DEV uint32_t text_cell(const PresentText &tx, float cx, float cy, float px, float py) {
    if (!(cx >= 0.0f && cy >= 0.0f && cx < (float)tx.cols && cy < (float)tx.rows)) return 0u;
    uint32_t k = tx.codes[(uint32_t)cy * tx.cols + (uint32_t)cx];
    if (k == 0u) k = 0x20u;  // (the character texture is cleared to zero, not to spaces)
    const float ftx = px * (float)(tx.cell_w - 2u * tx.margin) + (float)tx.margin;
    const float fty = py * (float)(tx.cell_h - 2u * tx.margin) + (float)tx.margin;
    if (!(ftx >= 0.0f && fty >= 0.0f && ftx < (float)tx.cell_w && fty < (float)tx.cell_h)) return 0u;
    return tx.atlas[((k >> 4) * tx.cell_h + (uint32_t)fty) * (16u * tx.cell_w) + (k & 15u) * tx.cell_w + (uint32_t)ftx];
}
AIC_DEV uint32_t max_bytes(uint32_t a, uint32_t b) {
    return max(a & 0xffu, b & 0xffu) | max(a & 0xff00u, b & 0xff00u) | max(a & 0xff0000u, b & 0xff0000u) | max(a & 0xff000000u, b & 0xff000000u);
}
// render_text (postprocess.wgsl:160-194) at the centre (u, v) of an output pixel: the component-wise maximum of the four nearest cells' texels. The
// maximum is taken on the bytes: b / 255 is monotonic, so it is the maximum of the quotients.
AIC_DEV float4 text_at(const PresentText &tx, float u, float v) {
    const float tcx = (u - tx.origin[0]) * tx.scale[0] * (float)tx.cols, tcy = (v - tx.origin[1]) * tx.scale[1] * (float)tx.rows;
    float fx = floorf(tcx), fy = floorf(tcy);
    float px = tcx - fx, py = tcy - fy;
    if (px < 0.5f) { fx -= 1.0f; px += 1.0f; }
    if (py < 0.5f) { fy -= 1.0f; py += 1.0f; }
    const uint32_t t = max_bytes(max_bytes(text_cell(tx, fx, fy, px, py), text_cell(tx, fx + 1.0f, fy, px - 1.0f, py)),
                                 max_bytes(text_cell(tx, fx, fy + 1.0f, px, py - 1.0f), text_cell(tx, fx + 1.0f, fy + 1.0f, px - 1.0f, py - 1.0f)));
    return make_float4((float)(t & 0xffu) / 255.0f, (float)((t >> 8) & 0xffu) / 255.0f, (float)((t >> 16) & 0xffu) / 255.0f, (float)(t >> 24) / 255.0f);
}

// postprocess_fragment (postprocess.wgsl:140-158, 251-276) on an opaque scene: mix(S, B, i), the tone map, (TEXT) the info text over it, then sRGB8 with
// alpha byte 255 or (F16) the linear colour as four f16 with alpha 1.0. STRETCH: S is formed here from an sw x sh frame; otherwise `src` holds S's
// texels at the window's size. The body of the composite kernels below: one output texel per lane, s_thr the workgroup's sRGB window in LDS.
template <bool STRETCH, bool F16, bool TEXT>
AIC_DEV void composite_texel(const float *s_thr, const uint2 *__restrict__ src, int sw, int sh, const uint2 *__restrict__ mip0, int w, int h, int t0x, int t0y,
                             float intensity, int32_t tone_mapping, float m, const PresentText &tx, void *__restrict__ out) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    const uint32_t pix = t < npix ? t : npix - 1u;  // (every lane of the wave runs srgb8_rgb's ballot; only the real pixels store)
    const int x = (int)(pix % (uint32_t)w), y = (int)(pix / (uint32_t)w);
    const SrcSplit s{src};
    const float4 c = scene_at<STRETCH>(s, sw, sh, w, h, x, y);
    float r = c.x, g = c.y, bl = c.z;
    if (mip0) {  // (launch-uniform: bloom_intensity > 0)
        const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)h;
        const float4 B = sample<false>(SrcGlobal{mip0}, t0x, t0y, u, v);
        const float keep = 1.0f - intensity;
        r = r * keep + B.x * intensity;
        g = g * keep + B.y * intensity;
        bl = bl * keep + B.z * intensity;
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
    if (TEXT) {  // tone_mapped_scene * (1 - text.a) + text (postprocess.wgsl:268-273): the text is not tone-mapped
        float4 text = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        // outside the rectangle every cell in reach holds a blank: the same zeros without the lookups
        if ((uint32_t)x >= tx.x0 && (uint32_t)x < tx.x1 && (uint32_t)y >= tx.y0 && (uint32_t)y < tx.y1)
            text = text_at(tx, ((float)x + 0.5f) / (float)w, ((float)y + 0.5f) / (float)h);
        const float keep = 1.0f - text.w;
        r = r * keep + text.x;
        g = g * keep + text.y;
        bl = bl * keep + text.z;
    }
    if (F16) {
        if (t < npix) ((uint2 *)out)[t] = pack_texel(make_float4(r, g, bl, 1.0f));
    } else {
        uint32_t R, G, B;
        srgb8_rgb(r, g, bl, s_thr, R, G, B);
        if (t < npix) ((uint32_t *)out)[t] = R | (G << 8) | (B << 16) | 0xff000000u;
    }
}
template <bool STRETCH, bool F16>
__global__ void __launch_bounds__(256) present_composite_kernel(const uint2 *__restrict__ src, int sw, int sh, const uint2 *__restrict__ mip0, int w, int h, int t0x,
                                                                int t0y, float intensity, int32_t tone_mapping, float m, const float *__restrict__ thr,
                                                                void *__restrict__ out) {
    __shared__ float s_thr[F16 ? 1u : kSrgbWindowWords];
    if (!F16) {
        srgb_window_to_lds(s_thr, thr, threadIdx.x, 256u);
        __syncthreads();
    }
    composite_texel<STRETCH, F16, false>(s_thr, src, sw, sh, mip0, w, h, t0x, t0y, intensity, tone_mapping, m, PresentText{}, out);
}
// ... with the info text of `tx` laid over the tone-mapped scene (aic_present_split_text)
template <bool STRETCH, bool F16>
__global__ void __launch_bounds__(256) present_composite_text_kernel(const uint2 *__restrict__ src, int sw, int sh, const uint2 *__restrict__ mip0, int w, int h, int t0x,
                                                                     int t0y, float intensity, int32_t tone_mapping, float m, const float *__restrict__ thr,
                                                                     const PresentText tx, void *__restrict__ out) {
    __shared__ float s_thr[F16 ? 1u : kSrgbWindowWords];
    if (!F16) {
        srgb_window_to_lds(s_thr, thr, threadIdx.x, 256u);
        __syncthreads();
    }
    composite_texel<STRETCH, F16, true>(s_thr, src, sw, sh, mip0, w, h, t0x, t0y, intensity, tone_mapping, m, tx, out);
}

// rerun_frame_copy_color_fragment / rerun_frame_copy_depth_fragment (rerun-copy.wgsl:47-88) on a resident Split frame, DESIGN.md 4.15: one output pixel per
// lane. COLOR: the scene texel of a presentation at the logged size through the same encoder, alpha byte 255. The depth is the NEAREST depth texel's
// (never interpolated): 0 for a UI pixel or a pixel of no layer (sign bit), a NaN, a pixel whose colour texel is the "nothing known" marker, and the far
// plane (1.0); else the distance lin_depth gives. The pixels whose exported depth is finite and > 0 are counted by ballot and their least and greatest
// depth reduced across the wave: one atomic of each kind per wave that has any, on the bit patterns (positive floats order as unsigned integers), into
// the slot of the counters that the wave's index selects.
struct ExportZw { float z[4]; };
template <bool STRETCH, bool COLOR>
__global__ void __launch_bounds__(256) export_kernel(const uint2 *__restrict__ src, const float *__restrict__ src_depth, int sw, int sh, int w, int h,
                                                     const ExportZw ipzw, const float *__restrict__ thr, uint32_t *__restrict__ color,
                                                     float *__restrict__ depth, ExportCounts *__restrict__ counts) {
    __shared__ float s_thr[COLOR ? kSrgbWindowWords : 1u];
    if (COLOR) {
        srgb_window_to_lds(s_thr, thr, threadIdx.x, 256u);
        __syncthreads();
    }
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    const uint32_t pix = t < npix ? t : npix - 1u;  // (every lane of the wave runs the ballots and the reduction; only the real pixels store and count)
    const int x = (int)(pix % (uint32_t)w), y = (int)(pix / (uint32_t)w);
    if (COLOR) {
        const float4 c = scene_at<STRETCH>(SrcSplit{src}, sw, sh, w, h, x, y);
        uint32_t R, G, B;
        srgb8_rgb(c.x, c.y, c.z, s_thr, R, G, B);
        if (t < npix) color[t] = R | (G << 8) | (B << 16) | 0xff000000u;
    }
    const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)h;
    const uint32_t ix = min((uint32_t)(u * (float)sw), (uint32_t)sw - 1u), iy = min((uint32_t)(v * (float)sh), (uint32_t)sh - 1u);
    const uint32_t at = iy * (uint32_t)sw + ix;
    const float d = src_depth[at];
    const uint2 c = src[at];
    float z = 0.0f;
    if ((__float_as_uint(d) >> 31) == 0u && d == d && texel_valid(c) && d != 1.0f) z = lin_depth(d, ipzw.z);
    if (depth && t < npix) depth[t] = z;
    const bool surface = t < npix && z > 0.0f && z <= 3.4028235e38f;  // finite and positive
    const unsigned long long b = __ballot(surface);
    if (b == 0ull) return;  // (wave-uniform)
    uint32_t lo = surface ? __float_as_uint(z) : 0xffffffffu, hi = surface ? __float_as_uint(z) : 0u;
    for (int m = 32; m >= 1; m >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, m, 64));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, m, 64));
    }
    if ((threadIdx.x & 63u) == 0u) {
        ExportCounts *const slot = counts + ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (kExportSlots - 1u));
        atomicAdd(&slot->n_surface, (uint32_t)__popcll(b));
        atomicMin(&slot->min_bits, lo);
        atomicMax(&slot->max_bits, hi);
    }
}

}  // namespace

hipError_t launch_export(const ExportParams &p, hipStream_t stream) {
    const uint32_t npix = p.out_width * p.out_height;
    if (!npix) return hipSuccess;
    hipError_t e;
    if ((e = hipMemsetAsync(p.counts, 0, sizeof(ExportCounts) * kExportSlots, stream)) != hipSuccess) return e;
    if ((e = hipMemset2DAsync(&p.counts->min_bits, sizeof(ExportCounts), 0xff, 4, kExportSlots, stream)) != hipSuccess) return e;
    const int w = (int)p.out_width, h = (int)p.out_height, sw = (int)p.src_width, sh = (int)p.src_height;
    const bool stretch = sw != w || sh != h;
    auto kernel = stretch ? (p.color ? export_kernel<true, true> : export_kernel<true, false>) : (p.color ? export_kernel<false, true> : export_kernel<false, false>);
    const float *src_depth = reinterpret_cast<const float *>(p.src + (size_t)p.src_width * p.src_height);
    ExportZw ipzw;
    for (int i = 0; i < 4; i++) ipzw.z[i] = p.ipzw[i];
    kernel<<<bloom_blocks_of(npix), 256, 0, stream>>>(p.src, src_depth, sw, sh, w, h, ipzw, p.srgb_thr, p.color, p.depth, p.counts);
    return hipGetLastError();
}

void launch_present_scene(const BloomGeom &g, const PresentParams &p, hipStream_t stream) {
    if (!g.width || !g.height) return;
    const int w = (int)g.width, h = (int)g.height, sw = (int)p.src_width, sh = (int)p.src_height;
    const uint32_t blocks = bloom_blocks_of(g.width * g.height);
    if (sw != w || sh != h) present_stretch_kernel<<<blocks, 256, 0, stream>>>(p.src, sw, sh, p.scene, w, h);
    else present_copy_kernel<<<blocks, 256, 0, stream>>>(p.src, p.scene, g.width * g.height, w);
}

void launch_present(const BloomGeom &g, const PresentParams &p, hipStream_t stream) {
    if (!g.width || !g.height || !g.levels) return;
    const int w = (int)g.width, h = (int)g.height, sw = (int)p.src_width, sh = (int)p.src_height;
    const uint32_t blocks = bloom_blocks_of(g.width * g.height);
    const bool bloomed = p.intensity > 0.0f;
    bool stretch = sw != w || sh != h;
    const uint2 *scene = p.src;
    if (bloomed) {
        if (stretch) {  // S is read five times over by downsample 0 and once by the composite: store it
            present_stretch_kernel<<<blocks, 256, 0, stream>>>(p.src, sw, sh, p.scene, w, h);
            scene = p.scene;
            stretch = false;
        }
        present_down0_kernel<<<bloom_blocks_of(g.mw[0] * g.mh[0]), 256, 0, stream>>>(scene, w, h, p.mips + g.off[0], (int)g.mw[0], (int)g.mh[0]);
        launch_bloom_stages(g, p.mips, stream);
    }
    const uint2 *const mip0 = bloomed ? p.mips + g.off[0] : nullptr;
    const int cw = stretch ? sw : w, ch = stretch ? sh : h;
    auto composite = stretch ? (p.out_f16 ? present_composite_kernel<true, true> : present_composite_kernel<true, false>)
                             : (p.out_f16 ? present_composite_kernel<false, true> : present_composite_kernel<false, false>);
    if (!p.text.codes) {
        composite<<<blocks, 256, 0, stream>>>(scene, cw, ch, mip0, w, h, (int)g.mw[0], (int)g.mh[0], p.intensity, p.tone_mapping, p.maximum_intensity, p.srgb_thr, p.out);
        return;
    }
    auto with_text = stretch ? (p.out_f16 ? present_composite_text_kernel<true, true> : present_composite_text_kernel<true, false>)
                             : (p.out_f16 ? present_composite_text_kernel<false, true> : present_composite_text_kernel<false, false>);
    with_text<<<blocks, 256, 0, stream>>>(scene, cw, ch, mip0, w, h, (int)g.mw[0], (int)g.mh[0], p.intensity, p.tone_mapping, p.maximum_intensity, p.srgb_thr, p.text, p.out);
}

}  // namespace aic
