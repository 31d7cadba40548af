// aic_reproject.hip -- the reprojection post-process on gfx950: a resident Split frame drawn into a new camera as depth-tested point sprites, then the
// reference's gap fill (aic_reproject.h; DESIGN.md "Reprojection", which restates every operation below and is what tests/reproject_ref.py follows).
//
//  * Splat: a lane per source pixel. The sprite's centre, scale and depth are the vertex shader's f32 operations in its order (-ffp-contract=off); the
//    lane then walks a box of output pixels that contains every pixel the coverage test can accept, and for each covered one makes one 64-bit
//    device-scope atomicMin of (bits(z) << 32) | (0xFFFFFFFF - s) on a key buffer cleared to all ones: z >= +0, so its bits order as its value, and
//    among equal z the greatest draw index s wins, which is what LessEqual in draw order leaves. Order-independent and exact.
//  * Resolve: a lane per output pixel turns its key into the splat image R (the winner's texel, bit for bit) and the depth plane D, and counts the gaps.
//  * Gap fill: every mip is f16 x 4; f32 -> f16 rounds to nearest even and overflows to infinity, as the Split store does. Sampling is Nearest and
//    MirrorRepeat on texel indices. Mip 0 as downsample 0 forms it is read by downsample 1 and by upsample 1 (its "higher" input) only, at texels
//    (2i+1, 2j+1) and their neighbours, and upsample 0 overwrites all of it from mip 1: it is never stored. Downsample 1 and upsample 1 form the texels of
//    it they read (SrcDown0), and the final store evaluates upsample 0 at the width x height texels it samples, straight into dst.
//  * Launches: one grid per stage, a texel per thread (the measured split per kernel is in profiles/reproject_timing.txt).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_reproject.h"
#include "aic_split_texel.h"
#include "aic_tunables.h"

namespace aic {

namespace {

constexpr unsigned long long kNoKey = ~0ull;
constexpr uint32_t kMarkerLo = 0u, kMarkerHi = 0xBC000000u;  // (0, 0, 0, -1) in f16: "nothing known"

AIC_DEV float f16_value(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
AIC_DEV uint32_t f16_bits(float x) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x); }  // nearest even, overflow to infinity
AIC_DEV float4 unpack_texel(uint2 v) {
    return make_float4(f16_value(v.x & 0xffffu), f16_value(v.x >> 16), f16_value(v.y & 0xffffu), f16_value(v.y >> 16));
}
AIC_DEV uint2 pack_texel(float4 c) { return make_uint2(f16_bits(c.x) | (f16_bits(c.y) << 16), f16_bits(c.z) | (f16_bits(c.w) << 16)); }
AIC_DEV uint2 marker() { return make_uint2(kMarkerLo, kMarkerHi); }

AIC_DEV int wrap_mirror(int i, int n) {  // AddressMode::MirrorRepeat on texel indices: period 2n, reflected
    if ((uint32_t)i < (uint32_t)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m >= n ? p - 1 - m : m;
}

// one add per wave (the lanes of a wave that count are balloted; lane 0 of the wave adds)
AIC_DEV void count_wave(unsigned long long *counter, bool mine) {
    const unsigned long long b = __ballot(mine);
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(counter, (unsigned long long)__popcll(b));
}

struct SplatArgs {
    float m[16];
    float ipzw[4];
    uint32_t width, height;
};

// rt_reproject_vertex + rt_reproject_fragment (rt-copy.wgsl:73-223) for source pixel s, against every output pixel its sprite can cover
__global__ void __launch_bounds__(256) reproject_splat_kernel(const float *__restrict__ depth, SplatArgs a, unsigned long long *__restrict__ keys,
                                                              ReprojectCounts *__restrict__ counts) {
    const uint32_t W = a.width, H = a.height;
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const bool live = s < W * H;
    bool draw = false;
    float ox = 0.f, oy = 0.f, oz = 0.f, ratio = 1.f;
    const float rw = 1.0f / (float)W, rh = 1.0f / (float)H;
    if (live) {
        const uint32_t sx = s % W, sy = s / W;
        const float tcx = ((float)sx + 0.5f) * rw, tcy = ((float)sy + 0.5f) * rh;
        const float nx = tcx * 2.0f - 1.0f, ny = -(tcy * 2.0f - 1.0f);
        const float e = depth[s];
        const bool ui = (__float_as_uint(e) >> 31) != 0u;
        const float d = fabsf(e);
        if (e != e) {
            // a NaN depth draws nothing
        } else if (ui) {
            ox = nx; oy = ny; oz = 0.0f; ratio = 1.0f;
            draw = true;
        } else {
            float h[4];
            for (int r = 0; r < 4; r++) h[r] = ((a.m[r] * nx + a.m[4 + r] * ny) + a.m[8 + r] * d) + a.m[12 + r];
            if (h[3] > 0.0f) {
                ox = h[0] / h[3]; oy = h[1] / h[3]; oz = h[2] / h[3];
                ratio = lin_depth(d, a.ipzw) / lin_depth(oz, a.ipzw);
                if (ratio > 0.0f && ratio <= 3.4028235e38f) {  // finite and positive
                    ratio = fminf(ratio, AIC_REPROJECT_RATIO_CAP);
                    draw = true;
                }
            }
        }
    }
    count_wave(&counts->n_splats, live && draw);
    count_wave(&counts->n_dropped, live && !draw);
    if (!draw) return;
    const float ozc = fminf(fmaxf(oz, 0.0f), 1.0f);
    const float kx = (4.0f * rw) * ratio, ky = (4.0f * rh) * ratio;
    // The candidate box. A covered pixel has qx^2 + qy^2 <= 0.33, so |fx - ox| <= 0.57446 kx: at most 1.14892 ratio pixels from the sprite's centre
    // ((ox + 1) W / 2 - 1/2 in pixel units), and the same above it; below it qy >= -1/2 allows ratio pixels. 1.15 ratio + 0.05 leaves 0.03 pixel and
    // more for the roundings of fx, of q and of the centre computed here (each a few ulp of the frame's size: 0.02 pixel at 65535). A centre that is
    // not finite covers nothing: q is then infinite or NaN.
    if (!(fabsf(ox) <= 3.4028235e38f) || !(fabsf(oy) <= 3.4028235e38f)) return;
    const float rad = 1.15f * ratio + 0.05f, below = 1.001f * ratio + 0.05f;
    const float cx = (ox + 1.0f) * 0.5f * (float)W - 0.5f, cy = (1.0f - oy) * 0.5f * (float)H - 0.5f;
    const float xlo = fmaxf(ceilf(cx - rad), 0.0f), xhi = fminf(floorf(cx + rad), (float)(W - 1u));
    const float ylo = fmaxf(ceilf(cy - rad), 0.0f), yhi = fminf(floorf(cy + below), (float)(H - 1u));
    if (!(xlo <= xhi) || !(ylo <= yhi)) return;
    const uint32_t x0 = (uint32_t)xlo, x1 = (uint32_t)xhi, y0 = (uint32_t)ylo, y1 = (uint32_t)yhi;  // within [0, W-1] and [0, H-1]
    const unsigned long long low = (unsigned long long)(0xFFFFFFFFu - s);
    for (uint32_t py = y0; py <= y1; py++) {
        const float fy = -(((float)py + 0.5f) * rh * 2.0f - 1.0f);
        const float qy = (fy - oy) / ky;
        if (!(qy >= -0.5f)) continue;
        for (uint32_t px = x0; px <= x1; px++) {
            const float fx = ((float)px + 0.5f) * rw * 2.0f - 1.0f;
            const float qx = (fx - ox) / kx;
            const float d2 = qx * qx + qy * qy;
            if (qy <= 1.0f - 1.7320508f * fabsf(qx) && d2 <= 0.33f) {
                const float z = fminf(ozc + d2 * 0.0125f, 1.0f);
                atomicMin(&keys[(size_t)py * W + px], ((unsigned long long)__float_as_uint(z) << 32) | low);
            }
        }
    }
}

__global__ void __launch_bounds__(256) reproject_resolve_kernel(const unsigned long long *__restrict__ keys, const uint2 *__restrict__ src_color,
                                                                const float *__restrict__ src_depth, uint32_t npix, uint2 *__restrict__ R,
                                                                float *__restrict__ D, ReprojectCounts *__restrict__ counts) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool gap = false;
    if (t < npix) {
        const unsigned long long key = keys[t];
        gap = key == kNoKey;
        if (gap) {
            R[t] = marker();
            D[t] = 1.0f;
        } else {
            const uint32_t s = 0xFFFFFFFFu - (uint32_t)key;
            R[t] = src_color[s];
            D[t] = __uint_as_float((uint32_t)(key >> 32) | (__float_as_uint(src_depth[s]) & 0x80000000u));
        }
    }
    count_wave(&counts->n_gaps, gap);
}

// The texel sources a stage reads; indices are already wrapped.
struct SrcTex {
    const uint2 *__restrict__ p;
    int w, h;
    AIC_DEV uint2 at(int x, int y) const { return p[(size_t)y * (uint32_t)w + (uint32_t)x]; }
};

// fill(c, list) of gap_fill_downsample / gap_fill_upsample (resampling.wgsl:134-176): the list is s at (x, y) with weight wc, then (xp, y), (xm, y),
// (x, yp), (x, ym) with weight 1; indices MirrorRepeat
template <class Src>
AIC_DEV uint2 fill(uint2 c, const Src &s, int x, int y, int xp, int xm, int yp, int ym, float wc) {
    if (texel_valid(c)) return c;
    const int xs[5] = {x, xp, xm, x, x}, ys[5] = {y, y, y, yp, ym};
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < 5; k++) {
        const uint2 b = s.at(wrap_mirror(xs[k], s.w), wrap_mirror(ys[k], s.h));
        if (texel_valid(b)) {
            const float4 v = unpack_texel(b);
            const float wt = k == 0 ? wc : 1.0f;
            acc.x = acc.x + v.x * wt; acc.y = acc.y + v.y * wt; acc.z = acc.z + v.z * wt; acc.w = acc.w + wt;
        }
    }
    if (acc.w > 0.5f) return pack_texel(make_float4(acc.x / acc.w, acc.y / acc.w, acc.z / acc.w, acc.w / acc.w));
    return marker();
}
template <class Src>
AIC_DEV uint2 downsample_texel(const Src &s, int bx, int by) {  // the centre is the list's first entry
    return fill(s.at(bx, by), s, bx, by, bx + 1, bx - 1, by + 1, by - 1, 1.0f);
}

struct SrcDown0 {  // mip 0 as downsample 0 writes it, formed from R where it is read
    SrcTex R;
    int w, h;  // T0
    AIC_DEV uint2 at(int i, int j) const {
        const int bx = (int)(((uint64_t)(2 * i + 1) * (uint32_t)R.w) / (2ull * (uint32_t)w));
        const int by = (int)(((uint64_t)(2 * j + 1) * (uint32_t)R.h) / (2ull * (uint32_t)h));
        return downsample_texel(R, bx, by);
    }
};

// downsample k >= 1 into mip k (ow x oh) from mip k-1
template <class Src>
AIC_DEV void down_stage(const Src &in, uint2 *__restrict__ out, int ow, int oh) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)ow * (uint32_t)oh) return;
    const int i = (int)(t % (uint32_t)ow), j = (int)(t / (uint32_t)ow);
    out[t] = downsample_texel(in, 2 * i + 1, 2 * j + 1);
}
__global__ void __launch_bounds__(256) reproject_down1_kernel(SrcDown0 in, uint2 *__restrict__ out, int ow, int oh) { down_stage(in, out, ow, oh); }
__global__ void __launch_bounds__(256) reproject_down_kernel(SrcTex in, uint2 *__restrict__ out, int ow, int oh) { down_stage(in, out, ow, oh); }

// upsample k >= 1 into mip k (ow x oh): the centre from `higher` = mip k-1 at the texel whose lower corner the sample point is, the list from
// `in` = mip k+1 at floor((2i+1)/4 + {0, +1/2, -1/2}) -- floors towards minus infinity (the arithmetic shifts)
template <class SrcH>
AIC_DEV void up_stage(const SrcTex &in, const SrcH &higher, uint2 *__restrict__ out, int ow, int oh) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)ow * (uint32_t)oh) return;
    const int i = (int)(t % (uint32_t)ow), j = (int)(t / (uint32_t)ow);
    out[t] = fill(higher.at(2 * i + 1, 2 * j + 1), in, i >> 1, j >> 1, (i + 1) >> 1, (i - 1) >> 1, (j + 1) >> 1, (j - 1) >> 1, 2.0f);
}
__global__ void __launch_bounds__(256) reproject_up1_kernel(SrcTex in, SrcDown0 higher, uint2 *__restrict__ out, int ow, int oh) { up_stage(in, higher, out, ow, oh); }
__global__ void __launch_bounds__(256) reproject_up_kernel(SrcTex in, SrcTex higher, uint2 *__restrict__ out, int ow, int oh) { up_stage(in, higher, out, ow, oh); }

// The final store: dst colour (x, y) is mip 0 at the texel its centre falls in -- upsample 0 evaluated there (its centre and its list are mip 1, which
// mip_ping.rs:353 gives it as the "higher" input too), or, in a chain of one level, downsample 0.
__global__ void __launch_bounds__(256) reproject_final_kernel(SrcDown0 mip0, SrcTex mip1, uint32_t levels, uint32_t keep_splats, uint2 *__restrict__ dst,
                                                              ReprojectCounts *__restrict__ counts) {
    const uint32_t W = (uint32_t)mip0.R.w, H = (uint32_t)mip0.R.h;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool unfilled = false;
    if (t < W * H) {
        const uint32_t x = t % W, y = t / W;
        const int i = (int)(((uint64_t)(2u * x + 1u) * (uint32_t)mip0.w) / (2ull * W));
        const int j = (int)(((uint64_t)(2u * y + 1u) * (uint32_t)mip0.h) / (2ull * H));
        uint2 c;
        const uint2 r = mip0.R.p[t];
        if (keep_splats && texel_valid(r)) c = r;
        else if (levels < 2u) c = mip0.at(i, j);
        else {
            const int hx = i >> 1, hy = j >> 1;
            c = fill(mip1.at(hx, hy), mip1, hx, hy, hx + 2, hx - 2, hy + 2, hy - 2, 2.0f);
        }
        dst[t] = c;
        unfilled = !texel_valid(c);
    }
    count_wave(&counts->n_unfilled, unfilled);
}

uint32_t blocks_of(size_t n) { return (uint32_t)((n + 255u) / 256u); }

}  // namespace

hipError_t launch_reproject(const ReprojectGeom &g, const ReprojectParams &p, hipStream_t stream) {
    const size_t npix = g.npix();
    if (!npix) return hipSuccess;
    const uint32_t L = g.levels;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(p.scratch);
    uint2 *R = reinterpret_cast<uint2 *>(p.scratch + g.keys_bytes());
    uint2 *M = R + npix;
    ReprojectCounts *counts = reinterpret_cast<ReprojectCounts *>(p.scratch + g.scratch_bytes() - 32);
    hipError_t e;
    if ((e = hipMemsetAsync(keys, 0xff, g.keys_bytes(), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(counts, 0, 32, stream)) != hipSuccess) return e;
    SplatArgs a;
    for (int i = 0; i < 16; i++) a.m[i] = p.m[i];
    for (int i = 0; i < 4; i++) a.ipzw[i] = p.ipzw[i];
    a.width = g.width;
    a.height = g.height;
    reproject_splat_kernel<<<blocks_of(npix), 256, 0, stream>>>(p.src_depth, a, keys, counts);
    reproject_resolve_kernel<<<blocks_of(npix), 256, 0, stream>>>(keys, p.src_color, p.src_depth, (uint32_t)npix, R, p.dst_depth, counts);
    auto mip = [&](uint32_t k) { return SrcTex{M + g.off[k], (int)g.mw[k], (int)g.mh[k]}; };
    const SrcDown0 mip0{SrcTex{R, (int)g.width, (int)g.height}, (int)g.mw[0], (int)g.mh[0]};
    // mip_ping.rs:301-420 with one repetition: downsample 0 .. L-1, then upsample L-2 .. 0 (0: the final store)
    for (uint32_t k = 1; k < L; k++) {
        const uint32_t blocks = blocks_of((size_t)g.mw[k] * g.mh[k]);
        if (k == 1) reproject_down1_kernel<<<blocks, 256, 0, stream>>>(mip0, M + g.off[1], (int)g.mw[1], (int)g.mh[1]);
        else reproject_down_kernel<<<blocks, 256, 0, stream>>>(mip(k - 1), M + g.off[k], (int)g.mw[k], (int)g.mh[k]);
    }
    for (uint32_t k = L >= 2u ? L - 2u : 0u; k >= 1u; k--) {
        const uint32_t blocks = blocks_of((size_t)g.mw[k] * g.mh[k]);
        if (k == 1) reproject_up1_kernel<<<blocks, 256, 0, stream>>>(mip(2), mip0, M + g.off[1], (int)g.mw[1], (int)g.mh[1]);
        else reproject_up_kernel<<<blocks, 256, 0, stream>>>(mip(k + 1), mip(k - 1), M + g.off[k], (int)g.mw[k], (int)g.mh[k]);
    }
    reproject_final_kernel<<<blocks_of(npix), 256, 0, stream>>>(mip0, L >= 2u ? mip(1) : SrcTex{nullptr, 1, 1}, L, p.keep_splats, p.dst_color, counts);
    return hipGetLastError();
}

}  // namespace aic
