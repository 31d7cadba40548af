// aic_present_lines.hip -- the line pass of a presentation on gfx950 (aic_present_split_lines; aic_present_lines.h): a line list drawn
// into the stored scene texture S, depth-tested against the resident Split frame's depth plane, before the bloom chain and the composite read S.
//
//  * One wave64 per line, four lines per 256-thread workgroup. Rules 1-3 (clip coordinates, Liang-Barsky clipping, screen coordinates) depend on the
//    line alone: every lane of the wave computes them from the same scalar loads. The lanes then stride over the line's major-axis range, a fragment each.
//  * Draw: the depth test first, then a 64-bit atomicMin of (bits(f) << 32) | line on the pixel's key. f >= +0, so its bits order as its value; among
//    equal depths the lowest line wins: CompareFunction::Less with depth write, in submission order.
//  * Resolve: the same walk. The one fragment whose key the pixel holds stores its colour into S and puts the key back to all ones, so the key image is
//    clean again when the call ends. No other fragment writes that pixel or that key, and none compares equal to all ones (bits(f) of all ones is a NaN).
//  * Both kernels run the same inlined functions, so a fragment's f is the same bits in both.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_bloom_device.h"
#include "aic_present_lines.h"

namespace aic {

namespace {

constexpr unsigned long long kNoKey = ~0ull;

// A line after rules 1-3 and the ordering of rule 4: its ends in screen space, major coordinate ascending.
struct Segment {
    float p0, p1;       // major coordinate
    float q0, q1;       // minor coordinate
    float d0, d1;       // depth z / w
    float c0[3], c1[3]; // colour
    int i_lo, i_hi;     // major indices whose centre lies in [p0, p1), inside the window
    bool x_major;
};

AIC_DEV bool finite6(const float *v) {  // position and r, g, b: alpha is never read
    bool ok = true;
    for (int k = 0; k < 6; k++) ok = ok && isfinite(v[k]);
    return ok;
}

// rules 1-3 and the ordering of rule 4; false: the line is dropped
AIC_DEV bool make_segment(const float *__restrict__ va, const float *__restrict__ vb, const float *m, float W, float H, Segment &s) {
    float a[6], b[6];
    for (int k = 0; k < 6; k++) { a[k] = va[k]; b[k] = vb[k]; }
    if (!finite6(a) || !finite6(b)) return false;
    // 1: clip = M (x, y, z, 1)
    float ca[4], cb[4];
    for (int r = 0; r < 4; r++) {
        ca[r] = ((m[r] * a[0] + m[4 + r] * a[1]) + m[8 + r] * a[2]) + m[12 + r];
        cb[r] = ((m[r] * b[0] + m[4 + r] * b[1]) + m[8 + r] * b[2]) + m[12 + r];
        if (!isfinite(ca[r]) || !isfinite(cb[r])) return false;
    }
    // 2: Liang-Barsky against w + x, w - x, w + y, w - y, z, w - z
    const float fa[6] = {ca[3] + ca[0], ca[3] - ca[0], ca[3] + ca[1], ca[3] - ca[1], ca[2], ca[3] - ca[2]};
    const float fb[6] = {cb[3] + cb[0], cb[3] - cb[0], cb[3] + cb[1], cb[3] - cb[1], cb[2], cb[3] - cb[2]};
    float t_in = 0.0f, t_out = 1.0f;
    bool clipped_in = false, clipped_out = false;
    for (int k = 0; k < 6; k++) {
        const bool na = fa[k] < 0.0f, nb = fb[k] < 0.0f;
        if (na && nb) return false;
        if (na || nb) {
            const float t = fa[k] / (fa[k] - fb[k]);
            if (!isfinite(t)) return false;
            if (na) { clipped_in = true; t_in = t > t_in ? t : t_in; }
            else { clipped_out = true; t_out = t < t_out ? t : t_out; }
        }
    }
    if (t_in > t_out) return false;
    const float e[7] = {ca[0], ca[1], ca[2], ca[3], a[3], a[4], a[5]}, g[7] = {cb[0], cb[1], cb[2], cb[3], b[3], b[4], b[5]};  // (alpha is not used)
    float ea[7], eb[7];
    for (int k = 0; k < 7; k++) {
        const float d = g[k] - e[k];
        ea[k] = clipped_in ? e[k] + t_in * d : e[k];
        eb[k] = clipped_out ? e[k] + t_out * d : g[k];
    }
    // 3: screen coordinates
    if (!(ea[3] > 0.0f) || !(eb[3] > 0.0f)) return false;
    float sa[3], sb[3];  // sx, sy, d
    sa[0] = ((ea[0] / ea[3]) * 0.5f + 0.5f) * W;
    sa[1] = (0.5f - (ea[1] / ea[3]) * 0.5f) * H;
    sa[2] = ea[2] / ea[3];
    sb[0] = ((eb[0] / eb[3]) * 0.5f + 0.5f) * W;
    sb[1] = (0.5f - (eb[1] / eb[3]) * 0.5f) * H;
    sb[2] = eb[2] / eb[3];
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && isfinite(sa[k]) && isfinite(sb[k]);
    for (int k = 4; k < 7; k++) ok = ok && isfinite(ea[k]) && isfinite(eb[k]);
    if (!ok) return false;
    // 4: the major axis, its coordinate ascending
    const float dx = sb[0] - sa[0], dy = sb[1] - sa[1];
    s.x_major = fabsf(dx) >= fabsf(dy);
    const int pi = s.x_major ? 0 : 1, qi = 1 - pi;
    const bool swap = sa[pi] > sb[pi];
    s.p0 = swap ? sb[pi] : sa[pi]; s.p1 = swap ? sa[pi] : sb[pi];
    s.q0 = swap ? sb[qi] : sa[qi]; s.q1 = swap ? sa[qi] : sb[qi];
    s.d0 = swap ? sb[2] : sa[2];   s.d1 = swap ? sa[2] : sb[2];
    for (int k = 0; k < 3; k++) { s.c0[k] = swap ? eb[4 + k] : ea[4 + k]; s.c1[k] = swap ? ea[4 + k] : eb[4 + k]; }
    // centres i + 0.5 in [p0, p1): ceil(p0 - 0.5) <= i < ceil(p1 - 0.5), clamped to the window while still float
    const float n_major = s.x_major ? W : H;
    s.i_lo = (int)fmaxf(ceilf(s.p0 - 0.5f), 0.0f);
    s.i_hi = (int)fminf(ceilf(s.p1 - 0.5f), n_major);
    return true;
}

struct Fragment {
    uint32_t pix;   // y * W + x
    uint32_t x, y;
    float f;        // depth in [0, 1]
    float t;
};

// rule 4 for major index i; false: the minor index falls outside the window
AIC_DEV bool make_fragment(const Segment &s, int i, uint32_t w, uint32_t h, Fragment &fr) {
    const float t = (((float)i + 0.5f) - s.p0) / (s.p1 - s.p0);
    const float jf = floorf(s.q0 + t * (s.q1 - s.q0));
    const float n_minor = (float)(s.x_major ? h : w);
    if (!(jf >= 0.0f && jf < n_minor)) return false;
    const uint32_t j = (uint32_t)jf;
    fr.x = s.x_major ? (uint32_t)i : j;
    fr.y = s.x_major ? j : (uint32_t)i;
    fr.pix = fr.y * w + fr.x;
    fr.t = t;
    fr.f = fminf(fmaxf(s.d0 + t * (s.d1 - s.d0), 0.0f), 1.0f);
    return true;
}

// rule 5: Less against the frame copy's frag_depth (rt-copy.wgsl:55-71: the nearest texel, clamped to [0, 1]; a negative or NaN texel clamps to 0)
AIC_DEV bool depth_test(const LinesParams &p, const Fragment &fr) {
    uint32_t tx = fr.x, ty = fr.y;
    if (p.src_width != p.width || p.src_height != p.height) {
        tx = (uint32_t)(((float)fr.x + 0.5f) / (float)p.width * (float)p.src_width);
        ty = (uint32_t)(((float)fr.y + 0.5f) / (float)p.height * (float)p.src_height);
    }
    tx = tx < p.src_width ? tx : p.src_width - 1u;  // (also at equal size: no index leaves the plane)
    ty = ty < p.src_height ? ty : p.src_height - 1u;
    const uint32_t bits = p.depth[(size_t)ty * p.src_width + tx];
    const float texel = __uint_as_float(bits);
    return !(bits >> 31) && !isnan(texel) && fr.f < fminf(texel, 1.0f);
}

AIC_DEV unsigned long long key_of(const Fragment &fr, uint32_t line) { return ((unsigned long long)__float_as_uint(fr.f) << 32) | line; }

// RESOLVE false: the draw (depth test, atomicMin on the key). true: the resolve (the key's owner stores its colour and resets the key).
template <bool RESOLVE>
__global__ void __launch_bounds__(256) present_lines_kernel(const LinesParams p) {
    const uint32_t line = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (line >= p.n_lines) return;
    const uint32_t lane = threadIdx.x & 63u;
    Segment s;
    const float *v = p.vertices + (size_t)line * (2u * kLineVertexWords);
    if (!make_segment(v, v + kLineVertexWords, p.m, (float)p.width, (float)p.height, s)) {
        if (!RESOLVE && lane == 0) atomicAdd(&p.counts->n_clipped_away, 1ull);
        return;
    }
    uint32_t n_fragments = 0, n_passed = 0, n_pixels = 0;  // wave-uniform: the loop is, and the ballots count whole waves
    for (int base = s.i_lo; base < s.i_hi; base += 64) {
        const int i = base + (int)lane;
        Fragment fr;
        const bool made = i < s.i_hi && make_fragment(s, i, p.width, p.height, fr);
        const bool passed = made && depth_test(p, fr);
        if (!RESOLVE) {
            if (passed) atomicMin(&p.keys[fr.pix], key_of(fr, line));
            n_fragments += (uint32_t)__popcll(__ballot(made));
            n_passed += (uint32_t)__popcll(__ballot(passed));
        } else {
            const bool owner = passed && p.keys[fr.pix] == key_of(fr, line);
            if (owner) {
                p.scene[fr.pix] = pack_texel(make_float4(s.c0[0] + fr.t * (s.c1[0] - s.c0[0]), s.c0[1] + fr.t * (s.c1[1] - s.c0[1]),
                                                         s.c0[2] + fr.t * (s.c1[2] - s.c0[2]), 1.0f));
                if (p.reset_keys) p.keys[fr.pix] = kNoKey;
            }
            n_pixels += (uint32_t)__popcll(__ballot(owner));
        }
    }
    if (lane == 0) {
        if (!RESOLVE) {
            if (n_fragments) atomicAdd(&p.counts->n_fragments, (unsigned long long)n_fragments);
            if (n_passed) atomicAdd(&p.counts->n_passed, (unsigned long long)n_passed);
        } else if (n_pixels) {
            atomicAdd(&p.counts->n_pixels, (unsigned long long)n_pixels);
        }
    }
}

}  // namespace

hipError_t launch_present_lines(const LinesParams &p, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(p.counts, 0, sizeof(LinesCounts), stream);
    if (e != hipSuccess) return e;
    if (p.clear_keys && (e = hipMemsetAsync(p.keys, 0xFF, (size_t)p.width * p.height * 8, stream)) != hipSuccess) return e;
    if (!p.n_lines || !p.width || !p.height) return hipSuccess;
    const uint32_t blocks = (p.n_lines + 3u) / 4u;
    present_lines_kernel<false><<<blocks, 256, 0, stream>>>(p);
    present_lines_kernel<true><<<blocks, 256, 0, stream>>>(p);
    return hipGetLastError();
}

}  // namespace aic
