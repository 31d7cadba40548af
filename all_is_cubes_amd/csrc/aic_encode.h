// aic_encode.h -- the colour encoder shared by the trace kernels (aic_trace.hip) and the bloom post-process (aic_bloom.hip):
// Rgba::from(ColorBuf), the PositiveSign arithmetic it relies on, and Rgba::to_srgb8 through the window table of sRGB8 thresholds.
// The bodies are the trace kernels' own, moved here unchanged so that a bloomed frame is encoded by the same instructions as a plain one.
// The bucket table of sRGB8 (srgb8_bucket_*, the trace kernels' FINISH) is plain C++ that also compiles for the host without HIP: tests build it with g++ and
// check it against the thresholds for every bit pattern (tests/test_srgb8_bucket_host.py).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AIC_ENC_HD __host__ __device__ __forceinline__
#else
#define AIC_ENC_HD static inline
#endif

namespace aic {

// Rgba::to_srgb8 colour channels by BUCKET: the encoding of c is the number of thresholds thr[1..255] <= c (below), a step function of c's bit pattern. The
// thresholds lie at least 100 925 bit patterns apart (k = 189 / 190, near 0.506), more than 2^16, so the patterns that share their upper 16 bits -- a bucket -- hold
// at most one threshold. One 4-byte entry per bucket from thr[1]'s (0x391f) to 1.0's (0x3f80) then gives the exact code with one load, one compare and one add:
//   bits 24-31  the code at the bucket's first pattern: the number of thresholds in the buckets below
//   bits 0-16   the low 16 bits of the bucket's threshold, or 0x10000 (which no pattern's low half reaches) when it has none
// A value below the first bucket encodes like the first bucket's first pattern (at or below thr[1]), one above 1.0 like 1.0: the caller clamps.
constexpr uint32_t kSrgbBucketFirst = 0x391fu, kSrgbBucketLast = 0x3f80u;
constexpr uint32_t kSrgbBucketWords = kSrgbBucketLast - kSrgbBucketFirst + 1u;  // 1634
constexpr uint32_t kSrgbBucketNoThreshold = 0x10000u;

AIC_ENC_HD uint32_t srgb8_float_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
#endif
}

// Builds the table from thr[0..255] (thr[k], k >= 1: the smallest f32 whose encoding is >= k; thr[0] is not read). False -- and the table is not to be used -- if
// the thresholds do not fit it: not ascending, outside the buckets, or two in one bucket.
AIC_ENC_HD bool srgb8_bucket_build(const float *thr, uint32_t *table) {
    for (uint32_t i = 0; i < kSrgbBucketWords; i++) table[i] = kSrgbBucketNoThreshold;
    uint32_t below = kSrgbBucketFirst << 16;  // (what smaller values are clamped to has to encode to 0)
    for (uint32_t k = 1; k < 256u; k++) {
        const uint32_t bits = srgb8_float_bits(thr[k]);
        if (bits <= below || (bits >> 16) < kSrgbBucketFirst || (bits >> 16) >= kSrgbBucketLast) return false;  // (the last bucket is 1.0's alone)
        below = bits;
        uint32_t &e = table[(bits >> 16) - kSrgbBucketFirst];
        if (e != kSrgbBucketNoThreshold) return false;
        e = bits & 0xffffu;
    }
    uint32_t code = 0u;
    for (uint32_t i = 0; i < kSrgbBucketWords; i++) {
        const bool has = table[i] != kSrgbBucketNoThreshold;
        table[i] |= code << 24;
        code += has ? 1u : 0u;
    }
    return code == 255u;
}

// The encoding of the float with bit pattern `bits`, which the caller has clamped to [kSrgbBucketFirst << 16, 1.0f]
AIC_ENC_HD uint32_t srgb8_bucket_encode(uint32_t bits, const uint32_t *table) {
    const uint32_t e = table[(bits >> 16) - kSrgbBucketFirst];
    return (e >> 24) + ((bits & 0xffffu) >= (e & 0x1ffffu) ? 1u : 0u);
}

// One colour channel: clamped into the table's range (NaN goes to its lower end: fmaxf returns the operand that is a number) and looked up for every value, so
// that nothing branches; 0, negatives (cannot occur) and NaN encode to 0.
AIC_ENC_HD uint32_t srgb8_bucket_channel(float c, const uint32_t *table) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float lo = __uint_as_float(kSrgbBucketFirst << 16);
#else
    const uint32_t lo_bits = kSrgbBucketFirst << 16;
    float lo;
    memcpy(&lo, &lo_bits, 4);
#endif
    const uint32_t code = srgb8_bucket_encode(srgb8_float_bits(fminf(fmaxf(c, lo), 1.0f)), table);
    return c > 0.f ? code : 0u;
}

}  // namespace aic

#if defined(__HIPCC__)

#ifndef AIC_DEV
#define AIC_DEV __device__ __forceinline__
#endif
// (aic_raycast.h explains it: a wave-uniform block that must stay a branch)
#ifndef AIC_RARE_PATH
#define AIC_RARE_PATH() asm volatile("" ::: "memory")
#endif

namespace aic {

AIC_DEV float ps_clamped(float v) { return v > 0.f ? v : 0.f; }          // restricted_number.rs:240-248

// PositiveSign::mul: 0 * inf => 0. Both factors are PositiveSign values (not NaN, sign bit clear: what the reference's type holds and aic_upload_* / the
// kernel's own clamps guarantee), so the product is >= +0 or the NaN of 0 * inf, and max(product, 0) -- one instruction: it returns the operand that
// is a number -- is the reference's "NaN becomes zero" (a compare and a select until round 6; fifteen of them in a SHADE event).
AIC_DEV float ps_mul(float a, float b) { return fmaxf(a * b, 0.0f); }

struct ColorBuf {  // raytracer_components.rs:20-39
    float l0, l1, l2, t;
};

AIC_DEV float luminance(float r, float g, float b) { return g * 0.7152f + (r * 0.2126f + b * 0.0722f); }

// Rgba::from(ColorBuf) (raytracer_components.rs:122-147)
AIC_DEV void cb_to_rgba(const ColorBuf &b, float out[4]) {
    if (b.t >= 1.0f) {
        out[0] = out[1] = out[2] = out[3] = 0.f;
        return;
    }
    float alpha = 1.0f - b.t;
    float c0 = b.l0, c1 = b.l1, c2 = b.l2;
    if (__ballot(alpha != 1.0f) != 0ull) {  // x / 1.0f == x: fully opaque pixels (the usual case) need no division
        c0 = b.l0 / alpha; c1 = b.l1 / alpha; c2 = b.l2 / alpha;
    }
    bool ok = (c0 >= 0.f) & (c1 >= 0.f) & (c2 >= 0.f);  // false for negative or NaN
    out[0] = ok ? (c0 > 0.f ? c0 : 0.f) : 1.0f;
    out[1] = ok ? (c1 > 0.f ? c1 : 0.f) : 0.0f;
    out[2] = ok ? (c2 > 0.f ? c2 : 0.f) : 0.0f;
    out[3] = (alpha > 0.f && alpha <= 1.f) ? alpha : (alpha == 0.f ? 0.f : 1.0f);
}

AIC_DEV uint32_t round_sat_u8(float x) {  // `(x).round() as u8`
    float r = roundf(x);
    if (!(r > 0.f)) return 0u;  // NaN, negatives, zero
    if (r >= 255.f) return 255u;
    return (uint32_t)r;
}

// Rgba::to_srgb8 colour channels (color.rs:1038-1054) without powf: `thr[k]` (k = 1..255) is the smallest f32 whose reference encoding is >= k (built on
// the host with the reference formula), so the encoding of c is the number of thresholds <= c. A fast estimate k seeds the count, the thresholds make
// it exact. The kernel holds them as a WINDOW table `w` of kSrgbWindowWords floats -- w[j] = thr[j - 1], with -inf below thr[1] and NaN above
// thr[255] -- so that the four thresholds around an estimate, thr[k - 1 .. k + 2], are w[k .. k + 3] for every k in 0..255: c >= -inf always holds,
// c >= NaN never. The three channels' eight reads are issued together and compared without a branch; the count of thresholds <= c among the four
// settles the encoding unless it is 0 or 4 (the estimate was off by two or more: v_log_f32 / v_exp_f32 are good to about an ulp, so never seen), and
// then the thresholds are searched as before round 6 (two dependent LDS reads per step of two loops per channel, for every pixel).
constexpr uint32_t kSrgbWindowWords = 260u;
AIC_DEV void srgb_window_to_lds(float *w, const float *thr, uint32_t tid, uint32_t nthreads) {
    for (uint32_t i = tid; i < kSrgbWindowWords; i += nthreads)
        w[i] = i < 2u ? __uint_as_float(0xff800000u) : (i <= 256u ? thr[i - 1u] : __uint_as_float(0x7fc00000u));
}
AIC_DEV int srgb8_estimate(float c) {  // 0..255 (c > 0)
    const float cc = fminf(c, 1.0f);
    const float e = cc <= 0.0031308f ? cc * 12.92f : 1.055f * __builtin_amdgcn_exp2f(0.41666666f * __builtin_amdgcn_logf(cc)) - 0.055f;
    const int k = (int)(e * 255.f + 0.5f);
    return k < 0 ? 0 : (k > 255 ? 255 : k);
}
AIC_DEV uint32_t srgb8_search(float c, int k, const float *__restrict__ w) {  // c > 0; thr[j] = w[j + 1]
    while (k < 255 && c >= w[k + 2]) k++;
    while (k > 0 && c < w[k + 1]) k--;
    return (uint32_t)k;
}
AIC_DEV void srgb8_rgb(float r, float g, float b, const float *__restrict__ w, uint32_t &R, uint32_t &G, uint32_t &B) {
    // 0, negatives (cannot occur) and NaN encode to 0
    const bool pr = r > 0.f, pg = g > 0.f, pb = b > 0.f;
    const int kr = pr ? srgb8_estimate(r) : 0, kg = pg ? srgb8_estimate(g) : 0, kb = pb ? srgb8_estimate(b) : 0;
    const float r0 = w[kr], r1 = w[kr + 1], r2 = w[kr + 2], r3 = w[kr + 3];
    const float g0 = w[kg], g1 = w[kg + 1], g2 = w[kg + 2], g3 = w[kg + 3];
    const float b0 = w[kb], b1 = w[kb + 1], b2 = w[kb + 2], b3 = w[kb + 3];
    const int nr = (int)(r >= r0) + (int)(r >= r1) + (int)(r >= r2) + (int)(r >= r3);
    const int ng = (int)(g >= g0) + (int)(g >= g1) + (int)(g >= g2) + (int)(g >= g3);
    const int nb = (int)(b >= b0) + (int)(b >= b1) + (int)(b >= b2) + (int)(b >= b3);
    R = pr ? (uint32_t)(kr - 2 + nr) : 0u;
    G = pg ? (uint32_t)(kg - 2 + ng) : 0u;
    B = pb ? (uint32_t)(kb - 2 + nb) : 0u;
    // (n - 1) > 2 unsigned <=> n is 0 or 4
    const bool open_r = pr & ((uint32_t)(nr - 1) > 2u), open_g = pg & ((uint32_t)(ng - 1) > 2u), open_b = pb & ((uint32_t)(nb - 1) > 2u);
    if (__builtin_amdgcn_ballot_w64(open_r | open_g | open_b) != 0ull) {
        AIC_RARE_PATH();
        if (open_r) R = srgb8_search(r, kr, w);
        if (open_g) G = srgb8_search(g, kg, w);
        if (open_b) B = srgb8_search(b, kb, w);
    }
}

// The three channels from the bucket table in global memory (the trace kernels' FINISH): one load per channel, no LDS
AIC_DEV void srgb8_rgb_bucket(float r, float g, float b, const uint32_t *__restrict__ table, uint32_t &R, uint32_t &G, uint32_t &B) {
    R = srgb8_bucket_channel(r, table);
    G = srgb8_bucket_channel(g, table);
    B = srgb8_bucket_channel(b, table);
}
}  // namespace aic

#endif  // __HIPCC__
