// aic_colour.h -- the f32 colour arithmetic of the trace kernels (part of the aic_trace.hip translation unit), in the reference's operation order:
//   ZeroOne clamping (all-is-cubes-base/src/math/restricted_number.rs:315-326)
//   ColorBuf::add / opaque (all-is-cubes/src/raytracer_components.rs:87-109; the struct itself and Rgba::from(ColorBuf) are aic_encode.h)
//   f32::powf and f32::exp as the reference's libm computes them (glibc's e_powf.c / e_expf.c), for apply_transmittance
//   (raytracer_components.rs:215-258) and distance_fog (all-is-cubes-render/src/raytracer/sr.rs:745-768)
// The tables are `__device__ const`: internal to the one translation unit that includes this.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_encode.h"

namespace aic {

// ---------------------------------------------------------------------------------------
// colour helpers (f32, reference operation order)

AIC_DEV float zo_clamped(float v) {                                        // restricted_number.rs:315-326
    if (v > 0.f && v <= 1.f) return v;
    if (v <= 0.f) return 0.f;
    return 1.f;
}

// f32::powf as the reference's libm computes it on x86-64 Linux. Rust's `f32::powf` is the C library's
// powf; glibc's (sysdeps/ieee754/flt-32/e_powf.c, from ARM's optimized-routines; not part of
// the reference's tree, restated from the published algorithm) is: log2(x) by a 16-entry table and a
// degree-4 polynomial, y*log2(x), exp2 by a 32-entry table and a cubic, all in f64, rounded to f32
// once. Table and coefficient values are the published __powf_log2_data / __exp2f_data. The
// multiply-adds are fused, as in the FMA build glibc selects on every current x86-64 CPU.
// Domain: 0 < x < 1 normal, y > 0 finite (everything apply_transmittance feeds it); the caller
// handles the rest of what can reach it (x == 0, x == 1, y == 0, y == +inf) itself. ~40 instructions instead of ~270; pinned against the host's
// powf on a million inputs (tests/test_gpu_encode.py).
__device__ const double kPowLog2Tab[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
    {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
    {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
    {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
    {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
    {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2},
};
__device__ const unsigned long long kPowExp2Tab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull,
};
// s_pow: [0,32) the log2 table as (invc, logc) pairs, [32,64) the exp2 table bit patterns
AIC_DEV void pow_tables_to_lds(double *s_pow, uint32_t tid, uint32_t nthreads) {
    for (uint32_t i = tid; i < 64u; i += nthreads)
        s_pow[i] = i < 32u ? kPowLog2Tab[i >> 1][i & 1u] : __longlong_as_double((long long)kPowExp2Tab[i - 32u]);
}
AIC_DEV bool powf_table_domain(float x, float y) {  // 0 < x < 1 normal; y > 0 finite
    const uint32_t ix = __float_as_uint(x), iy = __float_as_uint(y);
    return ix >= 0x00800000u && ix < 0x3f800000u && iy > 0u && iy < 0x7f800000u;
}
// A 64-bit literal that is materialised where it is used (two s_mov). Left to itself the compiler hoists such constants out of
// the persistent loop into VGPR pairs, runs out of registers, spills them to scratch at kernel start (every lane of every wave
// storing the same 8 bytes: most of round 2's 46 MB of WRITE_SIZE per frame) and reloads them from memory in every SHADE event.
AIC_DEV double KC(double v) { asm volatile("" : "+s"(v)); return v; }
AIC_DEV float powf_table(float x, float y, const double *s_pow) {
    const uint32_t ix = __float_as_uint(x);
    // log2_inline
    const uint32_t tmp = ix - 0x3f330000u;
    const uint32_t i = (tmp >> 19) & 15u;
    const uint32_t top = tmp & 0xff800000u;
    const uint32_t iz = ix - top;
    const int k = (int)top >> 23;
    const double invc = s_pow[2u * i], logc = s_pow[2u * i + 1u];
    const double z = (double)__uint_as_float(iz);
    const double r = fma(z, invc, -1.0);
    const double y0 = logc + (double)k;
    const double r2 = r * r;
    double yy = fma(KC(0x1.27616c9496e0bp-2), r, KC(-0x1.71969a075c67ap-2));
    const double pp = fma(KC(0x1.ec70a6ca7baddp-2), r, KC(-0x1.7154748bef6c8p-1));
    const double r4 = r2 * r2;
    double q = fma(KC(0x1.71547652ab82bp+0), r, y0);
    q = fma(pp, r2, q);
    yy = fma(yy, r4, q);
    const double ylogx = (double)y * yy;
    // |y*log2(x)| >= 126: x < 1 and y > 0 make it negative -- underflow to 0 at <= -150, else the
    // general path rounds into the subnormals by itself
    if (ylogx <= -150.0) return 0.0f;
    // exp2_inline
    double kd = ylogx + KC(0x1.8p+47);
    const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
    kd -= KC(0x1.8p+47);
    const double rr = ylogx - kd;
    unsigned long long t = (unsigned long long)__double_as_longlong(s_pow[32u + (uint32_t)(ki & 31u)]);
    t += ki << 47;
    const double sc = __longlong_as_double((long long)t);
    const double zz = fma(KC(0x1.c6af84b912394p-5), rr, KC(0x1.ebfce50fac4f3p-3));
    const double rr2 = rr * rr;
    double e = fma(KC(0x1.62e42ff0c52d6p-1), rr, 1.0);
    e = fma(zz, rr2, e);
    e = e * sc;
    return (float)e;
}
// f32::exp as the reference's libm computes it (glibc sysdeps/ieee754/flt-32/e_expf.c, from ARM's optimized-routines; restated
// from the published algorithm like powf_table above): x * 32/ln2 split into an integer and a remainder, 2^(k/32) from the
// same 32-entry table as powf's exp2 step, a cubic in the remainder, all in f64, rounded to f32 once. Domain: |x| < 88 (the fog
// term feeds it [-1.6, 0]); no overflow / underflow handling. Pinned against the host's expf on every f32 in [-1.6, 0]
// (aic_probe_expf; tests/test_gpu_linear_parity.py).
AIC_DEV float expf_table(float x, const double *s_pow) {
    const double z = KC(0x1.71547652b82fep+5) * (double)x;  // InvLn2N = N / ln 2, N = 32
    double kd = z + KC(0x1.8p+52);
    const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
    kd -= KC(0x1.8p+52);
    const double r = z - kd;
    unsigned long long t = (unsigned long long)__double_as_longlong(s_pow[32u + (uint32_t)(ki & 31u)]);
    t += ki << 47;
    const double sc = __longlong_as_double((long long)t);
    const double zz = fma(KC(0x1.c6af84b912394p-20), r, KC(0x1.ebfce50fac4f3p-13));  // poly_scaled: C0 / N^3, C1 / N^2
    const double r2 = r * r;
    double y = fma(KC(0x1.62e42ff0c52d6p-6), r, 1.0);                                // C2 / N
    y = fma(zz, r2, y);
    y = y * sc;
    return (float)y;
}

AIC_DEV void cb_add(ColorBuf &b, float s0, float s1, float s2, float st) {  // :87-92
    b.l0 += s0 * b.t;
    b.l1 += s1 * b.t;
    b.l2 += s2 * b.t;
    b.t *= st;
}
AIC_DEV bool cb_opaque(const ColorBuf &b) { return b.t < 1.0f / 256.0f; }  // :105-109

}  // namespace aic
