// aic_light_arith.h -- the f32 arithmetic of Space::compute_light that the light updater's gather kernel (aic_light.hip) and the light-ray records
// (aic_light_rays.hip) both need, each rule once: PositiveSign's clamps, the correctly rounded log2f behind PackedLight::scalar_in, and the face normals.
// Device code only; every user is built with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aic {
namespace {

// ---- PositiveSign / ZeroOne arithmetic (math/restricted_number.rs:240-326) ----
__device__ __forceinline__ float ps_new_clamped(float v) { return v > 0.f ? v : 0.f; }
__device__ __forceinline__ float ps_mul(float a, float b) {
    const float v = a * b;
    return (v != v) ? 0.f : v;
}

// ---- log2f: the table-driven routine of ARM optimized-routines as shipped in glibc >= 2.27 and musl
// (what f32::log2 calls on Linux): 16-entry table of 1/c and log2(c), degree-4 polynomial, double arithmetic.
__device__ const double kLog2Tab[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
    {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
    {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
    {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
    {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
    {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2}};

__device__ float log2f_exact(float x) {
    uint32_t ix = __float_as_uint(x);
    if (ix == 0x3f800000u) return 0.f;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        if (ix * 2u == 0u) return -__builtin_inff();
        if (ix == 0x7f800000u) return x;
        if ((ix & 0x80000000u) || ix * 2u >= 0xff000000u) return __builtin_nanf("");
        ix = __float_as_uint(x * 0x1p23f);  // subnormal: normalise
        ix -= 23u << 23;
    }
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) % 16u);
    const uint32_t top = tmp & 0xff800000u;
    const uint32_t iz = ix - top;
    const int k = (int32_t)tmp >> 23;
    const double invc = kLog2Tab[i][0], logc = kLog2Tab[i][1];
    const double z = (double)__uint_as_float(iz);
    const double r = z * invc - 1.0;
    const double y0 = logc + (double)k;
    const double r2 = r * r;
    double y = -0x1.712b6f70a7e4dp-2 * r2 + (0x1.ecabf496832ep-2 * r + -0x1.715479ffae3dep-1);
    const double p = 0x1.715475f35c8b8p0 * r + y0;
    y = y * r2 + p;
    return (float)y;
}

// data.rs:214-218 PackedLight::scalar_in: (log2(v) * 10 + 144).round() as u8 (saturating, NaN -> 0)
__device__ __forceinline__ uint32_t packed_scalar_in(float value) {
    const float x = roundf(log2f_exact(value) * 10.0f + 144.0f);
    if (x != x) return 0u;
    if (x <= 0.f) return 0u;
    if (x >= 255.f) return 255u;
    return (uint32_t)x;
}

__device__ __forceinline__ void normal_of(int f, int n[3]) {  // f: 0 nx 1 ny 2 nz 3 px 4 py 5 pz
    n[0] = n[1] = n[2] = 0;
    n[f >= 3 ? f - 3 : f] = f >= 3 ? 1 : -1;
}

}  // namespace
}  // namespace aic
