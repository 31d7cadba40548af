// aic_stale_rect_math.h -- the one copy of the arithmetic that turns a box of changed cubes into a screen rectangle (include/aic_hip.h under
// aic_stale_rects and aic_pick_stale_cubes): aic_stale_host.cpp runs it on the host for aic_stale_rects, aic_stale_cubes.hip
// on the device, one lane a box. All f64, one rounding an operation, in the order the header writes out: both translation units are built with
// -ffp-contract=off, and tests/stale_ref.py and tests/stale_cubes_ref.py give the same bits.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AIC_STALE_HD __host__ __device__ inline
#else
#define AIC_STALE_HD inline
#endif

namespace aic {

// A box's rectangle with both depth bounds; all fields 0: empty.
struct StaleBounds {
    uint16_t x0, y0, x1, y1;  // columns [x0, x1), rows [y0, y1)
    float dmin;               // nothing of the grown box is nearer than this depth; -inf: unknown
    float dmax;               // nothing of the grown box is farther than this depth; +inf: unknown
};

// floor(v) clamped to [0, n], for v that may be infinite (never NaN)
AIC_STALE_HD uint16_t stale_clamp_cell(double v, uint32_t n) { return v <= 0.0 ? (uint16_t)0 : (v >= (double)n ? (uint16_t)n : (uint16_t)v); }

// the f32 one step towards -inf / +inf of a d that is not NaN (std::nextafterf without the library)
AIC_STALE_HD float stale_step_down(float d) {
    const uint32_t b = __builtin_bit_cast(uint32_t, d);
    if (b == 0xFF800000u) return d;                                      // -inf stays
    if ((b << 1) == 0u) return __builtin_bit_cast(float, 0x80000001u);   // +-0: the least negative number
    return __builtin_bit_cast(float, (b >> 31) ? b + 1u : b - 1u);
}
AIC_STALE_HD float stale_step_up(float d) {
    const uint32_t b = __builtin_bit_cast(uint32_t, d);
    if (b == 0x7F800000u) return d;                                      // +inf stays
    if ((b << 1) == 0u) return __builtin_bit_cast(float, 0x00000001u);   // +-0: the least positive number
    return __builtin_bit_cast(float, (b >> 31) ? b - 1u : b + 1u);
}

// `v` rounded DOWN / UP to f32: to nearest, then a step back if that went past it
AIC_STALE_HD float stale_round_down(double v) {
    const float d = (float)v;
    return (double)d > v ? stale_step_down(d) : d;
}
AIC_STALE_HD float stale_round_up(double v) {
    const float d = (float)v;
    return (double)d < v ? stale_step_up(d) : d;
}

// The rectangle of box [lo, hi) (bounds of 32 bits, or one past them: a light cube at the i32 edge) grown by `expand` under the column-major view_projection `m`, as the header states it step by step. The eight corners are
// all projected and the "whole frame" answer overrides what they gave: no corner's result depends on another's, so this equals leaving at the first
// corner beside the camera, and the loops unroll with constant indices (registers, not scratch, on the device).
AIC_STALE_HD StaleBounds stale_bounds_of(const double *m, uint32_t width, uint32_t height, int64_t lx, int64_t ly, int64_t lz, int64_t hx, int64_t hy, int64_t hz,
                                         int32_t expand) {
    StaleBounds out = {0, 0, 0, 0, 0.f, 0.f};
    if (hx <= lx || hy <= ly || hz <= lz) return out;
    const double ex[2] = {(double)(lx - (int64_t)expand), (double)(hx + (int64_t)expand)};
    const double ey[2] = {(double)(ly - (int64_t)expand), (double)(hy + (int64_t)expand)};
    const double ez[2] = {(double)(lz - (int64_t)expand), (double)(hz + (int64_t)expand)};
    const double inf = __builtin_inf();
    double ax = inf, bx = -inf, ay = inf, by = -inf, az = inf, bz = -inf;
    bool whole = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double x = ex[k & 1], y = ey[(k >> 1) & 1], z = ez[(k >> 2) & 1];
        const double c0 = ((m[0] * x + m[4] * y) + m[8] * z) + m[12];
        const double c1 = ((m[1] * x + m[5] * y) + m[9] * z) + m[13];
        const double c2 = ((m[2] * x + m[6] * y) + m[10] * z) + m[14];
        const double c3 = ((m[3] * x + m[7] * y) + m[11] * z) + m[15];
        if (!(c3 > 0.0) || !__builtin_isfinite(c0) || !__builtin_isfinite(c1) || !__builtin_isfinite(c2) || !__builtin_isfinite(c3)) whole = true;
        const double nx = c0 / c3, ny = c1 / c3, nz = c2 / c3;
        ax = nx < ax ? nx : ax; bx = nx > bx ? nx : bx;
        ay = ny < ay ? ny : ay; by = ny > by ? ny : by;
        az = nz < az ? nz : az; bz = nz > bz ? nz : bz;
    }
    if (whole) {
        out.x1 = (uint16_t)width;
        out.y1 = (uint16_t)height;
        out.dmin = -__builtin_inff();
        out.dmax = __builtin_inff();
        return out;
    }
    const double W = (double)width, H = (double)height;
    const uint16_t x0 = stale_clamp_cell(__builtin_floor((ax + 1.0) / 2.0 * W) - 1.0, width), x1 = stale_clamp_cell(__builtin_floor((bx + 1.0) / 2.0 * W) + 2.0, width);
    const uint16_t y0 = stale_clamp_cell(__builtin_floor((1.0 - by) / 2.0 * H) - 1.0, height), y1 = stale_clamp_cell(__builtin_floor((1.0 - ay) / 2.0 * H) + 2.0, height);
    if (x0 >= x1 || y0 >= y1) return out;
    out.x0 = x0; out.y0 = y0; out.x1 = x1; out.y1 = y1;
    out.dmin = stale_round_down(az - 1.0 / 16777216.0);
    // (a least depth that overflowed to -inf says nothing about the box: neither does the greatest)
    out.dmax = out.dmin == -__builtin_inff() ? __builtin_inff() : stale_round_up(bz + 1.0 / 16777216.0);
    return out;
}

}  // namespace aic
