// aic_exposure_state.cpp -- the host-only half of automatic exposure: aic_exposure_init, aic_exposure_rays and aic_exposure_advance restate what
// character::exposure::State::step (all-is-cubes/src/character/exposure.rs:60-151) does around its sampling loop, in the reference's number formats and
// order of operations (built with -ffp-contract=off). No device, no context: a C host, the C++ mirror and the Rust shim get the same bits from here.
#include <cmath>

#include "../../include/aic_hip.h"

namespace {

const float kTargetLuminance = 0.9f;       // TARGET_LUMINANCE
const float kAdjustmentStrength = 0.375f;  // ADJUSTMENT_STRENGTH
const float kExposureChangeRate = 2.0f;    // EXPOSURE_CHANGE_RATE

// f32::ln and f32::exp: evaluated in f64 and rounded once, which is the correctly rounded f32 result but for arguments astronomically close to a
// rounding boundary, and the same bits on every host whose f64 log / exp are the usual ones (a libm's logf / expf promise less than that)
float ln_f32(float x) { return (float)std::log((double)x); }
float exp_f32(float x) { return (float)std::exp((double)x); }

// f32::clamp: NaN stays NaN
float clamp_f32(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// compute_target_exposure (exposure.rs:145-151)
float target_exposure(float luminance) {
    const float derived_exposure = clamp_f32(kTargetLuminance / luminance, 0.1f, 4.f);
    return derived_exposure * kAdjustmentStrength + 1.f * (1.f - kAdjustmentStrength);
}

// State::luminance_average (exposure.rs:139-142): the f32 sum in index order (from -0.0, the identity `Sum for f32` folds from) times 100f32.recip()
float luminance_average(const aic_exposure_state *s) {
    float sum = -0.0f;
    for (int i = 0; i < AIC_EXPOSURE_SAMPLES; i++) sum += s->luminance_samples[i];
    return sum * (1.0f / (float)AIC_EXPOSURE_SAMPLES);
}

}  // namespace

extern "C" {

int aic_exposure_init(aic_exposure_state *s) {
    if (!s) return AIC_ERR_INVALID;
    for (float &v : s->luminance_samples) v = 1.0f;
    s->luminance_sample_index = 0;
    s->exposure_log = 0.0f;
    return AIC_OK;
}

int aic_exposure_rays(const double rotation_ijkr[4], const double translation[3], uint32_t first_index, uint32_t n, double *rays) {
    if (!rotation_ijkr || !translation || (n && !rays)) return AIC_ERR_INVALID;
    // ViewTransform::to_transform(): Rotation3D::to_transform() then the translation, which lands in m41..m43 (as the host mirror's
    // Camera::compute_matrices restates it); row-vector convention, m[r][c] = m(r+1)(c+1)
    const double qi = rotation_ijkr[0], qj = rotation_ijkr[1], qk = rotation_ijkr[2], qr = rotation_ijkr[3];
    const double i2 = qi + qi, j2 = qj + qj, k2 = qk + qk;
    const double ii = qi * i2, ij = qi * j2, ik = qi * k2, jj = qj * j2, jk = qj * k2, kk = qk * k2;
    const double ri = qr * i2, rj = qr * j2, rk = qr * k2;
    const double m[4][4] = {{1.0 - (jj + kk), ij + rk, ik - rj, 0.0},
                            {ij - rk, 1.0 - (ii + kk), jk + ri, 0.0},
                            {ik + rj, jk - ri, 1.0 - (ii + jj), 0.0},
                            {translation[0], translation[1], translation[2], 1.0}};
    // transform_point3d(origin): the homogeneous product, then the division by w (which is 1: `None`, w <= 0, cannot happen)
    const double px = 0.0, py = 0.0, pz = 0.0;
    const double hx = px * m[0][0] + py * m[1][0] + pz * m[2][0] + m[3][0];
    const double hy = px * m[0][1] + py * m[1][1] + pz * m[2][1] + m[3][1];
    const double hz = px * m[0][2] + py * m[1][2] + pz * m[2][2] + m[3][2];
    const double hw = px * m[0][3] + py * m[1][3] + pz * m[2][3] + m[3][3];
    const double origin[3] = {hx / hw, hy / hw, hz / hw};
    const double sqrtedge = std::sqrt((double)AIC_EXPOSURE_SAMPLES);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t index = (uint32_t)(((uint64_t)first_index + k) % AIC_EXPOSURE_SAMPLES);
        const double indexf = (double)index;
        // f64::rem_euclid and f64::div_euclid of a non-negative value by a positive one: fmod, and the truncated quotient
        const double vx = std::fmod(indexf, sqrtedge) / sqrtedge * 2. - 1.;
        const double vy = std::trunc(indexf / sqrtedge) / sqrtedge * 2. - 1.;
        const double vz = -1.0;
        double *r = rays + 6 * (size_t)k;
        r[0] = origin[0]; r[1] = origin[1]; r[2] = origin[2];
        // transform_vector3d: no translation
        r[3] = vx * m[0][0] + vy * m[1][0] + vz * m[2][0];
        r[4] = vx * m[0][1] + vy * m[1][1] + vz * m[2][1];
        r[5] = vx * m[0][2] + vy * m[1][2] + vz * m[2][2];
    }
    return AIC_OK;
}

int aic_exposure_advance(aic_exposure_state *s, uint32_t n, const float *samples, double dt, float *exposure) {
    if (!s || n > AIC_EXPOSURE_SAMPLES || (n && !samples) || s->luminance_sample_index >= AIC_EXPOSURE_SAMPLES) return AIC_ERR_INVALID;
    if (dt != 0.) {  // (the reference returns before it samples)
        for (uint32_t k = 0; k < n; k++) {
            s->luminance_sample_index = (s->luminance_sample_index + 1u) % AIC_EXPOSURE_SAMPLES;
            s->luminance_samples[s->luminance_sample_index] = samples[k];
        }
        const float target = target_exposure(luminance_average(s));
        if (std::isfinite(target)) {
            const float delta_log = ln_f32(target) - s->exposure_log;
            s->exposure_log += delta_log * (float)dt * kExposureChangeRate;
        }
    }
    if (exposure) *exposure = exp_f32(s->exposure_log);
    return AIC_OK;
}

}  // extern "C"
