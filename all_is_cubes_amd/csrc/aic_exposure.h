// aic_exposure.h -- the luminance sampler of automatic exposure (aic_exposure.hip) as the host ABI code sees it: the parameter struct and the launch.
//
// aic_sample_luminance restates the sampling loop of character::exposure::State::step (all-is-cubes/src/character/exposure.rs:91-128) for a batch of
// rays: one lane per ray walks the cube grid with the device Raycaster (aic_raycast.h) until a visible block lies ahead whose texel behind is Visible, and
// leaves that texel's luminance, or the sky's. DESIGN.md 4.16 has the arithmetic; tests/exposure_ref.py is that text in NumPy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aic {

// The sampler's own kernarg (the trace kernels' DevLayer / DevFrame are not touched): everything a lane reads that is uniform, by value.
struct ExposureParams {
    const uint16_t *grid;     // the layer's cube grid: block index per cube, Z-major (the start of DevLayer::pool)
    const uint32_t *light;    // the layer's current light volume
    const uint32_t *visible;  // one bit per block index: EvaluatedBlock::visible() (NOT the block's class: see aic_exposure_visible_bits)
    const float *lut;         // PackedLight decode table, 256 floats
    const double *rays;       // [n][6] origin xyz, direction xyz
    float *out;               // [n]
    int32_t lo[3], size[3];
    uint32_t index_mask;      // a grid entry's block index = entry & index_mask (kCubeIndexMask when the entries carry tags, else 0xffff)
    uint32_t n, max_steps;
    int32_t sky_kind;         // 0 Sky::Uniform(sky[0]), 1 Sky::Octants
    float sky[8][3];
    uint32_t block_sky[7];    // BlockSky texels: nx ny nz px py pz mean
};

// Queues the sampler on `stream`; n is not zero.
hipError_t launch_sample_luminance(const ExposureParams &p, hipStream_t stream);

}  // namespace aic
