// aic_exposure.hip -- the luminance sampler behind aic_sample_luminance: the sampling loop of character::exposure::State::step
// (all-is-cubes/src/character/exposure.rs:91-128) for a batch of rays, one lane per ray. Its own translation unit with its own kernarg (aic_exposure.h):
// the trace kernels' code object and their DevLayer / DevFrame are not involved.
//
//   for step in Raycaster(o, d).within(bounds, include_exit = false).take(max_steps):
//       a = step.cube_ahead()
//       if a is outside the bounds:                      -> sky.sample(d).luminance()
//       elif the block at a is visible():
//           t = get_light(step.cube_behind())            (inside: the light volume; outside: BlockSky::light_outside)
//           if t.status == Visible:                      -> t.value().luminance()
//   nothing returned                                     -> sky.sample(d).luminance()
//
// The Raycaster is the trace kernels' own (aic_raycast.h, pinned to the reference's step tables by aic_probe_raycast); "visible" is one bit per block
// index made by the host from compute_derived (aic_light_derived.cpp) -- NOT the cube's class bits, which say "recursive" for a block whose voxels are all
// invisible. Wave64, no LDS: a step of automatic exposure is 10 rays, so the launch is one wave and what it costs is the launch and the latency of some
// tens of dependent lookups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_exposure.h"
#include "aic_ray_query.h"

namespace aic {

// Rgb::luminance (all-is-cubes-base/src/math/color.rs:288-297), f32 in the reference's order (built with -ffp-contract=off)
AIC_DEV float rgb_luminance(float r, float g, float b) { return g * 0.7152f + (r * 0.2126f + b * 0.0722f); }

__global__ void __launch_bounds__(64) sample_luminance_kernel(const ExposureParams p) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const double *ray = query_ray(p.rays, p.n, i);
    const double ox = ray[0], oy = ray[1], oz = ray[2], dx = ray[3], dy = ray[4], dz = ray[5];

    // Sky::sample (sky.rs:32-41) on the direction as given: -0.0 counts as positive, NaN as negative
    const uint32_t oct = p.sky_kind != 0 ? ((dx >= 0.0 ? 4u : 0u) + (dy >= 0.0 ? 2u : 0u) + (dz >= 0.0 ? 1u : 0u)) : 0u;
    float result = rgb_luminance(p.sky[oct][0], p.sky[oct][1], p.sky[oct][2]);

    const int lox = p.lo[0], loy = p.lo[1], loz = p.lo[2];
    const uint32_t sx = (uint32_t)p.size[0], sy = (uint32_t)p.size[1], sz = (uint32_t)p.size[2];
    const int hix = lox + (int)sx, hiy = loy + (int)sy, hiz = loz + (int)sz;  // (fits: aic_upload_space checks lo + size)
    const LightGridView G = query_light_grid(p);

    const RayDir rd = raydir_init(dx, dy, dz);
    const LvlLim ll = lvl_init(ox, oy, oz, rd, true, lox, loy, loz, hix, hiy, hiz, false, 0.5 / sqrt(rd.dx * rd.dx + rd.dy * rd.dy + rd.dz * rd.dz));
    Lvl s = ll.s;
    for (uint32_t step = 0; step < p.max_steps; step++) {
        const NextResult nr = lvl_next(s, ll.lim, rd, lox, loy, loz, hix, hiy, hiz);
        s = nr.s;
        if (!nr.got) break;
        const uint32_t ax = (uint32_t)s.cx - (uint32_t)lox, ay = (uint32_t)s.cy - (uint32_t)loy, az = (uint32_t)s.cz - (uint32_t)loz;
        if (!((ax < sx) & (ay < sy) & (az < sz))) break;  // the cube ahead is outside the bounds: the sky
        const uint32_t block = (uint32_t)p.grid[(ax * sy + ay) * sz + az] & p.index_mask;
        if (!((p.visible[block >> 5] >> (block & 31u)) & 1u)) continue;
        const uint32_t t = cube_behind(s, G).texel;
        if ((t >> 24) == 255u) {  // LightStatus::Visible: PackedLight::valid (light/data.rs:127-135)
            result = rgb_luminance(p.lut[t & 255u], p.lut[(t >> 8) & 255u], p.lut[(t >> 16) & 255u]);
            break;
        }
    }
    if (i < p.n) p.out[i] = result;
}

hipError_t launch_sample_luminance(const ExposureParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(sample_luminance_kernel, dim3((p.n + 63u) / 64u), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace aic
