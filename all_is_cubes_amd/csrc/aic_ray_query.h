// aic_ray_query.h -- what the one-lane-per-ray kernels (aic_exposure.hip, aic_cursor_raycast.hip) share on the device. Included by those two alone: the
// trace kernels' code object is not involved.
//   query_ray         ray i of [n][6] doubles (origin xyz, direction xyz). The lanes past the end read the last ray again and store nothing: the
//                     Raycaster's set-up asks the whole wave questions.
//   query_light_grid  the light grid of a flat kernarg with light, lo, size and block_sky (ExposureParams, CursorRaycastParams)
//   cube_behind       RaycastStep::cube_behind and get_light of it: cube_ahead + the normal of the face crossed (Within: the cube itself; faces NX NY NZ
//                     PX PY PZ = 1..6), and the texel there -- inside the bounds the light volume's, at `index` of the Z-major grid (below 2^30:
//                     aic_upload_space; 0 outside), outside them BlockSky::light_outside.
#pragma once

#include "aic_lightmath.h"
#include "aic_raycast.h"

namespace aic {

AIC_DEV const double *query_ray(const double *rays, uint32_t n, uint32_t i) { return rays + 6u * (size_t)(i < n ? i : n - 1u); }

template <typename Params>
AIC_DEV LightGridView query_light_grid(const Params &p) {
    LightGridView G;
    G.light = p.light;
    G.lo_x = p.lo[0]; G.lo_y = p.lo[1]; G.lo_z = p.lo[2];
    G.size_x = p.size[0]; G.size_y = p.size[1]; G.size_z = p.size[2];
    G.sky_nx = p.block_sky[0]; G.sky_ny = p.block_sky[1]; G.sky_nz = p.block_sky[2];
    G.sky_px = p.block_sky[3]; G.sky_py = p.block_sky[4]; G.sky_pz = p.block_sky[5]; G.sky_mean = p.block_sky[6];
    return G;
}

struct CubeBehind { int x, y, z; bool inside; uint32_t index, texel; };
AIC_DEV CubeBehind cube_behind(const Lvl &s, const LightGridView &G) {
    const int face = lvl_face(s);
    const int sign = face == FACE_WITHIN ? 0 : (face > 3 ? 1 : -1);
    const int face_axis = face > 3 ? face - 4 : face - 1;
    CubeBehind b;
    b.x = (int)((uint32_t)s.cx + (uint32_t)(face_axis == 0 ? sign : 0));
    b.y = (int)((uint32_t)s.cy + (uint32_t)(face_axis == 1 ? sign : 0));
    b.z = (int)((uint32_t)s.cz + (uint32_t)(face_axis == 2 ? sign : 0));
    const uint32_t sy = (uint32_t)G.size_y, sz = (uint32_t)G.size_z;
    const uint32_t ex = (uint32_t)b.x - (uint32_t)G.lo_x, ey = (uint32_t)b.y - (uint32_t)G.lo_y, ez = (uint32_t)b.z - (uint32_t)G.lo_z;
    b.inside = (ex < (uint32_t)G.size_x) & (ey < sy) & (ez < sz);
    b.index = b.inside ? (ex * sy + ey) * sz + ez : 0u;
    b.texel = G.light[b.index];
    if (!b.inside) b.texel = lm_light_outside(G, b.x, b.y, b.z);
    return b;
}

}  // namespace aic
