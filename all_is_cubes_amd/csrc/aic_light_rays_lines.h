// aic_light_rays_lines.h -- impl Wireframe for LightUpdateCubeInfo (all-is-cubes/src/space/light/debug.rs:50-95) one line at a time, written once for
// the two makers of include/aic_hip.h's aic_light_rays lines: aic_light_rays_wireframe on the host and the emitter kernel of aic_light_rays.hip, a
// thread per line. f64 in the reference's order, one rounding per operation (both translation units are built with -ffp-contract=off; sqrt and the
// division are correctly rounded on both sides), so the two write the same bytes. DESIGN.md 4.21 states the rules.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/aic_hip.h"

#if defined(__HIPCC__)
#define AIC_LR_FN __host__ __device__ inline
#else
#define AIC_LR_FN inline
#endif

namespace aic {

constexpr uint32_t kLightRayBoxLines = 12, kLightRayArrowLines = 17, kLightRayLines = kLightRayBoxLines + kLightRayArrowLines;

// sin and cos of k * (TAU / 8), k = 0..8, from the host's C library (Ray::wireframe_points' `ang`): [k][0] sin, [k][1] cos
struct LightRayAngles { double sc[9][2]; };

AIC_LR_FN void light_ray_put(aic_line_vertex *v, double x, double y, double z, float r, float g, float b) {
    v->position[0] = (float)x; v->position[1] = (float)y; v->position[2] = (float)z;
    v->color[0] = r; v->color[1] = g; v->color[2] = b; v->color[3] = 1.f;
}

// edge e of cube.aab().expand(d) in Aab::wireframe_points' order (aab.rs:569-588): pairs of octants, a set bit = the upper bound on that axis
// (bit 2 x, 1 y, 0 z), the pairs {0,1} {2,3} {4,5} {6,7} {0,2} {1,3} {4,6} {5,7} {0,4} {1,5} {2,6} {3,7}; colour Rgba(0.8, 0.8, 1.0, 1.0)
AIC_LR_FN void light_ray_box_edge(const int32_t cube[3], double d, uint32_t e, aic_line_vertex out[2]) {
    const uint32_t step = e < 4u ? 1u : (e < 8u ? 2u : 4u);
    const uint32_t i = e & 3u;
    const uint32_t first = e < 4u ? 2u * i : (e < 8u ? (i & 1u) + 4u * (i >> 1) : i);
    for (uint32_t end = 0; end < 2u; end++) {
        const uint32_t corner = first + end * step;
        double p[3];
        for (int a = 0; a < 3; a++) {
            const bool upper = (corner >> (2 - a)) & 1u;
            p[a] = upper ? ((double)cube[a] + 1.0) + d : (double)cube[a] - d;
        }
        light_ray_put(&out[end], p[0], p[1], p[2], 0.8f, 0.8f, 1.0f);
    }
}

AIC_LR_FN double light_ray_length(const double v[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
AIC_LR_FN void light_ray_cross(const double a[3], const double o[3], double out[3]) {
    out[0] = a[1] * o[2] - a[2] * o[1];
    out[1] = a[2] * o[0] - a[0] * o[2];
    out[2] = a[0] * o[1] - a[1] * o[0];
}

// line q (0..16) of Ray::wireframe_points (ray.rs:115-158) for Ray::new(lit.center(), hit_point - lit.center()), hit_point the midpoint of the trigger
// and value cubes' centres (exact in f64; never the lit cube's centre, so the length is positive): 0 the shaft, then for step 0..7 the lines
// [circle_point, tip] and [circle_point, adj_circle_point] of the arrowhead's cone.
AIC_LR_FN void light_ray_arrow_line(const int32_t lit[3], const aic_light_ray &ray, const LightRayAngles &ang, uint32_t q, aic_line_vertex out[2]) {
    double origin[3], dir[3], tip[3];
    for (int a = 0; a < 3; a++) {
        origin[a] = (double)lit[a] + 0.5;
        const double hit = ((double)ray.trigger_cube[a] + 0.5) * 0.5 + ((double)ray.value_cube[a] + 0.5) * 0.5;  // lerp(.., 0.5)
        dir[a] = hit - origin[a];
        tip[a] = origin[a] + dir[a];
    }
    const float r = ray.light_from_struck_face[0], g = ray.light_from_struck_face[1], b = ray.light_from_struck_face[2];
    if (q == 0u) {
        light_ray_put(&out[0], origin[0], origin[1], origin[2], r, g, b);
        light_ray_put(&out[1], tip[0], tip[1], tip[2], r, g, b);
        return;
    }
    const double length = light_ray_length(dir);
    double norm[3], base[3];
    for (int a = 0; a < 3; a++) norm[a] = dir[a] / length;
    const double head_length = fmin(length * 0.25, 0.125);
    const double head_width = head_length * 0.25;
    for (int a = 0; a < 3; a++) base[a] = tip[a] - norm[a] * head_length;
    const double up[3] = {0., 1., 0.}, right[3] = {1., 0., 0.};
    double perp1[3], perp2[3];
    light_ray_cross(norm, up, perp1);
    if (fabs(light_ray_length(perp1) - 1.0) > 1e-2) light_ray_cross(norm, right, perp1);  // parallel-to-up directions
    light_ray_cross(norm, perp1, perp2);
    const uint32_t step = (q - 1u) >> 1;
    double circle[2][3];  // circle_point of step and of step + 1
    for (uint32_t s = 0; s < 2u; s++)
        for (int a = 0; a < 3; a++) circle[s][a] = (base[a] + (perp1[a] * head_width) * ang.sc[step + s][0]) + (perp2[a] * head_width) * ang.sc[step + s][1];
    light_ray_put(&out[0], circle[0][0], circle[0][1], circle[0][2], r, g, b);
    if ((q - 1u) & 1u) light_ray_put(&out[1], circle[1][0], circle[1][1], circle[1][2], r, g, b);
    else light_ray_put(&out[1], tip[0], tip[1], tip[2], r, g, b);
}

// line j (0 .. 12 + 29 n_rays) of the cube's wireframe; `rays` are the cube's own records
AIC_LR_FN void light_rays_line(const int32_t cube[3], const aic_light_ray *rays, const LightRayAngles &ang, uint32_t j, aic_line_vertex out[2]) {
    if (j < kLightRayBoxLines) {
        light_ray_box_edge(cube, 0.1, j, out);
        return;
    }
    const uint32_t r = (j - kLightRayBoxLines) / kLightRayLines, q = (j - kLightRayBoxLines) % kLightRayLines;
    if (q < kLightRayBoxLines) light_ray_box_edge(rays[r].value_cube, 0.01, q, out);
    else light_ray_arrow_line(cube, rays[r], ang, q - kLightRayBoxLines, out);
}

}  // namespace aic
