// aic_light_rays.h -- the light-ray records of include/aic_hip.h's aic_light_rays: the kernarg of its kernels, their launchers
// (aic_light_rays.hip). What the context's side (aic_light_rays_host.cpp) takes from the light updater's host code -- the effective tree of a
// maximum_distance and the derived properties of the layer's blocks -- is declared in aic_light_host.h. The kernarg is this file's own: aic_light.o does
// not change with it.
#pragma once

#include "aic_light.h"
#include "aic_light_rays_lines.h"

namespace aic {

// what a cube's walk leaves for the scan
struct LightRayResult {
    uint32_t texel, cost, flags, pad;
};

struct LightRaysParams {
    // the scene
    const uint16_t *grid;
    uint32_t index_mask;
    const uint32_t *light;
    const DevDerived *derived;
    const float *lut;
    int32_t lo[3], size[3];
    uint32_t block_sky[7];
    // the effective tree of the call's maximum_distance, in pre-order (aic_light.h)
    const DevTreePos *tree;
    const float *child_w;      // [n_tree][6][6]
    const uint2 *child_ent;    // [n_tree][6]: {position | .., cube offset}; position 0 = no child
    uint32_t n_tree;
    // the batch
    const int32_t *cubes;      // [n][3]
    uint32_t n;
    uint32_t bound;            // aic_light_rays_bound(maximum_distance): the row length of `positions`
    uint32_t capacity;
    LightRayResult *results;   // [n]
    uint32_t *counts;          // [n] n_rays
    uint32_t *offsets;         // [n] first_ray
    uint32_t *positions;       // [n][bound]: the tree positions of a cube's records, ascending
    aic_light_cube_info *infos;  // [n]
    unsigned long long *totals;  // [4]: records of the batch, stored cubes, stored records, 0
    // per workgroup of the walk
    float4 *slots;             // [workgroups][4 * n_tree]: (incoming r, g, b; ray weight) by recursion-order number
    uint2 *queue;              // [workgroups][n_tree]: {tree position, alpha it is entered with}
    // the emitters
    aic_light_ray *rays;       // the stored records
    aic_line_vertex *lines;
    uint32_t n_stored, n_stored_rays;  // (read back from `totals` between the scan and the emitters)
    LightRayAngles angles;
};

// LDS words of the walk's two bitmaps: 4 bits a tree position for the terms, 1 for the records
inline uint32_t light_rays_bitmap_words(uint32_t n_tree) { return (4u * n_tree + 31u) / 32u + (n_tree + 31u) / 32u; }
constexpr uint32_t kLightRaysBlock = 256;

hipError_t launch_light_rays_walk(const LightRaysParams &p, uint32_t workgroups, hipStream_t stream);
hipError_t launch_light_rays_scan(const LightRaysParams &p, hipStream_t stream);
hipError_t launch_light_rays_emit(const LightRaysParams &p, hipStream_t stream);

}  // namespace aic
