// aic_cursor_raycast.h -- the cursor raycast (aic_cursor_raycast.hip) as the host ABI code sees it: the parameter struct and the launch.
//
// aic_cursor_raycast restates cursor_raycast (all-is-cubes/src/character/cursor.rs:26-107) for a batch of rays: one lane per ray walks the cube grid with
// the device Raycaster (aic_raycast.h) until a selectable block lies ahead -- for a block with voxels, until the sub-ray of
// RaycastStep::recursive_raycast meets a selectable voxel -- and leaves one aic_cursor_hit. DESIGN.md 4.18 has the rule; tests/cursor_ref.py is that
// text in Python.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aic_hip.h"
#include "aic_device.h"

namespace aic {

// The raycast's own kernarg (the trace kernels' DevLayer / DevFrame are not touched): everything a lane reads that is uniform, by value.
struct CursorRaycastParams {
    const uint16_t *pool;            // the layer's u16 pool: the cube grid (block index per cube, Z-major) at 0, then the blocks' voxel volumes
    const uint32_t *light;           // the layer's current light volume
    const DevBlock *blocks;          // pad[0] & kBlockSelectable, and where a block's voxels and palette are
    const DevPaletteEntry *palette;  // pad: the voxel's Evoxel::selectable as 1.0f / 0.0f
    const double *rays;              // [n][6] origin xyz, direction xyz
    aic_cursor_hit *out;             // [n]
    double maximum_distance;
    int32_t lo[3], size[3];
    uint32_t index_mask;             // a grid entry's block index = entry & index_mask (kCubeIndexMask when the entries carry tags, else 0xffff)
    uint32_t n;
    uint32_t block_sky[7];           // BlockSky texels: nx ny nz px py pz mean
};

// One lane per ray in workgroups of one wave: the launch's grid
inline uint32_t cursor_raycast_groups(uint32_t n) { return (n + 63u) / 64u; }
// Queues the raycast on `stream`, ONE launch of cursor_raycast_groups(n) workgroups; n is not zero.
hipError_t launch_cursor_raycast(const CursorRaycastParams &p, hipStream_t stream);

}  // namespace aic
