// aic_cursor_raycast.hip -- the kernel behind aic_cursor_raycast: cursor_raycast (all-is-cubes/src/character/cursor.rs:26-107) for a batch of rays, one
// lane per ray. Its own translation unit with its own kernarg (aic_cursor_raycast.h): the trace kernels' code object and their DevLayer / DevFrame are
// not involved.
//
//   direction = direction.normalize()
//   for step in Raycaster(o, d).within(bounds, include_exit = false):
//       if step.t_distance() > maximum_distance:            -> None
//       block = the block at step.cube_ahead()
//       if !block.attributes().selectable:                  continue
//       single voxel:  if !voxel.selectable continue;       face_selected = step.face()
//       else:          for vstep in step.recursive_raycast(ray, resolution, voxel bounds):      (within(voxel bounds, include_exit = true))
//                          face_selected = face_selected or vstep.face()
//                          the first vstep whose cube holds a selectable voxel is the hit        (the exit step holds none)
//                      no such vstep:                       continue
//       -> Cursor { step.face(), face_selected, step.intersection_point(ray), new_clamped(step.t_distance()), hit, preceding }
//   -> None
//
// "selectable" is one bit per block (DevBlock::pad[0], for a single-voxel block already ANDed with its voxel's) and one float per palette entry
// (DevPaletteEntry::pad), both made by convert_block on the host. The Raycaster is the trace kernels' own (aic_raycast.h). Wave64, no LDS: the cursor
// of a displayed frame is one or two rays, so what the call costs is the launch and the latency of some tens of dependent lookups; a batch fills waves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_cursor_raycast.h"
#include "aic_ray_query.h"

namespace aic {

__global__ void __launch_bounds__(64) cursor_raycast_kernel(const CursorRaycastParams p) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const double *ray = query_ray(p.rays, p.n, i);
    const double ox = ray[0], oy = ray[1], oz = ray[2];
    // Vector3D::normalize: self / self.length(), length = sqrt(x * x + y * y + z * z)
    const double len = sqrt(ray[3] * ray[3] + ray[4] * ray[4] + ray[5] * ray[5]);
    const double dx = ray[3] / len, dy = ray[4] / len, dz = ray[5] / len;

    const int lox = p.lo[0], loy = p.lo[1], loz = p.lo[2];
    const uint32_t sx = (uint32_t)p.size[0], sy = (uint32_t)p.size[1], sz = (uint32_t)p.size[2];
    const int hix = lox + (int)sx, hiy = loy + (int)sy, hiz = loz + (int)sz;  // (fits: aic_upload_space checks lo + size)
    const LightGridView G = query_light_grid(p);

    aic_cursor_hit rec = {};  // None: all zero

    const RayDir rd = raydir_init(dx, dy, dz);
    const double half_over_len = 0.5 / sqrt(rd.dx * rd.dx + rd.dy * rd.dy + rd.dz * rd.dz);
    const LvlLim ll = lvl_init(ox, oy, oz, rd, true, lox, loy, loz, hix, hiy, hiz, false, half_over_len);
    Lvl s = ll.s;
    // a ray within the bounds crosses at most size_x + size_y + size_z cube faces: a definite trip bound
    const uint32_t max_steps = sx + sy + sz + 3u;
    for (uint32_t step = 1; step <= max_steps; step++) {
        const NextResult nr = lvl_next(s, ll.lim, rd, lox, loy, loz, hix, hiy, hiz);
        s = nr.s;
        if (!nr.got) break;
        if (s.last_t > p.maximum_distance) break;
        const uint32_t ax = (uint32_t)s.cx - (uint32_t)lox, ay = (uint32_t)s.cy - (uint32_t)loy, az = (uint32_t)s.cz - (uint32_t)loz;
        if (!((ax < sx) & (ay < sy) & (az < sz))) continue;  // (a cube outside the bounds reads as AIR, which is unselectable)
        const size_t cube_index = ((size_t)ax * sy + ay) * sz + az;
        const uint32_t block = (uint32_t)p.pool[cube_index] & p.index_mask;
        const DevBlock *b = &p.blocks[block];
        if (!(b->pad[0] & kBlockSelectable)) continue;
        const uint32_t resolution = b->kind & 255u;  // 0: a single voxel, and the bit has decided it
        int face_selected = lvl_face(s);
        int vlx = 0, vly = 0, vlz = 0, vsx = 1, vsy = 1, vsz = 1, hvx = 0, hvy = 0, hvz = 0;
        if (resolution != 0u) {
            const uint32_t vlo = b->vlo_packed, vsize = b->vsize_packed, vox_off = b->vox_off, pal_off = b->pal_off;
            vlx = (int)(vlo & 255u); vly = (int)((vlo >> 8) & 255u); vlz = (int)((vlo >> 16) & 255u);
            vsx = (int)(vsize & 255u); vsy = (int)((vsize >> 8) & 255u); vsz = (int)((vsize >> 16) & 255u);
            const int vhx = vlx + vsx, vhy = vly + vsy, vhz = vlz + vsz;
            const LvlLim il = lvl_init_recursive(ox, oy, oz, s.cx, s.cy, s.cz, (double)resolution, rd, vlx, vly, vlz, vhx, vhy, vhz, half_over_len);
            Lvl v = il.s;
            bool first = true, found = false;
            const uint32_t max_sub = (uint32_t)(vsx + vsy + vsz) + 3u;
            for (uint32_t sub = 0; sub < max_sub; sub++) {
                const NextResult vr = lvl_next(v, il.lim, rd, vlx, vly, vlz, vhx, vhy, vhz);
                v = vr.s;
                if (!vr.got) break;
                if (first) face_selected = lvl_face(v);  // the face of the voxel bounds the ray met, whatever lies in that voxel
                first = false;
                const uint32_t ux = (uint32_t)(v.cx - vlx), uy = (uint32_t)(v.cy - vly), uz = (uint32_t)(v.cz - vlz);
                // get_opt_evoxel: the exit step, and any cube outside the stored volume, holds no voxel
                if (vr.is_exit | !((ux < (uint32_t)vsx) & (uy < (uint32_t)vsy) & (uz < (uint32_t)vsz))) continue;
                const uint32_t code = p.pool[(size_t)vox_off + (ux * (uint32_t)vsy + uy) * (uint32_t)vsz + uz];
                if (p.palette[pal_off + code].pad != 0.f) {
                    found = true;
                    hvx = v.cx; hvy = v.cy; hvz = v.cz;
                    break;
                }
            }
            if (!found) continue;
        }
        // a Cursor
        const int face = lvl_face(s);
        double point[3];
        intersection_point(s, ox, oy, oz, dx, dy, dz, point);
        rec.cursor.cube[0] = s.cx; rec.cursor.cube[1] = s.cy; rec.cursor.cube[2] = s.cz;
        rec.cursor.face_entered = face;
        rec.cursor.face_selected = face_selected;
        rec.cursor.point_entered[0] = point[0]; rec.cursor.point_entered[1] = point[1]; rec.cursor.point_entered[2] = point[2];
        rec.cursor.distance_to_point = s.last_t > 0.0 ? s.last_t : 0.0;  // PositiveSign::new_clamped
        rec.cursor.voxel_lo[0] = vlx; rec.cursor.voxel_lo[1] = vly; rec.cursor.voxel_lo[2] = vlz;
        rec.cursor.voxel_size[0] = vsx; rec.cursor.voxel_size[1] = vsy; rec.cursor.voxel_size[2] = vsz;
        rec.cursor.resolution = resolution != 0u ? (int)resolution : 1;
        rec.hit = 1;
        rec.block_index = block;
        rec.voxel[0] = hvx; rec.voxel[1] = hvy; rec.voxel[2] = hvz;
        rec.steps = step;
        const uint32_t th = p.light[cube_index];
        rec.light_hit[0] = (uint8_t)th; rec.light_hit[1] = (uint8_t)(th >> 8); rec.light_hit[2] = (uint8_t)(th >> 16); rec.light_hit[3] = (uint8_t)(th >> 24);
        if (face != FACE_WITHIN) {
            const CubeBehind b = cube_behind(s, G);
            const uint32_t tp = b.texel;
            rec.has_preceding = 1;
            rec.preceding_cube[0] = b.x; rec.preceding_cube[1] = b.y; rec.preceding_cube[2] = b.z;
            rec.preceding_block_index = b.inside ? ((uint32_t)p.pool[b.index] & p.index_mask) : AIC_CURSOR_NO_BLOCK;
            rec.light_preceding[0] = (uint8_t)tp; rec.light_preceding[1] = (uint8_t)(tp >> 8); rec.light_preceding[2] = (uint8_t)(tp >> 16);
            rec.light_preceding[3] = (uint8_t)(tp >> 24);
        }
        break;
    }
    if (i < p.n) p.out[i] = rec;
}

hipError_t launch_cursor_raycast(const CursorRaycastParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(cursor_raycast_kernel, dim3(cursor_raycast_groups(p.n)), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace aic
