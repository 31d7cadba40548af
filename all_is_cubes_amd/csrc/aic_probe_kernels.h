// aic_probe_kernels.h -- the probe kernels behind aic_probe_raycast / aic_probe_powf / aic_probe_expf, with their launchers (part of the aic_trace.hip
// translation unit): they run the trace kernels' own device functions on inputs the tests choose, so that the Raycaster restatement (aic_raycast.h) is pinned
// against the reference's step tables (all-is-cubes-base/src/raycast/tests.rs) and powf_table / expf_table (aic_colour.h) against the host's libm.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_colour.h"
#include "aic_launch.h"
#include "aic_raycast.h"

namespace aic {

// aic_probe_raycast: the device Raycaster, one ray
__global__ void probe_raycast_kernel(const double *od, int use_bounds, const int *lohi, int include_exit, uint32_t max_steps,
                                     double *out_rec, uint32_t *n_out, int *ended) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double ox = od[0], oy = od[1], oz = od[2], dx = od[3], dy = od[4], dz = od[5];
    int lo[3] = {lohi[0], lohi[1], lohi[2]}, hi[3] = {lohi[3], lohi[4], lohi[5]};
    if (!use_bounds) {
        lo[0] = lo[1] = lo[2] = I32_MIN_ + 1;
        hi[0] = hi[1] = hi[2] = I32_MAX_ - 1;
    }
    const RayDir rd = raydir_init(dx, dy, dz);
    const LvlLim ll = lvl_init(ox, oy, oz, rd, use_bounds != 0, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], include_exit != 0,
                               0.5 / sqrt(rd.dx * rd.dx + rd.dy * rd.dy + rd.dz * rd.dz));
    Lvl s = ll.s;
    const Lim lim = ll.lim;
    uint32_t n = 0;
    *ended = 0;
    // A bounded raycaster with its exit step -- what the image kernel's events set up -- takes its first step through the events' own code
    // (lvl_first_masks), so that the reference's step tables pin that too; lvl_next goes on from the state it leaves.
    bool first_by_masks = use_bounds != 0 && include_exit != 0;
    while (n < max_steps) {
        NextResult nr;
        if (first_by_masks) {
            first_by_masks = false;
            const FirstCube f = lvl_first_masks(s, rd, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
            nr.got = f.got; nr.is_exit = false;
            nr.s.tx = f.tx; nr.s.ty = f.ty; nr.s.tz = f.tz; nr.s.last_t = f.last_t;
            nr.s.cx = f.cx; nr.s.cy = f.cy; nr.s.cz = f.cz;
            const uint32_t face = (f.lax & 8u) ? (f.lax & 7u) : (((f.lax == 0u ? rd.sx : (f.lax == 1u ? rd.sy : rd.sz)) > 0 ? 1u : 4u) + f.lax);
            // "emitted, step scheduled" as lvl_next leaves it: InBounds | pick | need_step, or Ended
            nr.s.st = (face << 2) | 256u | (f.inbounds ? (FL_INBOUNDS | ((uint32_t)pick_axis(f.tx, f.ty, f.tz) << 5) | 128u) : FL_ENDED);
        } else {
            nr = lvl_next(s, lim, rd, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
        }
        s = nr.s;
        if (!nr.got) {
            *ended = 1;
            break;
        }
        double ip[3];
        intersection_point(s, ox, oy, oz, dx, dy, dz, ip);
        double *r = out_rec + 8 * (size_t)n;
        // record: cube[3] as doubles, face, t, ip[3]
        r[0] = (double)s.cx; r[1] = (double)s.cy; r[2] = (double)s.cz;
        r[3] = (double)lvl_face(s); r[4] = s.last_t; r[5] = ip[0]; r[6] = ip[1]; r[7] = ip[2];
        n++;
    }
    *n_out = n;
}

// f32::powf evaluated in f64 and rounded once: only for the probe below, outside powf_table's domain (the trace kernel never
// leaves that domain)
AIC_DEV float powf_exact(float x, float y) { return (float)pow((double)x, (double)y); }

// aic_probe_powf: the device's powf (table path where its domain allows, as the trace kernel chooses)
__global__ void probe_powf_kernel(const float *x, const float *y, float *out, uint32_t n) {
    __shared__ double s_pow[64];
    pow_tables_to_lds(s_pow, threadIdx.x, blockDim.x);
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = powf_table_domain(x[i], y[i]) ? powf_table(x[i], y[i], s_pow) : powf_exact(x[i], y[i]);
}

// aic_probe_expf: the device's expf as distance_fog uses it (expf_table; its domain, |x| < 88, is the caller's to keep)
__global__ void probe_expf_kernel(const float *x, float *out, uint32_t n) {
    __shared__ double s_pow[64];
    pow_tables_to_lds(s_pow, threadIdx.x, blockDim.x);
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = expf_table(x[i], s_pow);
}

void launch_probe_powf(const float *x, const float *y, float *out, uint32_t n, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(probe_powf_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, x, y, out, n);
}

void launch_probe_expf(const float *x, float *out, uint32_t n, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(probe_expf_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, x, out, n);
}

void launch_probe_raycast(const double *od, int use_bounds, const int *lohi, int include_exit, uint32_t max_steps,
                          double *out_rec, uint32_t *n_out, int *ended, hipStream_t stream) {
    hipLaunchKernelGGL(probe_raycast_kernel, dim3(1), dim3(64), 0, stream, od, use_bounds, lohi, include_exit, max_steps, out_rec,
                       n_out, ended);
}

}  // namespace aic
