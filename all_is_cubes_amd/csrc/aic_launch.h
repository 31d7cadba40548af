// aic_launch.h -- the kernels of the aic_trace.hip translation unit as the host code sees them: one declaration of every launcher. Included by the
// files that define them (aic_trace.hip, aic_scene_kernels.h, aic_probe_kernels.h), by the host code that calls them (aic_abi.cpp, aic_frame.cpp)
// and by the recording stand-in of tools/submit_record. Every launcher queues on `stream` and returns; none synchronises.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>

#include "aic_device.h"

namespace aic {

// ---- the image kernel (aic_trace.hip)
// Picks the trace_image_kernel instantiation from the frame's options (transparency, lighting, block-table size, `diag`: per-pixel records) and
// DevFrame::exchange, and sizes the persistent grid.
void launch_trace_image(const DevFrame &F, bool diag, hipStream_t stream);
// DevFrame::ray_cold of the exchanging variants (antialiased frames): bytes for the resident grid of a device of `n_cus` CUs; *groups = that grid.
size_t trace_ray_cold_bytes(uint32_t n_cus, uint32_t *groups);

// ---- scene maintenance and frame bookkeeping (aic_scene_kernels.h)
void launch_scatter_cubes(uint16_t *grid, uint32_t *light, const int32_t *xyz, const uint16_t *bi, const uint32_t *lt,
                          uint32_t n, const int lo[3], const int size[3], const uint32_t *cls, hipStream_t stream);
void launch_tag_cubes(uint16_t *grid, size_t n, const uint32_t *cls, int from_tagged, int to_tagged, hipStream_t stream);
// the OPEN tags (aic_device.h) of a tagged grid: all of them, behind launch_tag_cubes; those of `n` changed cubes (xyz: device memory) and their neighbours, behind the scatter
void launch_open_cubes(uint16_t *grid, const int size[3], hipStream_t stream);
void launch_open_changed_cubes(uint16_t *grid, const int32_t *xyz, uint32_t n, const int lo[3], const int size[3], hipStream_t stream);
void launch_order_tiles(const uint32_t *cost, uint32_t *order, uint32_t n_tiles, uint32_t macros_x, uint32_t sb_shift, uint32_t n_queues, uint32_t *queue_start,
                        hipStream_t stream, bool clear_cost = false, uint32_t *clear_words = nullptr, uint32_t n_clear_words = 0);
// the same for the frames of a batch, one workgroup each, in ONE launch (OrderJobs: aic_device.h)
void launch_order_tiles_jobs(const OrderJobs &jobs, uint32_t n_jobs, uint32_t n_tiles, uint32_t macros_x, uint32_t sb_shift, uint32_t n_queues, hipStream_t stream,
                             bool clear_cost, uint32_t n_clear_words);
void launch_assemble_strips(const uint32_t *gathered, uint32_t *out, uint32_t w, uint32_t h, uint32_t strip_rows,
                            uint32_t n_parts, uint32_t max_rows, hipStream_t stream);

// ---- probes (aic_probe_kernels.h)
void launch_probe_raycast(const double *od, int use_bounds, const int *lohi, int include_exit, uint32_t max_steps,
                          double *out_rec, uint32_t *n_out, int *ended, hipStream_t stream);
void launch_probe_powf(const float *x, const float *y, float *out, uint32_t n, hipStream_t stream);
void launch_probe_expf(const float *x, float *out, uint32_t n, hipStream_t stream);

}  // namespace aic
