// aic_scene_kernels.h -- the small kernels that maintain the device's copy of a scene and a frame's bookkeeping, with their launchers (part of the
// aic_trace.hip translation unit: DESIGN.md 4 says why they are not compiled on their own):
//   scatter_cubes_kernel   aic_update_cubes: SpaceChange::{CubeBlock, CubeLight} (all-is-cubes-render/src/raytracer/updating.rs:146-166)
//   tag_cubes_kernel       the tag bits of the cube grid (aic_device.h): the block classes ...
//   open_cubes_kernel, open_changed_cubes_kernel   ... and which invisible cubes are OPEN, for the whole grid / around changed cubes
//   order_tiles_kernel     the tile queues of the next frame, costliest tiles first (no counterpart in the reference: DESIGN.md 4.2)
//   assemble_strips_kernel aic_assemble_strips: a multi-device frame's strips into one image
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_device.h"
#include "aic_launch.h"

namespace aic {

// the tag of a cube holding block `b`, short of OPEN (aic_device.h): the block's class plus one
__device__ __forceinline__ uint32_t cube_tag_of(const uint32_t *cls, uint32_t b) { return ((cls[b >> 4] >> ((b & 15u) << 1)) & 3u) + 1u; }

// aic_update_cubes: scatter of SpaceChange::{CubeBlock,CubeLight} (updating.rs:146-166)
__global__ void scatter_cubes_kernel(uint16_t *grid, uint32_t *light, const int32_t *xyz, const uint16_t *bi,
                                     const uint32_t *lt, uint32_t n, int lx, int ly, int lz, int sx, int sy, int sz,
                                     const uint32_t *cls) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t dx = (uint32_t)xyz[3 * i + 0] - (uint32_t)lx;
    uint32_t dy = (uint32_t)xyz[3 * i + 1] - (uint32_t)ly;
    uint32_t dz = (uint32_t)xyz[3 * i + 2] - (uint32_t)lz;
    if ((dx >= (uint32_t)sx) | (dy >= (uint32_t)sy) | (dz >= (uint32_t)sz)) return;
    size_t idx = ((size_t)dx * sy + dy) * sz + dz;
    if (bi) {
        uint32_t b = bi[i];
        if (cls) b |= cube_tag_of(cls, b) << kCubeClassShift;  // cls != null: tagged grid (never OPEN: open_changed_cubes_kernel decides that, after every cube is in)
        grid[idx] = (uint16_t)b;
    }
    if (lt) light[idx] = lt[i];
}

// (re)writes the class bits of every cube-grid entry from the class table (aic_device.h); no entry comes out OPEN
__global__ void tag_cubes_kernel(uint16_t *grid, size_t n, const uint32_t *cls, int from_tagged, int to_tagged) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t b = grid[i];
    if (from_tagged) b &= kCubeIndexMask;
    if (to_tagged) b |= cube_tag_of(cls, b) << kCubeClassShift;
    grid[i] = (uint16_t)b;
}

// The OPEN tag (aic_device.h) of cube (x, y, z) of a tagged grid, decided from the grid as it stands: an invisible cube inside the outermost layer whose six
// face neighbours are invisible. Only the tag bit between OPEN and INVISIBLE is ever written, with a value that depends on nobody's tag bit but on classes
// alone (tag <= INVISIBLE), so threads that decide neighbouring cubes -- or the same cube twice -- at the same time write what a serial pass would.
__device__ __forceinline__ void decide_open(uint16_t *grid, int x, int y, int z, int sx, int sy, int sz) {
    const size_t i = ((size_t)x * sy + y) * sz + z;
    const uint32_t b = grid[i];
    if ((b >> kCubeClassShift) > kCubeTagInvisible) return;
    bool open = x > 0 && y > 0 && z > 0 && x < sx - 1 && y < sy - 1 && z < sz - 1;
    if (open) {
        const size_t stx = (size_t)sy * sz, sty = (size_t)sz;
        const uint32_t worst = max(max(max((uint32_t)grid[i - stx], (uint32_t)grid[i + stx]), max((uint32_t)grid[i - sty], (uint32_t)grid[i + sty])),
                                   max((uint32_t)grid[i - 1], (uint32_t)grid[i + 1]));
        open = (worst >> kCubeClassShift) <= kCubeTagInvisible;
    }
    const uint32_t nb = (b & kCubeIndexMask) | ((open ? kCubeTagOpen : kCubeTagInvisible) << kCubeClassShift);
    if (nb != b) grid[i] = (uint16_t)nb;
}

// every cube of a tagged grid (after tag_cubes_kernel: upload, a block that changed class)
__global__ void open_cubes_kernel(uint16_t *grid, int sx, int sy, int sz) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)sx * sy * sz) return;
    const int z = (int)(i % (size_t)sz), y = (int)((i / (size_t)sz) % (size_t)sy), x = (int)(i / ((size_t)sz * sy));
    decide_open(grid, x, y, z, sx, sy, sz);
}

// aic_update_cubes, after the scatter: the changed cubes and their six face neighbours (thread = change * 8 + which of the seven)
__global__ void open_changed_cubes_kernel(uint16_t *grid, const int32_t *xyz, uint32_t n, int lx, int ly, int lz, int sx, int sy, int sz) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 3, k = t & 7u;
    if (i >= n || k == 7u) return;
    // (in 64 bits: a change may name any i32 cube, inside the space or not)
    long long x = (long long)xyz[3 * i + 0] - lx, y = (long long)xyz[3 * i + 1] - ly, z = (long long)xyz[3 * i + 2] - lz;
    if (k == 1u) x--; else if (k == 2u) x++; else if (k == 3u) y--; else if (k == 4u) y++; else if (k == 5u) z--; else if (k == 6u) z++;
    if (x < 0 || y < 0 || z < 0 || x >= sx || y >= sy || z >= sz) return;
    decide_open(grid, (int)x, (int)y, (int)z, sx, sy, sz);
}

// Orders the tiles of the next frame by the cost the previous frame measured for them (its longest
// ray, in steps), costliest first: the rays most likely to be long start early instead of landing
// in the frame's tail, where a wave with two live lanes still pays a whole event phase for each.
// One workgroup: histogram over 1024 cost buckets per queue, prefix sum, scatter. Order inside a bucket is
// whatever the atomics give -- every pixel is traced exactly once either way.
//
// Queues (round 4): each XCD has its own L2, and with one dispenser for the chip the 4 waves' worth of rays of a macro tile and of
// its neighbours run on all eight at once -- every L2 fetches the same lines. With n_queues > 1 the macro tiles are dealt to queues
// by the super-block (2^sb_shift macro tiles on a side) they lie in, a workgroup serves the queue of the XCD it runs on (and helps
// the others when its own is empty), and `order` comes out as n_queues segments, each costliest first; queue_start[q] is where
// segment q begins. cost == nullptr: no record to go by (index order inside a queue, as far as the atomics keep it).
__device__ __forceinline__ uint32_t tile_queue_of(uint32_t mt, uint32_t macros_x, uint32_t sb_shift, uint32_t n_queues) {
    // mt / macros_x without the ~40-instruction integer division (this runs twice per macro tile on one workgroup, ahead of every frame):
    // a float quotient is within one of the truth for these sizes (mt < 2^24), corrected exactly
    uint32_t my = (uint32_t)((float)mt * __builtin_amdgcn_rcpf((float)macros_x));
    if (my * macros_x > mt) my--;
    else if ((my + 1u) * macros_x <= mt) my++;
    const uint32_t mx = mt - my * macros_x;
    const uint32_t v = (mx >> sb_shift) + 3u * (my >> sb_shift);
    return (n_queues & (n_queues - 1u)) == 0u ? (v & (n_queues - 1u)) : v % n_queues;
}
// One workgroup of kOrderThreads = 256 threads (four waves, 33 KB of LDS): what ONE retiring workgroup of a trace kernel leaves free on a CU. With 1024
// threads it needed a whole CU to drain, and while frames are streamed every CU is full of persistent trace workgroups: rocprofv3 showed it
// waiting 0.14 ms (C2) / 1.6 ms (C3) for a place to run (profiles/r04_experiments.txt L).
constexpr uint32_t kOrderThreads = 256;
// (a workgroup per job -- OrderJobs, aic_device.h: the frames of a batch, aic_render_submit_batch, are ordered by one launch)
__global__ __launch_bounds__(kOrderThreads) void order_tiles_kernel(const OrderJobs jobs, uint32_t n_tiles, uint32_t macros_x, uint32_t sb_shift, uint32_t n_queues,
                                                                    uint32_t clear_the_cost, uint32_t n_clear_words) {
    const uint32_t *__restrict__ const cost = jobs.cost[blockIdx.x];
    uint32_t *__restrict__ const order = jobs.order[blockIdx.x];
    uint32_t *__restrict__ const queue_start = jobs.queue_start[blockIdx.x];
    uint32_t *const clear_cost = (clear_the_cost && cost) ? const_cast<uint32_t *>(cost) : nullptr;
    uint32_t *const clear_words = jobs.clear_words[blockIdx.x];
    __shared__ uint32_t hist[kMaxTileQueues * 1024];
    __shared__ uint32_t scan[kOrderThreads];
    // (behind a frame this launch also does the slot's clearing -- the frame's counters, and below the cost record once it has been read -- instead of two
    //  fill launches that would each wait for room on a CU)
    if (clear_words) for (uint32_t i = threadIdx.x; i < n_clear_words; i += kOrderThreads) clear_words[i] = 0u;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_bins = n_queues * 1024u;
    const uint32_t per_thread = n_bins / kOrderThreads;  // 4 * n_queues consecutive buckets each
    const uint32_t *const cp = cost ? cost : order;  // no record: any readable words, masked away
    const uint32_t use = cost ? ~0u : 0u;
    for (uint32_t b = tid; b < n_bins; b += kOrderThreads) hist[b] = 0;
    __syncthreads();
    // (eight tiles per thread at a time: the eight cost fetches are issued together, not one ahead of each atomic)
    for (uint32_t base = tid; base < n_tiles; base += 8u * kOrderThreads) {
        uint32_t c[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) c[k] = cp[min(base + k * kOrderThreads, n_tiles - 1u)] & use;  // (unconditional: nothing keeps the eight fetches apart)
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            const uint32_t t = base + k * kOrderThreads;
            if (t < n_tiles) atomicAdd(&hist[tile_queue_of(t, macros_x, sb_shift, n_queues) * 1024u + 1023u - (c[k] < 1023u ? c[k] : 1023u)], 1u);
        }
    }
    __syncthreads();
    // exclusive prefix sum over the n_queues * 1024 buckets: thread `tid` owns `per_thread` consecutive buckets
    uint32_t mine = 0;
    for (uint32_t k = 0; k < per_thread; k++) mine += hist[tid * per_thread + k];
    scan[tid] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < kOrderThreads; off <<= 1) {  // Hillis-Steele over the partial sums
        const uint32_t v = tid >= off ? scan[tid - off] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    uint32_t run = scan[tid] - mine;
    for (uint32_t k = 0; k < per_thread; k++) {
        const uint32_t h = hist[tid * per_thread + k];
        hist[tid * per_thread + k] = run;  // start of each bucket
        run += h;
    }
    __syncthreads();
    if (queue_start && tid <= n_queues) queue_start[tid] = tid < n_queues ? hist[tid * 1024u] : n_tiles;
    __syncthreads();
    for (uint32_t base = tid; base < n_tiles; base += 8u * kOrderThreads) {
        uint32_t c[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) c[k] = cp[min(base + k * kOrderThreads, n_tiles - 1u)] & use;
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            const uint32_t t = base + k * kOrderThreads;
            if (t < n_tiles) {
                const uint32_t pos = atomicAdd(&hist[tile_queue_of(t, macros_x, sb_shift, n_queues) * 1024u + 1023u - (c[k] < 1023u ? c[k] : 1023u)], 1u);
                order[pos] = t;
                if (clear_cost) clear_cost[t] = 0u;
            }
        }
    }
}

// aic_assemble_strips: [n_parts][max_rows][w] compacted strips -> [h][w]
__global__ void assemble_strips_kernel(const uint32_t *gathered, uint32_t *out, uint32_t w, uint32_t h, uint32_t strip_rows,
                                       uint32_t n_parts, uint32_t max_rows) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)w * h) return;
    uint32_t y = (uint32_t)(i / w), x = (uint32_t)(i % w);
    uint32_t strip = y / strip_rows;
    uint32_t part = strip % n_parts;
    uint32_t lrow = (strip / n_parts) * strip_rows + (y % strip_rows);
    out[i] = gathered[((size_t)part * max_rows + lrow) * w + x];
}

void launch_tag_cubes(uint16_t *grid, size_t n, const uint32_t *cls, int from_tagged, int to_tagged, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(tag_cubes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, grid, n, cls, from_tagged, to_tagged);
}

// the OPEN tags of a whole tagged grid / of the cubes around `n` changes (device array of xyz triples): after the tags themselves, on the same stream
void launch_open_cubes(uint16_t *grid, const int size[3], hipStream_t stream) {
    const size_t n = (size_t)size[0] * (size_t)size[1] * (size_t)size[2];
    if (!n) return;
    hipLaunchKernelGGL(open_cubes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, grid, size[0], size[1], size[2]);
}
void launch_open_changed_cubes(uint16_t *grid, const int32_t *xyz, uint32_t n, const int lo[3], const int size[3], hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(open_changed_cubes_kernel, dim3((unsigned)(((size_t)n * 8 + 255) / 256)), dim3(256), 0, stream, grid, xyz, n, lo[0], lo[1], lo[2], size[0], size[1],
                       size[2]);
}

void launch_scatter_cubes(uint16_t *grid, uint32_t *light, const int32_t *xyz, const uint16_t *bi, const uint32_t *lt,
                          uint32_t n, const int lo[3], const int size[3], const uint32_t *cls, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(scatter_cubes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, grid, light, xyz, bi, lt, n, lo[0],
                       lo[1], lo[2], size[0], size[1], size[2], cls);
}

void launch_order_tiles_jobs(const OrderJobs &jobs, uint32_t n_jobs, uint32_t n_tiles, uint32_t macros_x, uint32_t sb_shift, uint32_t n_queues, hipStream_t stream,
                             bool clear_cost, uint32_t n_clear_words) {
    if (!n_tiles || !n_jobs) return;
    if (n_queues < 1u) n_queues = 1u;
    if (n_queues > kMaxTileQueues) n_queues = kMaxTileQueues;
    hipLaunchKernelGGL(order_tiles_kernel, dim3(n_jobs), dim3(kOrderThreads), 0, stream, jobs, n_tiles, macros_x ? macros_x : 1u, sb_shift, n_queues, clear_cost ? 1u : 0u,
                       n_clear_words);
}
void launch_order_tiles(const uint32_t *cost, uint32_t *order, uint32_t n_tiles, uint32_t macros_x, uint32_t sb_shift, uint32_t n_queues, uint32_t *queue_start,
                        hipStream_t stream, bool clear_cost, uint32_t *clear_words, uint32_t n_clear_words) {
    OrderJobs jobs{};
    jobs.cost[0] = cost; jobs.order[0] = order; jobs.queue_start[0] = queue_start; jobs.clear_words[0] = clear_words;
    launch_order_tiles_jobs(jobs, 1u, n_tiles, macros_x, sb_shift, n_queues, stream, clear_cost, n_clear_words);
}

void launch_assemble_strips(const uint32_t *gathered, uint32_t *out, uint32_t w, uint32_t h, uint32_t strip_rows,
                            uint32_t n_parts, uint32_t max_rows, hipStream_t stream) {
    size_t n = (size_t)w * h;
    if (!n) return;
    hipLaunchKernelGGL(assemble_strips_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, gathered, out, w, h,
                       strip_rows, n_parts, max_rows);
}

}  // namespace aic
