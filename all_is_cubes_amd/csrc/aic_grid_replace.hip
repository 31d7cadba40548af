// aic_grid_replace.hip -- the replacement of a layer's whole cube grid from device memory, on gfx950 (aic_grid_replace.h; DESIGN.md 4.23, which
// tests/grid_replace_ref.py follows).
//
// The streaming scan of aic_stale_blocks.hip with another match: a workgroup of 256 lanes owns 2048 consecutive entries; a lane loads its 8 entries of
// the grid and its 8 of the caller's array with one 16-byte access each (the last partial group with 2-byte accesses: nothing past the grid's n entries
// is read or written, where the pool goes on with voxel volumes) and forms an 8-bit mask of "the new index differs from the index held". A run of
// changes along z starts where the entry before has not changed or lies in another row, and ends likewise; the neighbour's bit comes from the adjacent
// lane's mask through LDS and, across workgroups, from one entry of each array read again. The k-th start and the k-th end in linear order belong to the
// same run, so two stable compactions -- of the starts and of the ends -- give the run list with no walk along a run.
//
//  * Count: per workgroup the starts, ends and changes, summed in the wave and through LDS and stored; the largest new index, reduced in the wave and
//    the workgroup, one atomic max per workgroup; at most one atomic min / max per workgroup and bound. One workgroup then sums the stored counts into
//    the record. Nothing but scratch is written: the host reads the record and refuses an index out of range with the grid untouched.
//  * Scan and write of the boxes: as the finder's. They compare the grid as it was, so they run before the store.
//  * Store: new | tag in the workgroups that hold a change, the tag from the class table staged in LDS. OPEN is decided afterwards, by the pass that
//    decides it after an upload (launch_open_cubes).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_device.h"
#include "aic_grid_replace.h"

#ifndef AIC_DEV
#define AIC_DEV __device__ __forceinline__
#endif

namespace aic {

namespace {

static_assert(kGridReplaceClsWords * 16u == kCubeIndexMask + 1u, "a grid that carries tags has at most 16384 blocks: its class table always fits the LDS copy");

AIC_DEV GridReplaceRecord *replace_record(const GridReplaceParams &p) { return reinterpret_cast<GridReplaceRecord *>(p.scratch); }
// the offsets are aic_grid_replace.h's
AIC_DEV uint32_t *replace_counts(const GridReplaceParams &p) { return reinterpret_cast<uint32_t *>(p.scratch + sizeof(GridReplaceRecord)); }
AIC_DEV uint2 *replace_offsets(const GridReplaceParams &p, unsigned long long groups) {
    return reinterpret_cast<uint2 *>(p.scratch + ((sizeof(GridReplaceRecord) + 4u * (size_t)groups + 15u) & ~(size_t)15u));
}
AIC_DEV uint32_t *replace_changed(const GridReplaceParams &p, unsigned long long groups) {
    return reinterpret_cast<uint32_t *>(p.scratch + ((sizeof(GridReplaceRecord) + 4u * (size_t)groups + 15u) & ~(size_t)15u) + 8u * (size_t)groups);
}

// bit j (0..8) set: entry i0 + j is the first of its row, for a lane whose first entry has z = z0
AIC_DEV uint32_t row_starts9(uint32_t z0, uint32_t sz) {
    if (sz >= 9u) {  // at most one row start among nine entries
        const uint32_t j0 = z0 ? sz - z0 : 0u;
        return j0 < 9u ? 1u << j0 : 0u;
    }
    uint32_t bits = 0u, z = z0;
    for (uint32_t j = 0u; j < 9u; j++) {
        bits |= (z == 0u ? 1u : 0u) << j;
        z = z + 1u == sz ? 0u : z + 1u;
    }
    return bits;
}

// whether entry i (inside the grid) changes
AIC_DEV uint32_t entry_changes(const GridReplaceParams &p, unsigned long long i) { return (((uint32_t)p.grid[i] & p.index_mask) != (uint32_t)p.fresh[i]) ? 1u : 0u; }

// What a lane knows of its 8 entries. x, y, z: the grid coordinates of its first entry; only made when m is not 0.
struct LaneRuns {
    uint32_t m;             // bit j: entry i0 + j changes
    uint32_t starts, ends;  // ... starts a run, ends a run
    uint32_t x, y, z;
    uint32_t top;           // the largest of the lane's new indices
};

// The lane's part of the scan, the same in both passes. `masks` (256 words) is LDS; all lanes of the workgroup call it.
AIC_DEV LaneRuns lane_runs(const GridReplaceParams &p, uint32_t *masks) {
    const uint32_t tid = threadIdx.x;
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kGridReplaceGroup + tid * kGridReplacePerLane;
    LaneRuns r = {};
    if (i0 + kGridReplacePerLane <= p.n) {
        // i0 is a multiple of 8; the grid starts an allocation and the caller's array is checked: 16-byte aligned
        const uint4 o = *reinterpret_cast<const uint4 *>(p.grid + i0);
        const uint4 f = *reinterpret_cast<const uint4 *>(p.fresh + i0);
        const uint32_t eo[4] = {o.x, o.y, o.z, o.w}, ef[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t f0 = ef[k] & 0xffffu, f1 = ef[k] >> 16;
            r.m |= (((eo[k] & 0xffffu) & p.index_mask) != f0 ? 1u : 0u) << (2u * k);
            r.m |= (((eo[k] >> 16) & p.index_mask) != f1 ? 1u : 0u) << (2u * k + 1u);
            r.top = max(r.top, max(f0, f1));
        }
    } else {
        for (uint32_t j = 0u; j < kGridReplacePerLane; j++)
            if (i0 + j < p.n) {
                r.m |= entry_changes(p, i0 + j) << j;
                r.top = max(r.top, (uint32_t)p.fresh[i0 + j]);
            }
    }
    masks[tid] = r.m;
    __syncthreads();
    if (!r.m) return r;
    // the entries before and after the lane's: the adjacent lane's mask, or across workgroups the entries themselves (inside the grid, or no change)
    uint32_t prev, next;
    if (tid > 0u) prev = masks[tid - 1u] >> 7;
    else prev = i0 > 0ull ? entry_changes(p, i0 - 1ull) : 0u;
    if (tid + 1u < kGridReplaceLanes) next = masks[tid + 1u] & 1u;
    else next = i0 + kGridReplacePerLane < p.n ? entry_changes(p, i0 + kGridReplacePerLane) : 0u;
    // one division for z, one for x and y; 32-bit where the grid allows it
    if ((p.n >> 32) == 0ull) {
        const uint32_t row = (uint32_t)i0 / p.sz;
        r.z = (uint32_t)i0 - row * p.sz;
        r.x = row / p.sy;
        r.y = row - r.x * p.sy;
    } else {
        const unsigned long long row = i0 / p.sz;
        r.z = (uint32_t)(i0 - row * p.sz);
        r.x = (uint32_t)(row / p.sy);  // row < sx * sy
        r.y = (uint32_t)(row - (unsigned long long)r.x * p.sy);
    }
    const uint32_t zs9 = row_starts9(r.z, p.sz);
    r.starts = r.m & ((zs9 & 0xffu) | ~((r.m << 1) | prev));
    r.ends = r.m & ((zs9 >> 1) | ~((r.m >> 1) | (next << 7)));
    return r;
}

// one step along the grid's linear order
AIC_DEV void next_cube(const GridReplaceParams &p, uint32_t &x, uint32_t &y, uint32_t &z) {
    if (++z == p.sz) {
        z = 0u;
        if (++y == p.sy) { y = 0u; x++; }
    }
}

AIC_DEV uint32_t wave_min(uint32_t v) {
    for (uint32_t d = 32u; d; d >>= 1) { const uint32_t t = __shfl_xor(v, d); v = t < v ? t : v; }
    return v;
}
AIC_DEV uint32_t wave_max(uint32_t v) {
    for (uint32_t d = 32u; d; d >>= 1) { const uint32_t t = __shfl_xor(v, d); v = t > v ? t : v; }
    return v;
}

__global__ void __launch_bounds__(256) grid_replace_count_kernel(GridReplaceParams p) {
    __shared__ uint32_t masks[kGridReplaceLanes];
    __shared__ uint32_t wave_sum[4], wave_top[4];
    __shared__ uint32_t lo[3], hi[3];
    if (threadIdx.x < 3u) { lo[threadIdx.x] = 0xFFFFFFFFu; hi[threadIdx.x] = 0u; }  // (lane_runs' barrier stands between this and the atomics)
    const LaneRuns r = lane_runs(p, masks);
    // starts | ends << 10 | changes << 20: a wave's sums are at most 512 each
    uint32_t s = (uint32_t)__popc(r.starts) | ((uint32_t)__popc(r.ends) << 10) | ((uint32_t)__popc(r.m) << 20);
    for (uint32_t d = 32u; d; d >>= 1) s += __shfl_xor(s, d);
    const uint32_t top = wave_max(r.top);
    if ((threadIdx.x & 63u) == 0u) { wave_sum[threadIdx.x >> 6] = s; wave_top[threadIdx.x >> 6] = top; }
    if (s >> 20) {  // the wave holds a change: every change lies in a run, whose start and end give the bounds
        uint32_t bx0 = 0xFFFFFFFFu, by0 = 0xFFFFFFFFu, bz0 = 0xFFFFFFFFu, bx1 = 0u, by1 = 0u, bz1 = 0u;
        if (r.m) {
            uint32_t x = r.x, y = r.y, z = r.z;
            for (uint32_t j = 0u; j < kGridReplacePerLane; j++) {
                if ((r.starts >> j) & 1u) {
                    bx0 = x < bx0 ? x : bx0; by0 = y < by0 ? y : by0; bz0 = z < bz0 ? z : bz0;
                    bx1 = x + 1u > bx1 ? x + 1u : bx1; by1 = y + 1u > by1 ? y + 1u : by1;
                }
                if ((r.ends >> j) & 1u) bz1 = z + 1u > bz1 ? z + 1u : bz1;
                next_cube(p, x, y, z);
            }
        }
        bx0 = wave_min(bx0); by0 = wave_min(by0); bz0 = wave_min(bz0);
        bx1 = wave_max(bx1); by1 = wave_max(by1); bz1 = wave_max(bz1);
        if ((threadIdx.x & 63u) == 0u) {
            atomicMin(&lo[0], bx0); atomicMin(&lo[1], by0); atomicMin(&lo[2], bz0);
            atomicMax(&hi[0], bx1); atomicMax(&hi[1], by1); atomicMax(&hi[2], bz1);
        }
    }
    __syncthreads();
    const uint32_t a = wave_sum[0], b = wave_sum[1], c = wave_sum[2], d = wave_sum[3];
    const uint32_t n_starts = (a & 1023u) + (b & 1023u) + (c & 1023u) + (d & 1023u);
    const uint32_t n_ends = ((a >> 10) & 1023u) + ((b >> 10) & 1023u) + ((c >> 10) & 1023u) + ((d >> 10) & 1023u);
    const uint32_t n_changed = (a >> 20) + (b >> 20) + (c >> 20) + (d >> 20);
    GridReplaceRecord *rec = replace_record(p);
    if (threadIdx.x == 0u) {
        replace_counts(p)[blockIdx.x] = n_starts | (n_ends << 16);  // at most 2048 each
        replace_changed(p, gridDim.x)[blockIdx.x] = n_changed;
        // A value read first that is as good already -- stale or not -- says the atomic would change nothing: a maximum only ever grows.
        const uint32_t group_top = max(max(wave_top[0], wave_top[1]), max(wave_top[2], wave_top[3]));
        if (group_top > __hip_atomic_load(&rec->max_index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&rec->max_index, group_top);
    }
    if (n_changed && threadIdx.x < 3u) {  // (a change in the workgroup; one that lies wholly inside a run has neither a start nor an end and leaves lo and hi at their initial values, which move nothing)
        if (lo[threadIdx.x] < __hip_atomic_load(&rec->lo[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&rec->lo[threadIdx.x], lo[threadIdx.x]);
        if (hi[threadIdx.x] > __hip_atomic_load(&rec->hi[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&rec->hi[threadIdx.x], hi[threadIdx.x]);
    }
}

// one workgroup: the record's two counts, summed from what the count's workgroups stored (no atomic: the finder measured thousands of adds to one address at ten times the scan)
__global__ void __launch_bounds__(1024) grid_replace_total_kernel(GridReplaceParams p, uint32_t groups) {
    __shared__ unsigned long long wave_runs[16], wave_cubes[16];
    const uint32_t *counts = replace_counts(p);
    const uint32_t *changed = replace_changed(p, groups);
    unsigned long long runs = 0ull, cubes = 0ull;
    for (uint32_t i = threadIdx.x; i < groups; i += 1024u) {
        runs += counts[i] & 0xffffu;
        cubes += changed[i];
    }
    for (uint32_t d = 32u; d; d >>= 1) {
        runs += __shfl_xor(runs, d);
        cubes += __shfl_xor(cubes, d);
    }
    if ((threadIdx.x & 63u) == 0u) { wave_runs[threadIdx.x >> 6] = runs; wave_cubes[threadIdx.x >> 6] = cubes; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        runs = cubes = 0ull;
        for (uint32_t w = 0u; w < 16u; w++) { runs += wave_runs[w]; cubes += wave_cubes[w]; }
        replace_record(p)->n_runs = runs;
        replace_record(p)->n_cubes = cubes;
    }
}

// one workgroup: offsets[g] = the starts and the ends of the workgroups before g. Only run when the runs are written: their number fits 32 bits.
__global__ void __launch_bounds__(1024) grid_replace_scan_kernel(GridReplaceParams p, uint32_t groups) {
    __shared__ unsigned long long wave_sum[16];
    const uint32_t *counts = replace_counts(p);
    uint2 *offsets = replace_offsets(p, groups);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = 0ull;  // starts in the low half, ends in the high half
    for (uint32_t base = 0u; base < groups; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < groups ? counts[i] : 0u;
        const unsigned long long v = (unsigned long long)(c & 0xffffu) | ((unsigned long long)(c >> 16) << 32);
        unsigned long long s = v;  // inclusive over the wave
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const unsigned long long t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (lane == 63u) wave_sum[wave] = s;
        __syncthreads();
        unsigned long long before = 0ull, total = 0ull;
        for (uint32_t w = 0u; w < 16u; w++) {
            const unsigned long long x = wave_sum[w];
            if (w < wave) before += x;
            total += x;
        }
        const unsigned long long o = carry + before + (s - v);
        if (i < groups) offsets[i] = make_uint2((uint32_t)o, (uint32_t)(o >> 32));
        carry += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) grid_replace_write_kernel(GridReplaceParams p, uint32_t groups) {
    __shared__ uint32_t masks[kGridReplaceLanes];
    __shared__ uint32_t wave_sum[4];
    if (replace_counts(p)[blockIdx.x] == 0u) return;  // no start and no end: the whole workgroup alike
    const LaneRuns r = lane_runs(p, masks);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t v = (uint32_t)__popc(r.starts) | ((uint32_t)__popc(r.ends) << 16);  // a workgroup's sums are at most 2048 each
    uint32_t s = v;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(s, d);
        if (lane >= d) s += t;
    }
    if (lane == 63u) wave_sum[wave] = s;
    __syncthreads();
    if (!v) return;
    uint32_t before = s - v;
    for (uint32_t w = 0u; w < 3u; w++)
        if (w < wave) before += wave_sum[w];
    const uint2 base = replace_offsets(p, groups)[blockIdx.x];
    uint32_t ks = base.x + (before & 0xffffu), ke = base.y + (before >> 16);
    uint32_t x = r.x, y = r.y, z = r.z;
    for (uint32_t j = 0u; j < kGridReplacePerLane; j++) {
        if (((r.starts >> j) & 1u) && ks < p.n_runs) {
            int32_t *box = p.boxes + (size_t)ks * 6u;
            box[0] = p.lo[0] + (int32_t)x;
            box[1] = p.lo[1] + (int32_t)y;
            box[2] = p.lo[2] + (int32_t)z;
            box[3] = p.lo[0] + (int32_t)x + 1;
            box[4] = p.lo[1] + (int32_t)y + 1;
        }
        ks += (r.starts >> j) & 1u;
        if (((r.ends >> j) & 1u) && ke < p.n_runs) p.boxes[(size_t)ke * 6u + 5u] = p.lo[2] + (int32_t)z + 1;
        ke += (r.ends >> j) & 1u;
        next_cube(p, x, y, z);
    }
}

// a new index with its tag, short of OPEN (aic_device.h): the block's class plus one, from the staged class table; a plain index where the grid has none
AIC_DEV uint32_t tagged(const uint32_t *cls, uint32_t tags, uint32_t b) {
    return tags ? b | ((((cls[b >> 4] >> ((b & 15u) << 1)) & 3u) + 1u) << kCubeClassShift) : b;
}

__global__ void __launch_bounds__(256) grid_replace_store_kernel(GridReplaceParams p, uint32_t groups) {
    __shared__ uint32_t cls[kGridReplaceClsWords];
    if (replace_changed(p, groups)[blockIdx.x] == 0u) return;  // every index stays, and so does every tag: the whole workgroup alike
    const uint32_t tid = threadIdx.x, tags = p.cls ? 1u : 0u;
    if (tags) {  // (the host has checked every new index against the block count, so every lookup stays inside cls_words <= kGridReplaceClsWords)
        for (uint32_t w = tid; w < p.cls_words; w += kGridReplaceLanes) cls[w] = p.cls[w];
        __syncthreads();
    }
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kGridReplaceGroup + tid * kGridReplacePerLane;
    if (i0 + kGridReplacePerLane <= p.n) {
        const uint4 f = *reinterpret_cast<const uint4 *>(p.fresh + i0);
        uint32_t e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) e[k] = tagged(cls, tags, e[k] & 0xffffu) | (tagged(cls, tags, e[k] >> 16) << 16);
        *reinterpret_cast<uint4 *>(p.grid + i0) = make_uint4(e[0], e[1], e[2], e[3]);
    } else {
        for (uint32_t j = 0u; j < kGridReplacePerLane; j++)
            if (i0 + j < p.n) p.grid[i0 + j] = (uint16_t)tagged(cls, tags, (uint32_t)p.fresh[i0 + j]);
    }
}

__global__ void __launch_bounds__(256) copy_cube_grid_kernel(const uint16_t *grid, unsigned long long n, uint32_t index_mask, uint16_t *out) {
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * kGridReplaceLanes + threadIdx.x) * kGridReplacePerLane;
    const uint32_t both = index_mask | (index_mask << 16);
    if (i0 + kGridReplacePerLane <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(grid + i0);
        *reinterpret_cast<uint4 *>(out + i0) = make_uint4(v.x & both, v.y & both, v.z & both, v.w & both);
    } else {
        for (uint32_t j = 0u; j < kGridReplacePerLane; j++)
            if (i0 + j < n) out[i0 + j] = (uint16_t)((uint32_t)grid[i0 + j] & index_mask);
    }
}

}  // namespace

hipError_t launch_count_grid_replace(const GridReplaceParams &p, hipStream_t stream) {
    if (!p.n) return hipSuccess;
    const uint32_t groups = (uint32_t)grid_replace_groups(p.n);
    grid_replace_count_kernel<<<groups, kGridReplaceLanes, 0, stream>>>(p);
    grid_replace_total_kernel<<<1, 1024, 0, stream>>>(p, groups);
    return hipGetLastError();
}

hipError_t launch_write_grid_replace(const GridReplaceParams &p, hipStream_t stream) {
    if (!p.n || !p.n_runs) return hipSuccess;
    const uint32_t groups = (uint32_t)grid_replace_groups(p.n);
    grid_replace_scan_kernel<<<1, 1024, 0, stream>>>(p, groups);
    grid_replace_write_kernel<<<groups, kGridReplaceLanes, 0, stream>>>(p, groups);
    return hipGetLastError();
}

hipError_t launch_store_grid_replace(const GridReplaceParams &p, hipStream_t stream) {
    if (!p.n) return hipSuccess;
    const uint32_t groups = (uint32_t)grid_replace_groups(p.n);
    grid_replace_store_kernel<<<groups, kGridReplaceLanes, 0, stream>>>(p, groups);
    return hipGetLastError();
}

hipError_t launch_copy_cube_grid(const uint16_t *grid, unsigned long long n, uint32_t index_mask, uint16_t *out, hipStream_t stream) {
    if (!n) return hipSuccess;
    copy_cube_grid_kernel<<<(uint32_t)grid_replace_groups(n), kGridReplaceLanes, 0, stream>>>(grid, n, index_mask, out);
    return hipGetLastError();
}

}  // namespace aic
