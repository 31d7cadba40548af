// aic_stale_blocks.hip -- the finder of the cubes that hold given block indices, on gfx950 (aic_stale_blocks.h; DESIGN.md 4.20, which
// tests/stale_blocks_ref.py follows).
//
// A streaming scan of the layer's Z-major u16 cube grid. A workgroup of 256 lanes owns 2048 consecutive entries and stages the set of block indices --
// a bitset of at most 8 KB -- in LDS; a lane loads its 8 entries with one 16-byte access (the grid's last partial group with 2-byte loads: nothing past
// the grid's n entries is read, where the pool goes on with voxel volumes) and forms an 8-bit match mask. A run of matches along z starts where the
// entry before does not match or lies in another row, and ends likewise; the neighbour's bit comes from the adjacent lane's mask through LDS and, across
// workgroups, from one entry read again. The k-th start and the k-th end in linear order belong to the same run, so two stable compactions -- of the
// starts and of the ends -- give the run list with no walk along a run: the start's lane writes box[k][0..4], the end's lane box[k][5].
//
//  * Count: per workgroup the starts, ends and matches, summed in the wave and through LDS and stored; at most one atomic min / max per workgroup and
//    bound (integer atomics are order-free), none where the bound read first is as good already. One workgroup then sums the stored counts into the record.
//  * Scan: one workgroup over the workgroups' counts, as the pickers' compactions do it.
//  * Write: the same lane arithmetic again, a scan of the lanes' counts in the workgroup, and the stores.
// The host reads the record between count and scan: with more runs than the caller's capacity nothing more is queued.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_stale_blocks.h"

#ifndef AIC_DEV
#define AIC_DEV __device__ __forceinline__
#endif

namespace aic {

namespace {

AIC_DEV BlockCubesRecord *blocks_record(const BlockCubesParams &p) { return reinterpret_cast<BlockCubesRecord *>(p.scratch); }
AIC_DEV const uint32_t *blocks_set(const BlockCubesParams &p) { return reinterpret_cast<const uint32_t *>(p.scratch + sizeof(BlockCubesRecord)); }
// the offsets are aic_stale_blocks.h's
AIC_DEV uint32_t *blocks_counts(const BlockCubesParams &p) {
    return reinterpret_cast<uint32_t *>(p.scratch + ((sizeof(BlockCubesRecord) + 4u * (size_t)p.set_words + 15u) & ~(size_t)15u));
}
AIC_DEV uint2 *blocks_offsets(const BlockCubesParams &p, unsigned long long groups) {
    const size_t counts = (sizeof(BlockCubesRecord) + 4u * (size_t)p.set_words + 15u) & ~(size_t)15u;
    return reinterpret_cast<uint2 *>(p.scratch + ((counts + 4u * (size_t)groups + 15u) & ~(size_t)15u));
}

// whether a grid entry's block index is in the staged set; an index past the set's words is not (0xFFFFFFFF stands for "no entry")
AIC_DEV uint32_t entry_matches(const uint32_t *set, uint32_t set_words, uint32_t index) {
    const uint32_t w = index >> 5;
    return w < set_words ? (set[w] >> (index & 31u)) & 1u : 0u;
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

// What a lane knows of its 8 entries. x, y, z: the grid coordinates of its first entry; only made when m is not 0.
struct LaneRuns {
    uint32_t m;             // bit j: entry i0 + j matches
    uint32_t starts, ends;  // ... starts a run, ends a run
    uint32_t x, y, z;
};

// The lane's part of the scan, the same in both passes. `set` (kBlockSetWords words) and `masks` (256 words) are LDS; all lanes of the workgroup call it.
AIC_DEV LaneRuns lane_runs(const BlockCubesParams &p, uint32_t *set, uint32_t *masks) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t w = tid; w < p.set_words; w += kBlockCubesLanes) set[w] = blocks_set(p)[w];
    __syncthreads();
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kBlockCubesGroup + tid * kBlockCubesPerLane;
    LaneRuns r = {};
    if (i0 + kBlockCubesPerLane <= p.n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p.grid + i0);  // i0 is a multiple of 8 and the grid starts an allocation: 16-byte aligned
        const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0u; k < 4u; k++) {
            r.m |= entry_matches(set, p.set_words, (e[k] & 0xffffu) & p.index_mask) << (2u * k);
            r.m |= entry_matches(set, p.set_words, (e[k] >> 16) & p.index_mask) << (2u * k + 1u);
        }
    } else {
        for (uint32_t j = 0u; j < kBlockCubesPerLane; j++)
            if (i0 + j < p.n) r.m |= entry_matches(set, p.set_words, (uint32_t)p.grid[i0 + j] & p.index_mask) << j;
    }
    masks[tid] = r.m;
    __syncthreads();
    if (!r.m) return r;
    // the entries before and after the lane's: the adjacent lane's mask, or across workgroups the entry itself (inside the grid, or no match)
    uint32_t prev, next;
    if (tid > 0u) prev = masks[tid - 1u] >> 7;
    else prev = i0 > 0ull ? entry_matches(set, p.set_words, (uint32_t)p.grid[i0 - 1ull] & p.index_mask) : 0u;
    if (tid + 1u < kBlockCubesLanes) next = masks[tid + 1u] & 1u;
    else next = i0 + kBlockCubesPerLane < p.n ? entry_matches(set, p.set_words, (uint32_t)p.grid[i0 + kBlockCubesPerLane] & p.index_mask) : 0u;
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
AIC_DEV void next_cube(const BlockCubesParams &p, uint32_t &x, uint32_t &y, uint32_t &z) {
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

__global__ void __launch_bounds__(256) block_cubes_count_kernel(BlockCubesParams p) {
    __shared__ uint32_t set[kBlockSetWords];
    __shared__ uint32_t masks[kBlockCubesLanes];
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t lo[3], hi[3];
    if (threadIdx.x < 3u) { lo[threadIdx.x] = 0xFFFFFFFFu; hi[threadIdx.x] = 0u; }  // (lane_runs' barriers stand between this and the atomics)
    const LaneRuns r = lane_runs(p, set, masks);
    // starts | ends << 10 | matches << 20: a wave's sums are at most 512 each
    uint32_t s = (uint32_t)__popc(r.starts) | ((uint32_t)__popc(r.ends) << 10) | ((uint32_t)__popc(r.m) << 20);
    for (uint32_t d = 32u; d; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = s;
    if (s >> 20) {  // the wave holds a match: every match lies in a run, whose start and end give the bounds
        uint32_t bx0 = 0xFFFFFFFFu, by0 = 0xFFFFFFFFu, bz0 = 0xFFFFFFFFu, bx1 = 0u, by1 = 0u, bz1 = 0u;
        if (r.m) {
            uint32_t x = r.x, y = r.y, z = r.z;
            for (uint32_t j = 0u; j < kBlockCubesPerLane; j++) {
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
    const uint32_t n_match = (a >> 20) + (b >> 20) + (c >> 20) + (d >> 20);
    if (threadIdx.x == 0u) {
        blocks_counts(p)[blockIdx.x] = n_starts | (n_ends << 16);  // at most 2048 each
        blocks_offsets(p, gridDim.x)[blockIdx.x].x = n_match;       // (the offsets' place until the scan: block_cubes_total_kernel sums it)
    }
    if (n_match && threadIdx.x < 3u) {  // (a match in the workgroup; one that lies wholly inside a run has neither a start nor an end and leaves lo and hi at their initial values, which move nothing)
        // Thousands of workgroups meet at these six words, and atomics on one address run one behind the other; a bound only ever moves one way, so a
        // value read first that is as good already -- stale or not -- says the atomic would change nothing.
        BlockCubesRecord *rec = blocks_record(p);
        if (lo[threadIdx.x] < __hip_atomic_load(&rec->lo[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&rec->lo[threadIdx.x], lo[threadIdx.x]);
        if (hi[threadIdx.x] > __hip_atomic_load(&rec->hi[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&rec->hi[threadIdx.x], hi[threadIdx.x]);
    }
}

// one workgroup: the record's two counts, summed from what the count's workgroups stored (no atomic: thousands of adds to one address took ten times the scan)
__global__ void __launch_bounds__(1024) block_cubes_total_kernel(BlockCubesParams p, uint32_t groups) {
    __shared__ unsigned long long wave_runs[16], wave_cubes[16];
    const uint32_t *counts = blocks_counts(p);
    const uint2 *matches = blocks_offsets(p, groups);
    unsigned long long runs = 0ull, cubes = 0ull;
    for (uint32_t i = threadIdx.x; i < groups; i += 1024u) {
        runs += counts[i] & 0xffffu;
        cubes += matches[i].x;
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
        blocks_record(p)->n_runs = runs;
        blocks_record(p)->n_cubes = cubes;
    }
}

// one workgroup: offsets[g] = the starts and the ends of the workgroups before g. Only run when the runs are written: their number fits 32 bits.
__global__ void __launch_bounds__(1024) block_cubes_scan_kernel(BlockCubesParams p, uint32_t groups) {
    __shared__ unsigned long long wave_sum[16];
    const uint32_t *counts = blocks_counts(p);
    uint2 *offsets = blocks_offsets(p, groups);
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

__global__ void __launch_bounds__(256) block_cubes_write_kernel(BlockCubesParams p, uint32_t groups) {
    __shared__ uint32_t set[kBlockSetWords];
    __shared__ uint32_t masks[kBlockCubesLanes];
    __shared__ uint32_t wave_sum[4];
    if (blocks_counts(p)[blockIdx.x] == 0u) return;  // no start and no end: the whole workgroup alike
    const LaneRuns r = lane_runs(p, set, masks);
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
    const uint2 base = blocks_offsets(p, groups)[blockIdx.x];
    uint32_t ks = base.x + (before & 0xffffu), ke = base.y + (before >> 16);
    uint32_t x = r.x, y = r.y, z = r.z;
    for (uint32_t j = 0u; j < kBlockCubesPerLane; j++) {
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

}  // namespace

hipError_t launch_count_block_cubes(const BlockCubesParams &p, hipStream_t stream) {
    if (!p.n) return hipSuccess;
    const uint32_t groups = (uint32_t)block_cubes_groups(p.n);
    block_cubes_count_kernel<<<groups, kBlockCubesLanes, 0, stream>>>(p);
    block_cubes_total_kernel<<<1, 1024, 0, stream>>>(p, groups);
    return hipGetLastError();
}

hipError_t launch_write_block_cubes(const BlockCubesParams &p, hipStream_t stream) {
    if (!p.n || !p.n_runs) return hipSuccess;
    const uint32_t groups = (uint32_t)block_cubes_groups(p.n);
    block_cubes_scan_kernel<<<1, 1024, 0, stream>>>(p, groups);
    block_cubes_write_kernel<<<groups, kBlockCubesLanes, 0, stream>>>(p, groups);
    return hipGetLastError();
}

}  // namespace aic
