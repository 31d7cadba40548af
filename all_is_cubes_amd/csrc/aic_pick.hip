// aic_pick.hip -- the device-side pixel picker on gfx950 (aic_pick.h; DESIGN.md "Picking pixels on the device", which tests/pick_ref.py follows).
//
// Rank r of the picker's order holds pixel order[r]; a rank is "unknown" when that pixel's texel of the last reprojection's splat image R fails the
// gap fill's validity test (alpha > -0.5). The unknown ranks are compacted in rank order -- a stable stream compaction, the same list on every run:
// nothing is ordered by an atomic --, and the rest of the list is PixelPicker's sequence from a cursor.
//
//  * Count: a scan block is 256 consecutive ranks, a lane each. A wave64 counts its unknown ranks with one ballot and popcount, the four waves add
//    through LDS, and the block leaves one number.
//  * Scan: one workgroup of 1024 walks the block counts 1024 at a time (wave scan by shuffles, the sixteen wave sums through LDS, a running carry) and
//    leaves for every block the unknown ranks before it; lane 0 then forms the record the host reads back: n_unknown, g, the next cursor.
//  * Write: the first grid part re-derives each block's flags; a lane's position in the rank list is block offset + wave offset + mbcnt, and it
//    stores its pixel when skip <= position < skip + g. A block whose range misses that window leaves at once. The second part writes the picker
//    picks behind the g entries; g comes from the record, so the host never waits between the launches.
//
// The gathers R[order[r]] are scattered 4-byte reads (only the alpha half's word is read). The picker order is left as it is.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_pick.h"

#ifndef AIC_DEV
#define AIC_DEV __device__ __forceinline__
#endif

namespace aic {

namespace {

AIC_DEV uint32_t *pick_counts(const PickParams &p) { return p.scratch + sizeof(PickRecord) / 4u; }
AIC_DEV uint32_t *pick_offsets(const PickParams &p, uint32_t nb) { return pick_counts(p) + nb; }

// the pixel of rank r < count
AIC_DEV uint32_t rank_pixel(const PickParams &p, uint32_t r) { return p.order ? p.order[r] : r; }

// !(alpha > -0.5) of the pixel's texel in R: no sprite, a winner that carried the marker, a NaN alpha. An entry that is no pixel is never unknown.
AIC_DEV bool pixel_unknown(const PickParams &p, uint32_t px) {
    if (px >= p.count) return false;
    const uint32_t hi = reinterpret_cast<const uint32_t *>(p.R)[(size_t)px * 2u + 1u];  // blue | alpha << 16
    const float alpha = (float)__builtin_bit_cast(_Float16, (uint16_t)(hi >> 16));
    return !(alpha > -0.5f);
}

// lanes of the wave below this one whose bit is set in `b`
AIC_DEV uint32_t lanes_before(unsigned long long b) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)); }

__global__ void __launch_bounds__(256) pick_count_kernel(PickParams p) {
    __shared__ uint32_t wave_n[4];
    const uint32_t r = blockIdx.x * kPickBlock + threadIdx.x;  // (count rounded up to whole blocks is still below 2^32)
    const bool unknown = r < p.count && pixel_unknown(p, rank_pixel(p, r));
    const unsigned long long b = __ballot(unknown);
    if ((threadIdx.x & 63u) == 0u) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0u) pick_counts(p)[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

__global__ void __launch_bounds__(1024) pick_scan_kernel(PickParams p, uint32_t nb) {
    __shared__ uint32_t wave_sum[16];
    const uint32_t *counts = pick_counts(p);
    uint32_t *offsets = pick_offsets(p, nb);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;  // unknown ranks before this round's blocks; at most count
    for (uint32_t base = 0u; base < nb; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? counts[i] : 0u;
        uint32_t s = v;  // inclusive over the wave
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (lane == 63u) wave_sum[wave] = s;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0u; w < 16u; w++) {
            const uint32_t x = wave_sum[w];
            if (w < wave) before += x;
            total += x;
        }
        if (i < nb) offsets[i] = carry + before + (s - v);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0u) {
        const unsigned long long n_unknown = carry;
        const unsigned long long left = n_unknown > p.skip_unknown ? n_unknown - p.skip_unknown : 0ull;
        unsigned long long g = p.n < p.max_unknown ? p.n : p.max_unknown;
        if (left < g) g = left;
        PickRecord rec;
        rec.n_unknown = n_unknown;
        rec.next_cursor = p.cursor + (unsigned long long)(p.n - (uint32_t)g);
        rec.n_from_unknown = (uint32_t)g;
        rec.n_from_order = p.n - (uint32_t)g;
        rec.pad[0] = rec.pad[1] = 0u;
        *reinterpret_cast<PickRecord *>(p.scratch) = rec;
    }
}

// pick k of PixelPicker's sequence as a rank (include/aic_hip.h under aic_pixel_order); all 64-bit
AIC_DEV uint32_t pick_rank(unsigned long long k, uint32_t count) {
    const uint32_t quarter = count / 4u, central = quarter < 60000u ? quarter : 60000u;
    if (central == 0u) return (uint32_t)(k % count);
    const unsigned long long h = k >> 1;
    return (k & 1ull) ? central + (uint32_t)(h % (count - central)) : (uint32_t)(h % central);
}

// blocks [0, nbc): the unknown ranks (nbc = 0 with max_unknown == 0: the record is then not read, g = 0); blocks from nbc on: the picker picks
__global__ void __launch_bounds__(256) pick_write_kernel(PickParams p, uint32_t nbc) {
    __shared__ uint32_t wave_n[4];
    const uint32_t g = nbc ? reinterpret_cast<const PickRecord *>(p.scratch)->n_from_unknown : 0u;  // <= n
    if (blockIdx.x < nbc) {
        if (g == 0u) return;
        const unsigned long long lo = p.skip_unknown, hi = lo + g;  // g > 0: skip < n_unknown < 2^32
        const unsigned long long b0 = pick_offsets(p, nbc)[blockIdx.x], bn = pick_counts(p)[blockIdx.x];
        if (b0 >= hi || b0 + bn <= lo) return;  // the whole workgroup alike
        const uint32_t r = blockIdx.x * kPickBlock + threadIdx.x;
        const uint32_t px = r < p.count ? rank_pixel(p, r) : 0xFFFFFFFFu;
        const bool unknown = r < p.count && pixel_unknown(p, px);
        const unsigned long long b = __ballot(unknown);
        const uint32_t wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0u) wave_n[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t wave_off = 0u;
        for (uint32_t w = 0u; w < 3u; w++)
            if (w < wave) wave_off += wave_n[w];
        const unsigned long long pos = b0 + wave_off + lanes_before(b);
        if (unknown && pos >= lo && pos < hi) p.out[pos - lo] = px;  // pos - lo < g <= n
        return;
    }
    const uint32_t j = (blockIdx.x - nbc) * kPickBlock + threadIdx.x;  // (n is at most 2048 x 65535)
    if (j >= p.n - g) return;
    const uint32_t r = pick_rank(p.cursor + j, p.count);  // < count
    p.out[g + j] = rank_pixel(p, r);                      // g + j < n
}

}  // namespace

hipError_t launch_pick(const PickParams &p, hipStream_t stream) {
    if (!p.count || !p.n) return hipSuccess;
    const uint32_t nb = pick_blocks(p.count), nbc = p.max_unknown ? nb : 0u;
    if (nbc) {
        pick_count_kernel<<<nb, kPickBlock, 0, stream>>>(p);
        pick_scan_kernel<<<1, 1024, 0, stream>>>(p, nb);
    }
    pick_write_kernel<<<nbc + (p.n + kPickBlock - 1u) / kPickBlock, kPickBlock, 0, stream>>>(p, nbc);
    return hipGetLastError();
}

}  // namespace aic
