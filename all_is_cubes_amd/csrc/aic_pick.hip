// aic_pick.hip -- the device-side pixel picker on gfx950 (aic_pick.h; DESIGN.md "Picking pixels on the device", which tests/pick_ref.py follows).
//
// Rank r of the picker's order holds pixel order[r]; a rank is "unknown" when that pixel's texel of the last reprojection's splat image R fails the
// gap fill's validity test (alpha > -0.5). The unknown ranks are compacted in rank order -- a stable stream compaction, the same list on every run:
// nothing is ordered by an atomic --, and the rest of the list is PixelPicker's sequence from a cursor.
//
// The compaction's three phases (count, scan, write) and the picker's picks are aic_rank_list.h's, which the stale pickers use too. What is this
// file's own: the predicate, and a write whose first grid part re-derives each block's flags (the scratch holds no ballots) and so takes the wave
// offsets through LDS.
//
// The gathers R[order[r]] are scattered 4-byte reads (only the alpha half's word is read). The picker order is left as it is.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_pick.h"

namespace aic {

namespace {

static_assert(kPickBlock == kRankBlock, "aic_rank_list.h's scan block");

AIC_DEV uint32_t *pick_counts(const PickParams &p) { return p.scratch + sizeof(PickRecord) / 4u; }
AIC_DEV uint32_t *pick_offsets(const PickParams &p, uint32_t nb) { return pick_counts(p) + nb; }

// !(alpha > -0.5) of the pixel's texel in R: no sprite, a winner that carried the marker, a NaN alpha. An entry that is no pixel is never unknown.
AIC_DEV bool pixel_unknown(const PickParams &p, uint32_t px) {
    if (px >= p.count) return false;
    const uint32_t hi = reinterpret_cast<const uint32_t *>(p.R)[(size_t)px * 2u + 1u];  // blue | alpha << 16
    const float alpha = (float)__builtin_bit_cast(_Float16, (uint16_t)(hi >> 16));
    return !(alpha > -0.5f);
}

__global__ void __launch_bounds__(256) pick_count_kernel(PickParams p) {
    const uint32_t r = blockIdx.x * kPickBlock + threadIdx.x;  // (count rounded up to whole blocks is still below 2^32)
    const bool unknown = r < p.count && pixel_unknown(p, rank_pixel(p.order, r));
    block_count(__ballot(unknown), pick_counts(p));
}

__global__ void __launch_bounds__(1024) pick_scan_kernel(PickParams p, uint32_t nb) {
    const uint32_t n_unknown = scan_block_counts(pick_counts(p), pick_offsets(p, nb), nb);
    if (threadIdx.x == 0u) {
        PickRecord rec;
        rec.head = rank_list_record(n_unknown, p.n, p.max_unknown, p.skip_unknown, p.cursor);
        rec.pad[0] = rec.pad[1] = 0u;
        *reinterpret_cast<PickRecord *>(p.scratch) = rec;
    }
}

// blocks [0, nbc): the unknown ranks (nbc = 0 with max_unknown == 0: the record is then not read, g = 0); blocks from nbc on: the picker picks
__global__ void __launch_bounds__(256) pick_write_kernel(PickParams p, uint32_t nbc) {
    __shared__ uint32_t wave_n[4];
    const uint32_t g = nbc ? reinterpret_cast<const PickRecord *>(p.scratch)->head.n_from_set : 0u;  // <= n
    if (blockIdx.x < nbc) {
        RankWindow win;
        if (!win.open(pick_counts(p), pick_offsets(p, nbc), p.skip_unknown, g)) return;
        const uint32_t r = blockIdx.x * kPickBlock + threadIdx.x;
        const uint32_t px = r < p.count ? rank_pixel(p.order, r) : 0xFFFFFFFFu;
        const bool unknown = r < p.count && pixel_unknown(p, px);
        const unsigned long long b = __ballot(unknown);
        const uint32_t wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0u) wave_n[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t wave_off = 0u;
        for (uint32_t w = 0u; w < 3u; w++)
            if (w < wave) wave_off += wave_n[w];
        if (unknown) win.store(p.out, wave_off, b, px);
        return;
    }
    write_picks(p.order, p.out, p.count, p.n, g, p.cursor, (blockIdx.x - nbc) * kPickBlock + threadIdx.x);
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
