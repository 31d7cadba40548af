// aic_stale.hip -- the picker of stale pixels on gfx950 (aic_stale.h; DESIGN.md 4.17, which tests/stale_ref.py follows).
//
// Rank r of the picker's order holds pixel order[r]; a rank is "stale" when that pixel lies inside a rectangle that does not keep it out. The stale ranks
// are compacted in rank order -- aic_pick.hip's stable stream compaction with another predicate, the same list on every run: nothing is ordered by an
// atomic --, and the rest of the list is PixelPicker's sequence from a cursor.
//
//  * Count: a scan block is 256 consecutive ranks, a lane each. The rectangles go through LDS 256 at a time (one 16-byte load a thread, then every lane
//    reads the same rectangle: a broadcast); a lane walks a chunk until a rectangle makes its pixel stale, and the block leaves the loop once every lane
//    has. With the depth test a lane loads its two texels once, at the first rectangle that contains it. A wave64's ballot of "stale" is its popcount and,
//    stored by one lane as a 64-bit word, its part of the rank-indexed bitmap; the four waves add through LDS and the block leaves one number
//    (aic_rank_list.h's block_count).
//  * Scan and write: aic_rank_list.h's, shared with the other pickers. The write's first grid part reads the bitmap instead of testing again.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_stale.h"

namespace aic {

namespace {

static_assert(kStaleBlock == kRankBlock, "aic_rank_list.h's scan block");

AIC_DEV uint32_t *stale_counts(const StaleParams &p) { return reinterpret_cast<uint32_t *>(p.scratch + sizeof(StaleRecord)); }
AIC_DEV uint32_t *stale_offsets(const StaleParams &p, uint32_t nb) { return stale_counts(p) + nb; }
// word [block * 4 + wave]; the offset is stale_bitmap_offset's
AIC_DEV unsigned long long *stale_bitmap(const StaleParams &p, uint32_t nb) {
    return reinterpret_cast<unsigned long long *>(p.scratch + ((sizeof(StaleRecord) + 8u * (size_t)nb + 7u) & ~(size_t)7u));
}

__global__ void __launch_bounds__(256) stale_count_kernel(StaleParams p, uint32_t nb) {
    __shared__ uint4 chunk[kStaleChunk];
    const uint32_t r = blockIdx.x * kStaleBlock + threadIdx.x;  // (count rounded up to whole blocks is still below 2^32)
    const uint32_t px = r < p.count ? rank_pixel(p.order, r) : 0xFFFFFFFFu;
    const bool is_pixel = px < p.count;  // an entry that is no pixel is never stale
    const uint32_t x = is_pixel ? px % p.width : 0u, y = is_pixel ? px / p.width : 0u;
    bool stale = false, loaded = false, front_able = false;
    float depth = 0.f;
    for (uint32_t base = 0u; base < p.n_rects; base += kStaleChunk) {
        const uint32_t m = p.n_rects - base < kStaleChunk ? p.n_rects - base : kStaleChunk;
        if (threadIdx.x < m) chunk[threadIdx.x] = reinterpret_cast<const uint4 *>(p.rects)[base + threadIdx.x];  // base + threadIdx.x < n_rects
        __syncthreads();
        if (is_pixel && !stale) {
            for (uint32_t i = 0u; i < m; i++) {
                const uint4 rc = chunk[i];
                if (x < (rc.x & 0xFFFFu) || x >= (rc.y & 0xFFFFu) || y < (rc.x >> 16) || y >= (rc.y >> 16)) continue;
                if (!p.depth_test) { stale = true; break; }
                if (!loaded) {  // px < count: inside both planes
                    const uint32_t hi = reinterpret_cast<const uint32_t *>(p.color)[(size_t)px * 2u + 1u];  // blue | alpha << 16
                    const float alpha = (float)__builtin_bit_cast(_Float16, (uint16_t)(hi >> 16));
                    depth = p.depth[px];
                    // a world pixel (clear sign bit: not UI, not "no layer", not -0.0) that is opaque (not NaN, not the marker)
                    front_able = !(__builtin_bit_cast(uint32_t, depth) >> 31) && alpha >= 1.0f;
                    loaded = true;
                }
                // (a NaN depth compares false: stale)
                if (!(front_able && depth < __builtin_bit_cast(float, rc.z))) { stale = true; break; }
            }
        }
        // also the barrier before the next chunk overwrites this one; the answer is the whole workgroup's alike
        if (__syncthreads_and(stale || !is_pixel)) break;
    }
    block_count(__ballot(stale), stale_counts(p), stale_bitmap(p, nb));
}

__global__ void __launch_bounds__(1024) stale_scan_kernel(StaleParams p, uint32_t nb) {
    const uint32_t n_stale = scan_block_counts(stale_counts(p), stale_offsets(p, nb), nb);
    if (threadIdx.x == 0u) {
        StaleRecord rec;
        rec.head = rank_list_record(n_stale, p.n, p.max_stale, p.skip_stale, p.cursor);
        rec.pad[0] = rec.pad[1] = 0u;
        *reinterpret_cast<StaleRecord *>(p.scratch) = rec;
    }
}

// blocks [0, nbc): the stale ranks (nbc = 0: nothing was looked at, the record is not read, g = 0); blocks from nbc on: the picker picks
__global__ void __launch_bounds__(256) stale_write_kernel(StaleParams p, uint32_t nbc) {
    const uint32_t g = nbc ? reinterpret_cast<const StaleRecord *>(p.scratch)->head.n_from_set : 0u;  // <= n
    if (blockIdx.x < nbc)
        write_set_ranks(p.order, p.out, stale_counts(p), stale_offsets(p, nbc), stale_bitmap(p, nbc), p.skip_stale, g);
    else
        write_picks(p.order, p.out, p.count, p.n, g, p.cursor, (blockIdx.x - nbc) * kStaleBlock + threadIdx.x);
}

}  // namespace

hipError_t launch_pick_stale(const StaleParams &p, hipStream_t stream) {
    if (!p.count || !p.n) return hipSuccess;
    const uint32_t nb = stale_blocks(p.count), nbc = (p.n_rects && p.max_stale) ? nb : 0u;
    if (nbc) {
        stale_count_kernel<<<nb, kStaleBlock, 0, stream>>>(p, nb);
        stale_scan_kernel<<<1, 1024, 0, stream>>>(p, nb);
    }
    stale_write_kernel<<<nbc + (p.n + kStaleBlock - 1u) / kStaleBlock, kStaleBlock, 0, stream>>>(p, nbc);
    return hipGetLastError();
}

}  // namespace aic
