// aic_stale.hip -- the picker of stale pixels on gfx950 (aic_stale.h; DESIGN.md 4.17, which tests/stale_ref.py follows).
//
// Rank r of the picker's order holds pixel order[r]; a rank is "stale" when that pixel lies inside a rectangle that does not keep it out. The stale ranks
// are compacted in rank order -- aic_pick.hip's stable stream compaction with another predicate, the same list on every run: nothing is ordered by an
// atomic --, and the rest of the list is PixelPicker's sequence from a cursor.
//
//  * Count: a scan block is 256 consecutive ranks, a lane each. The rectangles go through LDS 256 at a time (one 16-byte load a thread, then every lane
//    reads the same rectangle: a broadcast); a lane walks a chunk until a rectangle makes its pixel stale, and the block leaves the loop once every lane
//    has. With the depth test a lane loads its two texels once, at the first rectangle that contains it. A wave64's ballot of "stale" is its popcount and,
//    stored by one lane as a 64-bit word, its part of the rank-indexed bitmap; the four waves add through LDS and the block leaves one number.
//  * Scan: one workgroup of 1024 walks the block counts 1024 at a time (wave scan by shuffles, the sixteen wave sums through LDS, a running carry) and
//    leaves for every block the stale ranks before it; lane 0 then forms the record the host reads back.
//  * Write: the first grid part reads the bitmap instead of testing again; a lane's position in the rank list is block offset + the popcounts of the
//    block's earlier waves + mbcnt, and it stores its pixel when skip <= position < skip + g. A block whose range misses that window leaves at once. The
//    second part writes the picker picks behind the g entries; g comes from the record, so the host never waits between the launches.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_stale.h"

#ifndef AIC_DEV
#define AIC_DEV __device__ __forceinline__
#endif

namespace aic {

namespace {

AIC_DEV uint32_t *stale_counts(const StaleParams &p) { return reinterpret_cast<uint32_t *>(p.scratch + sizeof(StaleRecord)); }
AIC_DEV uint32_t *stale_offsets(const StaleParams &p, uint32_t nb) { return stale_counts(p) + nb; }
// word [block * 4 + wave]; the offset is stale_bitmap_offset's
AIC_DEV unsigned long long *stale_bitmap(const StaleParams &p, uint32_t nb) {
    return reinterpret_cast<unsigned long long *>(p.scratch + ((sizeof(StaleRecord) + 8u * (size_t)nb + 7u) & ~(size_t)7u));
}

// the pixel of rank r < count
AIC_DEV uint32_t rank_pixel(const StaleParams &p, uint32_t r) { return p.order ? p.order[r] : r; }

// lanes of the wave below this one whose bit is set in `b`
AIC_DEV uint32_t lanes_before(unsigned long long b) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)); }

__global__ void __launch_bounds__(256) stale_count_kernel(StaleParams p, uint32_t nb) {
    __shared__ uint4 chunk[kStaleChunk];
    __shared__ uint32_t wave_n[4];
    const uint32_t r = blockIdx.x * kStaleBlock + threadIdx.x;  // (count rounded up to whole blocks is still below 2^32)
    const uint32_t px = r < p.count ? rank_pixel(p, r) : 0xFFFFFFFFu;
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
    const unsigned long long b = __ballot(stale);
    if ((threadIdx.x & 63u) == 0u) {
        wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(b);
        stale_bitmap(p, nb)[blockIdx.x * (kStaleBlock / 64u) + (threadIdx.x >> 6)] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0u) stale_counts(p)[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

__global__ void __launch_bounds__(1024) stale_scan_kernel(StaleParams p, uint32_t nb) {
    __shared__ uint32_t wave_sum[16];
    const uint32_t *counts = stale_counts(p);
    uint32_t *offsets = stale_offsets(p, nb);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;  // stale ranks before this round's blocks; at most count
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
        const unsigned long long n_stale = carry;
        const unsigned long long left = n_stale > p.skip_stale ? n_stale - p.skip_stale : 0ull;
        unsigned long long g = p.n < p.max_stale ? p.n : p.max_stale;
        if (left < g) g = left;
        StaleRecord rec;
        rec.n_stale = n_stale;
        rec.next_cursor = p.cursor + (unsigned long long)(p.n - (uint32_t)g);
        rec.n_from_stale = (uint32_t)g;
        rec.n_from_order = p.n - (uint32_t)g;
        rec.pad[0] = rec.pad[1] = 0u;
        *reinterpret_cast<StaleRecord *>(p.scratch) = rec;
    }
}

// pick k of PixelPicker's sequence as a rank (include/aic_hip.h under aic_pixel_order); all 64-bit
AIC_DEV uint32_t pick_rank(unsigned long long k, uint32_t count) {
    const uint32_t quarter = count / 4u, central = quarter < 60000u ? quarter : 60000u;
    if (central == 0u) return (uint32_t)(k % count);
    const unsigned long long h = k >> 1;
    return (k & 1ull) ? central + (uint32_t)(h % (count - central)) : (uint32_t)(h % central);
}

// blocks [0, nbc): the stale ranks (nbc = 0: nothing was looked at, the record is not read, g = 0); blocks from nbc on: the picker picks
__global__ void __launch_bounds__(256) stale_write_kernel(StaleParams p, uint32_t nbc) {
    const uint32_t g = nbc ? reinterpret_cast<const StaleRecord *>(p.scratch)->n_from_stale : 0u;  // <= n
    if (blockIdx.x < nbc) {
        if (g == 0u) return;
        const unsigned long long lo = p.skip_stale, hi = lo + g;  // g > 0: skip < n_stale < 2^32
        const unsigned long long b0 = stale_offsets(p, nbc)[blockIdx.x], bn = stale_counts(p)[blockIdx.x];
        if (b0 >= hi || b0 + bn <= lo) return;  // the whole workgroup alike
        const unsigned long long *words = stale_bitmap(p, nbc) + (size_t)blockIdx.x * (kStaleBlock / 64u);
        const uint32_t wave = threadIdx.x >> 6;
        uint32_t wave_off = 0u;
        for (uint32_t w = 0u; w < kStaleBlock / 64u - 1u; w++)
            if (w < wave) wave_off += (uint32_t)__popcll(words[w]);
        const unsigned long long b = words[wave];
        if (!((b >> (threadIdx.x & 63u)) & 1ull)) return;  // (a set bit: r < count and order[r] < count)
        const unsigned long long pos = b0 + wave_off + lanes_before(b);
        if (pos >= lo && pos < hi) p.out[pos - lo] = rank_pixel(p, blockIdx.x * kStaleBlock + threadIdx.x);  // pos - lo < g <= n
        return;
    }
    const uint32_t j = (blockIdx.x - nbc) * kStaleBlock + threadIdx.x;  // (n is at most 2048 x 65535)
    if (j >= p.n - g) return;
    const uint32_t r = pick_rank(p.cursor + j, p.count);  // < count
    p.out[g + j] = rank_pixel(p, r);                      // g + j < n
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
