// aic_rank_list.h -- what the pixel pickers share (aic_pick.hip, aic_stale.hip, aic_stale_cubes.hip): the stable compaction of a set of ranks and the
// picker's own picks behind it, each rule written once. DESIGN.md "Picking pixels on the device" states the list; tests/pick_ref.py is that text in NumPy.
//
// Rank r of the picker's order holds pixel order[r]. A picker decides with a predicate of its own which ranks are in its set (unknown, stale); the list
// it writes is the set's ranks skip .. skip + g in rank order, g = min(n, max, what is left of the set), then n - g picks of PixelPicker's sequence from
// a cursor. The three phases on the device:
//
//  * Count: a scan block is 256 consecutive ranks, a lane each. A wave64's ballot of the predicate is its popcount (and, where the picker stores it, its
//    part of a rank-indexed bitmap); the four waves add through LDS and the block leaves one number (block_count).
//  * Scan: one workgroup of 1024 walks the block counts 1024 at a time (wave scan by shuffles, the sixteen wave sums through LDS, a running carry) and
//    leaves for every block the set's ranks before it (scan_block_counts); lane 0 then forms the record the host reads back (rank_list_record).
//  * Write: in the first grid part a lane's position in the set's list is block offset + the popcounts of the block's earlier waves + mbcnt, and it
//    stores its pixel when skip <= position < skip + g; a block whose range misses that window leaves at once (RankWindow; write_set_ranks where the
//    ballots were stored). The second part writes the picker's picks behind the g entries (write_picks); g comes from the record, so the host never
//    waits between the launches.
//
// Nothing here knows a picker's parameters: the kernels, their scratch layouts and their predicates stay in the pickers' own files.
#pragma once

#include <stdint.h>

namespace aic {

// The head of what every picker leaves for the host at the start of its scratch, written by its scan. A picker's record is this and two words of its
// own: 32 bytes.
struct RankListRecord {
    unsigned long long n_set;        // ranks in the set
    unsigned long long next_cursor;  // cursor + n_from_order
    uint32_t n_from_set, n_from_order;
};
static_assert(sizeof(RankListRecord) == 24, "the head of the pickers' records");

}  // namespace aic

#if defined(__HIPCC__)

#include <hip/hip_runtime.h>

#ifndef AIC_DEV
#define AIC_DEV __device__ __forceinline__
#endif

namespace aic {

constexpr uint32_t kRankBlock = 256;  // ranks per scan block: one per thread, four waves

// the pixel of rank r < count
AIC_DEV uint32_t rank_pixel(const uint32_t *order, uint32_t r) { return order ? order[r] : r; }

// lanes of the wave below this one whose bit is set in `b`
AIC_DEV uint32_t lanes_before(unsigned long long b) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)); }

// pick k of PixelPicker's sequence as a rank (include/aic_hip.h under aic_pixel_order); all 64-bit
AIC_DEV uint32_t pick_rank(unsigned long long k, uint32_t count) {
    const uint32_t quarter = count / 4u, central = quarter < 60000u ? quarter : 60000u;
    if (central == 0u) return (uint32_t)(k % count);
    const unsigned long long h = k >> 1;
    return (k & 1ull) ? central + (uint32_t)(h % (count - central)) : (uint32_t)(h % central);
}

// the record of a call that found n_set ranks in the set
AIC_DEV RankListRecord rank_list_record(unsigned long long n_set, uint32_t n, uint32_t max, unsigned long long skip, unsigned long long cursor) {
    const unsigned long long left = n_set > skip ? n_set - skip : 0ull;
    unsigned long long g = n < max ? n : max;
    if (left < g) g = left;
    RankListRecord rec;
    rec.n_set = n_set;
    rec.next_cursor = cursor + (unsigned long long)(n - (uint32_t)g);
    rec.n_from_set = (uint32_t)g;
    rec.n_from_order = n - (uint32_t)g;
    return rec;
}

// The end of a count kernel, by all 256 threads: `b` is the wave's ballot of the predicate. counts[block] becomes the block's popcount.
AIC_DEV void block_count(unsigned long long b, uint32_t *counts) {
    __shared__ uint32_t wave_n[kRankBlock / 64u];
    if ((threadIdx.x & 63u) == 0u) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}
// The same, and the wave's word goes to ballots[block * 4 + wave] for write_set_ranks.
AIC_DEV void block_count(unsigned long long b, uint32_t *counts, unsigned long long *ballots) {
    if ((threadIdx.x & 63u) == 0u) ballots[blockIdx.x * (kRankBlock / 64u) + (threadIdx.x >> 6)] = b;
    block_count(b, counts);
}

// A scan kernel, by one workgroup of 1024: offsets[i] becomes counts[0] + .. + counts[i - 1] for i < nb. Returns the sum of all counts (at most the
// number of ranks) to every thread.
AIC_DEV uint32_t scan_block_counts(const uint32_t *counts, uint32_t *offsets, uint32_t nb) {
    __shared__ uint32_t wave_sum[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;  // the set's ranks before this round's blocks
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
    return carry;
}

// The part [skip, skip + g) of the set's list as block blockIdx.x of a write kernel meets it.
struct RankWindow {
    unsigned long long lo, hi;  // g > 0: skip < n_set < 2^32
    unsigned long long b0;      // the set's ranks before the block

    // false: the block's range misses the window (the whole workgroup alike)
    AIC_DEV bool open(const uint32_t *counts, const uint32_t *offsets, unsigned long long skip, uint32_t g) {
        if (g == 0u) return false;
        lo = skip, hi = lo + g;
        b0 = offsets[blockIdx.x];
        const unsigned long long bn = counts[blockIdx.x];
        return !(b0 >= hi || b0 + bn <= lo);
    }
    // by a lane whose rank is in the set: `b` its wave's ballot, wave_off the set's ranks in the block's earlier waves
    AIC_DEV void store(uint32_t *out, uint32_t wave_off, unsigned long long b, uint32_t px) const {
        const unsigned long long pos = b0 + wave_off + lanes_before(b);
        if (pos >= lo && pos < hi) out[pos - lo] = px;  // pos - lo < g <= n
    }
};

// The first part of a write kernel whose count stored its ballots: block blockIdx.x's ranks of the set.
AIC_DEV void write_set_ranks(const uint32_t *order, uint32_t *out, const uint32_t *counts, const uint32_t *offsets, const unsigned long long *ballots, unsigned long long skip,
                             uint32_t g) {
    RankWindow win;
    if (!win.open(counts, offsets, skip, g)) return;
    const unsigned long long *words = ballots + (size_t)blockIdx.x * (kRankBlock / 64u);
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t wave_off = 0u;
    for (uint32_t w = 0u; w < kRankBlock / 64u - 1u; w++)
        if (w < wave) wave_off += (uint32_t)__popcll(words[w]);
    const unsigned long long b = words[wave];
    if (!((b >> (threadIdx.x & 63u)) & 1ull)) return;  // (a set bit: r < count and order[r] < count)
    win.store(out, wave_off, b, rank_pixel(order, blockIdx.x * kRankBlock + threadIdx.x));
}

// The second part of a write kernel, by thread j of it (n is at most 2048 x 65535): the picker's picks behind the g entries.
AIC_DEV void write_picks(const uint32_t *order, uint32_t *out, uint32_t count, uint32_t n, uint32_t g, unsigned long long cursor, uint32_t j) {
    if (j >= n - g) return;
    const uint32_t r = pick_rank(cursor + j, count);  // < count
    out[g + j] = rank_pixel(order, r);                // g + j < n
}

}  // namespace aic

#endif  // __HIPCC__
