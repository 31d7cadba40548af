// aic_bit_gather.h -- the ordered compaction of an LDS bitmap by a whole workgroup, shared by the light updater's gather kernel (aic_light.hip: the
// ordered reduction of a cube's terms and dependencies) and the light-ray records (aic_light_rays.hip: the same reduction, and the records in the
// reference's order). Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aic {
namespace {

constexpr uint32_t kOrderCap = 2048u;   // set bits gathered per pass of the ordered reduction

// Gathers set bits of bits[*word_io, n_words) into order[] in ascending order -- all of them if they fit kOrderCap, else
// the longest prefix of words that does -- and advances *word_io. All threads of the block take part (no divergence
// around the call): each counts and then writes out a contiguous stretch of words; `s_scan` (>= 4 words) carries the
// waves' counts. Returns the number gathered; 0 = nothing left; 0xffffffff = this span was empty but words remain.
__device__ uint32_t gather_set_bits(const uint32_t *bits, uint32_t n_words, uint32_t *word_io, uint32_t *order, uint32_t tid, uint32_t nt, uint32_t *s_scan) {
    const uint32_t w0 = *word_io;
    if (w0 >= n_words) return 0u;
    const uint32_t wl = tid & 63u, wid = tid >> 6, nw = nt >> 6;
    uint32_t span = n_words - w0, a, e, count, incl, total, base;
    for (;;) {
        const uint32_t per = (span + nt - 1u) / nt;
        a = min(w0 + tid * per, w0 + span);
        e = min(a + per, w0 + span);
        count = 0u;
        for (uint32_t w = a; w < e; w++) count += __popc(bits[w]);
        incl = count;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if ((int)wl >= d) incl += up;
        }
        if (wl == 63u) s_scan[wid] = incl;
        __syncthreads();
        base = 0u; total = 0u;
        for (uint32_t q = 0u; q < nw; q++) {
            const uint32_t t = s_scan[q];
            if (q < wid) base += t;
            total += t;
        }
        __syncthreads();
        if (total <= kOrderCap || span <= kOrderCap / 32u) break;
        span = max(kOrderCap / 32u, span / 2u);
    }
    uint32_t at = base + incl - count;
    for (uint32_t w = a; w < e; w++) {
        uint32_t v = bits[w];
        while (v) { const uint32_t bpos = __ffs(v) - 1u; v &= v - 1u; order[at++] = w * 32u + bpos; }
    }
    __syncthreads();
    *word_io = w0 + span;
    return total == 0u ? 0xffffffffu : total;
}

}  // namespace
}  // namespace aic
