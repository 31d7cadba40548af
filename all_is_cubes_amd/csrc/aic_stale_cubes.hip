// aic_stale_cubes.hip -- the picker of the pixels changed blocks and changed light made stale, on gfx950 (aic_stale_cubes.h; DESIGN.md 4.19, which
// tests/stale_cubes_ref.py follows).
//
//  * Project: a lane per box or light cube, in f64 (aic_stale_rect_math.h: aic_stale_rects' own arithmetic; a light cube q is the box [q, q + 1) grown by
//    one). It stores the 24-byte rectangle, all zero for a dropped one. A wave adds its ballot of non-empty rectangles to the record with one atomic, and
//    ORs the record's whole-frame flag when a rectangle is the whole frame and no depth bound of it can keep a pixel out under the call's flags.
//  * Mark: a wave per rectangle (four to a workgroup); its lanes go over the rectangle's (row, word) pairs of the pixel bitmap. A lane forms its word's
//    mask from the column range, reads the word (bits are only ever set: an old value costs at most an atomic that sets nothing new) and drops what is
//    set already; with a depth flag it then reads depth and alpha of the pixels still wanted -- up to 32, consecutive along the row -- and drops those the
//    rectangle keeps out; what is left goes in with one atomicOr. OR is order-free: the bitmap is the same on every run. A rectangle the projection
//    flagged as the whole frame is left out, and under that flag every wave leaves at once.
//  * Count / scan / write: aic_stale.hip's compaction, which both take from aic_rank_list.h; rank r is stale when the bit of pixel order[r] is set, or,
//    under the whole-frame flag, when order[r] is a pixel at all. The scan keeps the record's two projection counters.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_stale_cubes.h"
#include "aic_stale_rect_math.h"

namespace aic {

namespace {

static_assert(kStaleCubesBlock == kRankBlock, "aic_rank_list.h's scan block");

AIC_DEV StaleCubesRecord *cubes_record(const StaleCubesParams &p) { return reinterpret_cast<StaleCubesRecord *>(p.scratch); }
AIC_DEV uint32_t *cubes_pixmap(const StaleCubesParams &p) { return reinterpret_cast<uint32_t *>(p.scratch + sizeof(StaleCubesRecord)); }
AIC_DEV uint32_t cubes_row_words(const StaleCubesParams &p) { return (p.width + 31u) / 32u; }
// the offsets are aic_stale_cubes.h's
AIC_DEV uint32_t *cubes_counts(const StaleCubesParams &p) {
    return reinterpret_cast<uint32_t *>(p.scratch + ((sizeof(StaleCubesRecord) + 4u * (size_t)cubes_row_words(p) * p.height + 7u) & ~(size_t)7u));
}
AIC_DEV uint32_t *cubes_offsets(const StaleCubesParams &p, uint32_t nb) { return cubes_counts(p) + nb; }
// word [block * 4 + wave]
AIC_DEV unsigned long long *cubes_ballots(const StaleCubesParams &p, uint32_t nb) { return reinterpret_cast<unsigned long long *>(cubes_counts(p) + 2u * (size_t)nb); }

// which of a rectangle's two depth bounds can keep a pixel out under the call's flags
AIC_DEV bool front_usable(const StaleCubesParams &p, float dmin) { return p.depth_front && dmin > -__builtin_inff(); }
AIC_DEV bool behind_usable(const StaleCubesParams &p, bool is_light, float dmax) { return p.depth_behind && is_light && dmax < __builtin_inff(); }
// the whole frame and nothing to keep a pixel out: the projection raises the flag, the marks leave the rectangle out
AIC_DEV bool whole_unbounded(const StaleCubesParams &p, const StaleCubeRect &rc, bool is_light) {
    return rc.x0 == 0u && rc.y0 == 0u && rc.x1 == p.width && rc.y1 == p.height && !front_usable(p, rc.dmin) && !behind_usable(p, is_light, rc.dmax);
}

__global__ void __launch_bounds__(256) stale_cubes_project_kernel(StaleCubesParams p, uint32_t n_total) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kStaleCubesBlock + threadIdx.x;
    bool holds = false, whole = false;
    if (i < n_total) {
        const bool is_light = i >= p.n_boxes;
        StaleBounds b;
        if (!is_light) {
            const int32_t *box = p.boxes + i * 6u;
            b = stale_bounds_of(p.m, p.width, p.height, box[0], box[1], box[2], box[3], box[4], box[5], p.expand);
        } else {
            const int32_t *q = p.light_cubes + (i - p.n_boxes) * 3u;
            const int64_t x = q[0], y = q[1], z = q[2];  // (64 bits: q + 1 of a cube at the i32 edge)
            b = stale_bounds_of(p.m, p.width, p.height, x, y, z, x + 1, y + 1, z + 1, 1);
        }
        StaleCubeRect rc;
        rc.x0 = b.x0; rc.y0 = b.y0; rc.x1 = b.x1; rc.y1 = b.y1;
        rc.dmin = b.dmin; rc.dmax = b.dmax;
        p.rects[i] = rc;
        holds = rc.x0 < rc.x1 && rc.y0 < rc.y1;
        whole = holds && whole_unbounded(p, rc, is_light);
    }
    const unsigned long long hb = __ballot(holds), wb = __ballot(whole);
    if ((threadIdx.x & 63u) == 0u) {
        if (hb) atomicAdd(&cubes_record(p)->n_rects, (uint32_t)__popcll(hb));
        if (wb) atomicOr(&cubes_record(p)->whole_frame, 1u);
    }
}

__global__ void __launch_bounds__(256) stale_cubes_mark_kernel(StaleCubesParams p, uint32_t n_total) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long ri = (unsigned long long)blockIdx.x * (kStaleCubesBlock / 64u) + (threadIdx.x >> 6);
    if (ri >= n_total) return;  // the whole wave alike
    if (cubes_record(p)->whole_frame) return;  // the projection found every pixel stale: the count does not look at the bitmap
    const StaleCubeRect rc = p.rects[ri];
    if (rc.x0 >= rc.x1 || rc.y0 >= rc.y1) return;
    const bool is_light = ri >= p.n_boxes;
    if (whole_unbounded(p, rc, is_light)) return;
    const bool front = front_usable(p, rc.dmin), behind = behind_usable(p, is_light, rc.dmax);
    uint32_t *pix = cubes_pixmap(p);
    const uint32_t wpr = cubes_row_words(p);
    const uint32_t wx0 = rc.x0 >> 5, nw = ((rc.x1 - 1u) >> 5) - wx0 + 1u;  // x1 <= width: the last word is below wpr
    const uint32_t total = nw * (rc.y1 - rc.y0);                           // at most 2048 x 65535
    for (uint32_t i = lane; i < total; i += 64u) {
        const uint32_t row = rc.y0 + i / nw, wc = wx0 + i % nw;  // row < y1 <= height
        const uint32_t c0 = wc * 32u;
        const uint32_t lo = (rc.x0 > c0 ? rc.x0 : c0) - c0, hi = (rc.x1 < c0 + 32u ? rc.x1 : c0 + 32u) - c0;  // 0 <= lo < hi <= 32
        const uint32_t mask = (hi == 32u ? 0xFFFFFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
        uint32_t *word = pix + (size_t)row * wpr + wc;
        uint32_t need = mask & ~*word;
        if (front || behind) {
            uint32_t todo = need;
            while (todo) {
                const uint32_t b = (uint32_t)__builtin_ctz(todo);
                todo &= todo - 1u;
                const size_t px = (size_t)row * p.width + c0 + b;  // c0 + b < x1 <= width: inside both planes
                const uint32_t ba = reinterpret_cast<const uint32_t *>(p.color)[px * 2u + 1u];  // blue | alpha << 16
                const float alpha = (float)__builtin_bit_cast(_Float16, (uint16_t)(ba >> 16));
                const float depth = p.depth[px];
                const bool world = !(__builtin_bit_cast(uint32_t, depth) >> 31);  // not UI, not "no layer", not -0.0
                // (a NaN depth compares false both times: stale; alpha > -0.5 is the gap fill's validity test: not NaN, not the marker's -1)
                const bool kept_out = (front && world && alpha >= 1.0f && depth < rc.dmin) || (behind && world && alpha > -0.5f && depth > rc.dmax);
                if (kept_out) need &= ~(1u << b);
            }
        }
        if (need) atomicOr(word, need);
    }
}

__global__ void __launch_bounds__(256) stale_cubes_count_kernel(StaleCubesParams p, uint32_t nb) {
    const uint32_t count = p.width * p.height;
    const uint32_t r = blockIdx.x * kStaleCubesBlock + threadIdx.x;  // (count rounded up to whole blocks is still below 2^32)
    const uint32_t px = r < count ? rank_pixel(p.order, r) : 0xFFFFFFFFu;
    bool stale = px < count;  // an entry that is no pixel is never stale
    if (stale && !cubes_record(p)->whole_frame) {
        const uint32_t x = px % p.width, y = px / p.width;
        stale = (cubes_pixmap(p)[(size_t)y * cubes_row_words(p) + (x >> 5)] >> (x & 31u)) & 1u;
    }
    block_count(__ballot(stale), cubes_counts(p), cubes_ballots(p, nb));
}

__global__ void __launch_bounds__(1024) stale_cubes_scan_kernel(StaleCubesParams p, uint32_t nb) {
    const uint32_t n_stale = scan_block_counts(cubes_counts(p), cubes_offsets(p, nb), nb);
    // (the head alone: n_rects and whole_frame stay the projection's)
    if (threadIdx.x == 0u) cubes_record(p)->head = rank_list_record(n_stale, p.n, p.max_stale, p.skip_stale, p.cursor);
}

// blocks [0, nbc): the stale ranks (nbc = 0: nothing was looked at, the record is not read, g = 0); blocks from nbc on: the picker picks
__global__ void __launch_bounds__(256) stale_cubes_write_kernel(StaleCubesParams p, uint32_t nbc) {
    const uint32_t g = nbc ? cubes_record(p)->head.n_from_set : 0u;  // <= n
    if (blockIdx.x < nbc)
        write_set_ranks(p.order, p.out, cubes_counts(p), cubes_offsets(p, nbc), cubes_ballots(p, nbc), p.skip_stale, g);
    else
        write_picks(p.order, p.out, p.width * p.height, p.n, g, p.cursor, (blockIdx.x - nbc) * kStaleCubesBlock + threadIdx.x);
}

uint32_t total_of(const StaleCubesParams &p) { return p.n_boxes + p.n_light_cubes; }  // the host has checked the sum

}  // namespace

hipError_t launch_project_stale_cubes(const StaleCubesParams &p, hipStream_t stream) {
    const uint32_t n_total = total_of(p);
    if (!n_total) return hipSuccess;
    hipError_t e = hipMemsetAsync(p.scratch, 0, sizeof(StaleCubesRecord), stream);
    if (e != hipSuccess) return e;
    stale_cubes_project_kernel<<<(uint32_t)(((uint64_t)n_total + kStaleCubesBlock - 1u) / kStaleCubesBlock), kStaleCubesBlock, 0, stream>>>(p, n_total);
    return hipGetLastError();
}

hipError_t launch_pick_stale_cubes(const StaleCubesParams &p, hipStream_t stream) {
    const uint64_t count = (uint64_t)p.width * p.height;
    if (!count || !p.n) return hipSuccess;
    const uint32_t n_total = total_of(p);
    const uint32_t nb = stale_cubes_blocks(count), nbc = (n_total && p.max_stale) ? nb : 0u;
    if (nbc) {
        // record and pixel bitmap, which lie together
        hipError_t e = hipMemsetAsync(p.scratch, 0, sizeof(StaleCubesRecord) + 4u * (size_t)stale_cubes_row_words(p.width) * p.height, stream);
        if (e != hipSuccess) return e;
        stale_cubes_project_kernel<<<(uint32_t)(((uint64_t)n_total + kStaleCubesBlock - 1u) / kStaleCubesBlock), kStaleCubesBlock, 0, stream>>>(p, n_total);
        stale_cubes_mark_kernel<<<(uint32_t)(((uint64_t)n_total + 3u) / 4u), kStaleCubesBlock, 0, stream>>>(p, n_total);
        stale_cubes_count_kernel<<<nb, kStaleCubesBlock, 0, stream>>>(p, nb);
        stale_cubes_scan_kernel<<<1, 1024, 0, stream>>>(p, nb);
    }
    stale_cubes_write_kernel<<<nbc + (p.n + kStaleCubesBlock - 1u) / kStaleCubesBlock, kStaleCubesBlock, 0, stream>>>(p, nbc);
    return hipGetLastError();
}

}  // namespace aic
