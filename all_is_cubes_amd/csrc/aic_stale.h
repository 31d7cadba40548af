// aic_stale.h -- the picker of the pixels a scene change made stale (aic_stale.hip) as the host ABI code sees it: the scratch layout, the record read
// back and the launch.
//
// aic_pick_stale is aic_pick_pixels with the unknown set replaced by the stale set S of a resident Split frame: the pixels inside at least one of the
// caller's screen rectangles that does not keep them out (with AIC_STALE_DEPTH_TEST a rectangle keeps out an opaque world pixel whose depth lies in front
// of it). The exact rule is in DESIGN.md 4.17; tests/stale_ref.py is that text in NumPy. The three phases are aic_pick.hip's (count, scan, write); what
// the pickers share of them is aic_rank_list.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "aic_rank_list.h"

namespace aic {

constexpr uint32_t kStaleBlock = 256;  // ranks per scan block: one per thread (aic_pick.h's kPickBlock)
constexpr uint32_t kStaleChunk = 256;  // rectangles staged through LDS at a time: one per thread, 4 KB

// A rectangle as the device holds it: 16 bytes, the layout of aic_stale_rect.
struct StaleRect {
    uint32_t x0y0, x1y1;  // x | y << 16; columns [x0, x1), rows [y0, y1)
    float dmin;
    uint32_t reserved;
};

// What the device leaves for the host (the first 32 bytes of the scratch); written by the scan.
struct StaleRecord {
    RankListRecord head;  // the set: the stale ranks
    uint32_t pad[2];
};
static_assert(sizeof(StaleRecord) == 32 && offsetof(StaleRecord, head) == 0 && offsetof(StaleRecord, pad) == 24, "the scratch layout and the host's copy count on it");

// The scratch, in bytes: the record; per scan block its count of stale ranks and the count of those before it (32 bits each); per wave of a scan block
// the ballot of its stale ranks (64 bits: the rank-indexed bitmap); the rectangles.
inline uint32_t stale_blocks(uint64_t count) { return (uint32_t)((count + kStaleBlock - 1u) / kStaleBlock); }
inline size_t stale_bitmap_offset(uint64_t count) { return (sizeof(StaleRecord) + 8u * (size_t)stale_blocks(count) + 7u) & ~(size_t)7u; }
inline size_t stale_rects_offset(uint64_t count) { return (stale_bitmap_offset(count) + 8u * (size_t)(kStaleBlock / 64u) * stale_blocks(count) + 15u) & ~(size_t)15u; }
inline size_t stale_scratch_bytes(uint64_t count, uint32_t n_rects) { return stale_rects_offset(count) + sizeof(StaleRect) * (size_t)n_rects; }

struct StaleParams {
    const uint2 *color;     // [count] the frame's colour plane; only read with depth_test
    const float *depth;     // [count] its depth plane
    const uint32_t *order;  // [count], or nullptr: row-major
    uint32_t *out;          // [n]
    unsigned char *scratch; // stale_scratch_bytes(count, n_rects); only touched with n_rects > 0 and max_stale > 0
    const StaleRect *rects; // [n_rects], inside the scratch
    uint32_t width, count;  // count = width * height: at most 65535^2, below 2^32
    uint32_t n, max_stale;
    uint32_t n_rects, depth_test;
    unsigned long long skip_stale, cursor;
};

// Queues the call on `stream`: with n_rects > 0 and max_stale > 0 the count of every scan block (which leaves the bitmap), the scan and the record, then
// the write of both parts of the list; otherwise the write of the picker's picks alone. Returns the first failure of what it queued. count and n are not
// zero.
hipError_t launch_pick_stale(const StaleParams &p, hipStream_t stream);

}  // namespace aic
