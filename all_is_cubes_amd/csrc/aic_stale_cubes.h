// aic_stale_cubes.h -- the picker of the pixels that changed blocks and changed light made stale (aic_stale_cubes.hip) as the host ABI code sees it: the
// scratch layout, the record read back and the launches.
//
// aic_pick_stale_cubes is aic_pick_stale for any number of changed boxes and light cubes: the device projects them (aic_stale_rect_math.h, the arithmetic
// of aic_stale_rects), marks every rectangle's pixels in a pixel-indexed bitmap -- one wave a rectangle, so the cost follows the rectangles' area and
// not pixels x rectangles --, and compacts the ranks whose pixel's bit is set. The exact rule is in DESIGN.md 4.19; tests/stale_cubes_ref.py is that
// text in NumPy. The compaction (count, scan, write) is aic_stale.hip's with another predicate; what the two share of it is aic_rank_list.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "aic_rank_list.h"

namespace aic {

constexpr uint32_t kStaleCubesBlock = 256;  // ranks per scan block, boxes per projection block, four rectangles (a wave each) per mark block

// A projected rectangle as the device holds it and aic_probe_stale_cube_rects copies it back: 24 bytes, the layout of aic_stale_cube_rect. All zero:
// dropped.
struct StaleCubeRect {
    uint32_t x0, y0, x1, y1;  // columns [x0, x1), rows [y0, y1)
    float dmin, dmax;
};

// What the device leaves for the host (the first 32 bytes of the scratch). n_rects and whole_frame are zeroed in the stream and raised by the projection;
// the rest is written by the scan.
struct StaleCubesRecord {
    RankListRecord head;   // the set: the stale ranks
    uint32_t n_rects;      // rectangles that hold a pixel
    uint32_t whole_frame;  // not 0: a rectangle was the whole frame with no usable depth bound: every pixel is stale
};

static_assert(sizeof(StaleCubesRecord) == 32 && offsetof(StaleCubesRecord, head) == 0 && offsetof(StaleCubesRecord, n_rects) == 24 && offsetof(StaleCubesRecord, whole_frame) == 28,
              "the scratch layout, the projection's atomics and the host's copy count on it");

// The scratch, in bytes: the record; the pixel bitmap (height rows of ceil(width / 32) words: a row never shares a word with the next) -- the two are
// zeroed by one memset --; per scan block its count of stale ranks and the count of those before it (32 bits each); per wave of a scan block the ballot
// of its stale ranks (64 bits); the rectangles; the caller's boxes and light cubes.
inline uint32_t stale_cubes_blocks(uint64_t count) { return (uint32_t)((count + kStaleCubesBlock - 1u) / kStaleCubesBlock); }
inline uint32_t stale_cubes_row_words(uint32_t width) { return (width + 31u) / 32u; }
inline size_t stale_cubes_pixmap_offset() { return sizeof(StaleCubesRecord); }
inline size_t stale_cubes_counts_offset(uint32_t width, uint32_t height) { return (stale_cubes_pixmap_offset() + 4u * (size_t)stale_cubes_row_words(width) * height + 7u) & ~(size_t)7u; }
inline size_t stale_cubes_ballots_offset(uint32_t width, uint32_t height) {
    return (stale_cubes_counts_offset(width, height) + 8u * (size_t)stale_cubes_blocks((uint64_t)width * height) + 7u) & ~(size_t)7u;
}
inline size_t stale_cubes_rects_offset(uint32_t width, uint32_t height) {
    return (stale_cubes_ballots_offset(width, height) + 8u * (size_t)(kStaleCubesBlock / 64u) * stale_cubes_blocks((uint64_t)width * height) + 15u) & ~(size_t)15u;
}
inline size_t stale_cubes_input_offset(uint32_t width, uint32_t height, uint64_t n_total) { return (stale_cubes_rects_offset(width, height) + sizeof(StaleCubeRect) * (size_t)n_total + 15u) & ~(size_t)15u; }
inline size_t stale_cubes_scratch_bytes(uint32_t width, uint32_t height, uint32_t n_boxes, uint32_t n_light_cubes) {
    return stale_cubes_input_offset(width, height, (uint64_t)n_boxes + n_light_cubes) + 24u * (size_t)n_boxes + 12u * (size_t)n_light_cubes;
}

struct StaleCubesParams {
    const uint2 *color;     // [count] the frame's colour plane; only read with a depth flag
    const float *depth;     // [count] its depth plane
    const uint32_t *order;  // [count], or nullptr: row-major
    uint32_t *out;          // [n]
    unsigned char *scratch; // stale_cubes_scratch_bytes(...); only touched when anything is looked at
    const int32_t *boxes;        // [n_boxes][6], inside the scratch
    const int32_t *light_cubes;  // [n_light_cubes][3], inside the scratch
    StaleCubeRect *rects;        // [n_boxes + n_light_cubes], inside the scratch
    double m[16];           // view_projection
    uint32_t width, height; // at most 65535 each: count = width * height is below 2^32
    uint32_t n, max_stale;  // max_stale = 0: nothing is looked at
    uint32_t n_boxes, n_light_cubes;  // their sum is below 2^32
    int32_t expand;
    uint32_t depth_front, depth_behind;  // AIC_STALE_DEPTH_TEST, AIC_STALE_DEPTH_BEHIND
    unsigned long long skip_stale, cursor;
};

// Queues the call on `stream`: with rectangles and max_stale > 0 the memset of record and bitmap, the projection, the marks, the count of every scan
// block, the scan and the record, then the write of both parts of the list; otherwise the write of the picker's picks alone. Returns the first failure of
// what it queued. count and n are not zero.
hipError_t launch_pick_stale_cubes(const StaleCubesParams &p, hipStream_t stream);
// Queues the projection alone (the probe): rects[n_boxes + n_light_cubes] afterwards; the record's two counters are zeroed first and raised.
hipError_t launch_project_stale_cubes(const StaleCubesParams &p, hipStream_t stream);

}  // namespace aic
