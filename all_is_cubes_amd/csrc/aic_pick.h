// aic_pick.h -- the device-side pixel picker (aic_pick.hip) as the host ABI code sees it: the scratch layout, the record read back and the launch.
//
// aic_pick_pixels writes the next pixel indices for aic_trace_pixels into device memory: first the pixels the context's last reprojection knows
// nothing about (the texels of the splat image R that fail the gap fill's validity test), in the picker's centre-first order, then PixelPicker's own
// sequence from a cursor (all-is-cubes-gpu/src/raytrace_to_texture.rs:838-908, restated under aic_pixel_order in include/aic_hip.h). The exact list
// is in DESIGN.md "Picking pixels on the device"; tests/pick_ref.py is that text in NumPy.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "aic_rank_list.h"

namespace aic {

constexpr uint32_t kPickBlock = 256;  // ranks per scan block: one per thread

// What the device leaves for the host (the first 32 bytes of the scratch); written by the scan, so only by a call with max_unknown > 0.
struct PickRecord {
    RankListRecord head;  // the set: the unknown ranks
    uint32_t pad[2];
};
static_assert(sizeof(PickRecord) == 32 && offsetof(PickRecord, head) == 0 && offsetof(PickRecord, pad) == 24, "pick_scratch_words and the host's copy count on it");

// The scratch, in 32-bit words: the record, then per scan block its count of unknown ranks and the count of those before it.
inline uint32_t pick_blocks(uint64_t count) { return (uint32_t)((count + kPickBlock - 1u) / kPickBlock); }
inline size_t pick_scratch_words(uint64_t count) { return sizeof(PickRecord) / 4u + 2u * (size_t)pick_blocks(count); }

struct PickParams {
    const uint2 *R;         // [count] the splat image of the last reprojection; only read with max_unknown > 0
    const uint32_t *order;  // [count], or nullptr: row-major
    uint32_t *out;          // [n]
    uint32_t *scratch;      // pick_scratch_words(count); only touched with max_unknown > 0
    uint32_t count;         // width * height: at most 65535^2, below 2^32
    uint32_t n, max_unknown;
    unsigned long long skip_unknown, cursor;
};

// Queues the call on `stream`: with max_unknown > 0 the count of every scan block, the scan and the record, then the write of both parts of the
// list; with max_unknown == 0 the write alone. Returns the first failure of what it queued. count and n are not zero.
hipError_t launch_pick(const PickParams &p, hipStream_t stream);

}  // namespace aic
