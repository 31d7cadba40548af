// aic_stale_blocks.h -- the finder of the cubes that hold given block indices (aic_stale_blocks.hip) as the host ABI code sees it: the scratch layout,
// the record read back and the launches.
//
// aic_find_block_cubes answers "which cubes hold a block of this set" from the layer's resident cube grid, as runs along z: a re-evaluated block
// (aic_replace_block(s)) leaves the grid as it is and changes what those cubes look like, so their boxes are what aic_pick_stale_cubes needs to repair a
// resident frame narrowly. aic_pick_stale_blocks writes the boxes straight behind the caller's own in aic_pick_stale_cubes' scratch. The exact rule is in
// DESIGN.md 4.20; tests/stale_blocks_ref.py is that text in NumPy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aic {

constexpr uint32_t kBlockCubesLanes = 256;    // lanes of a workgroup
constexpr uint32_t kBlockCubesPerLane = 8;    // consecutive grid entries of a lane: one 16-byte load
constexpr uint32_t kBlockCubesGroup = kBlockCubesLanes * kBlockCubesPerLane;  // entries of a workgroup
constexpr uint32_t kBlockSetWords = 2048;     // 65536 block indices x 1 bit: the most the set can hold

// What the count leaves for the host (the first 64 bytes of the scratch). The host writes the initial value -- counts 0, lo all ones, hi 0 -- with the
// set, in one copy; the count's workgroups move the bounds with integer atomics, which are order-free, and one workgroup sums the counts: the same bytes
// on every run.
struct BlockCubesRecord {
    unsigned long long n_cubes, n_runs;
    uint32_t lo[3];  // grid coordinates (0 .. size - 1) of the matches' lowest corner
    uint32_t hi[3];  // ... and of their upper corner, exclusive
    uint32_t pad[6];
};
static_assert(sizeof(BlockCubesRecord) == 64, "the record is 64 bytes");

// The scratch, in bytes: the record; the set (set_words 32-bit words, bit b of word w: block index 32 w + b); per workgroup its count of run starts
// (low half) and run ends (high half; both at most 2048); per workgroup the starts and the ends before it (32 bits each: only made when the runs are
// written, and then there are at most 2^32 - 1 of them; until then the first of the two holds the workgroup's count of matches).
inline uint64_t block_cubes_groups(uint64_t n) { return (n + kBlockCubesGroup - 1u) / kBlockCubesGroup; }
inline size_t block_cubes_set_offset() { return sizeof(BlockCubesRecord); }
inline size_t block_cubes_counts_offset(uint32_t set_words) { return (block_cubes_set_offset() + 4u * (size_t)set_words + 15u) & ~(size_t)15u; }
inline size_t block_cubes_offsets_offset(uint32_t set_words, uint64_t n) { return (block_cubes_counts_offset(set_words) + 4u * (size_t)block_cubes_groups(n) + 15u) & ~(size_t)15u; }
inline size_t block_cubes_scratch_bytes(uint32_t set_words, uint64_t n) { return block_cubes_offsets_offset(set_words, n) + 8u * (size_t)block_cubes_groups(n); }

struct BlockCubesParams {
    const uint16_t *grid;     // [n] the layer's cube grid, Z-major; the pool goes on behind it and is never read
    unsigned long long n;     // sx * sy * sz, not 0; at most 2^31 - 1 workgroups: n <= 2048 x (2^31 - 1)
    uint32_t sx, sy, sz;
    uint32_t index_mask;      // a grid entry's block index = entry & index_mask (kCubeIndexMask when the entries carry tags, else 0xffff)
    uint32_t set_words;       // ceil(the layer's block count / 32), at most kBlockSetWords
    int32_t lo[3];            // the space's lower corner
    unsigned char *scratch;   // block_cubes_scratch_bytes(set_words, n)
    int32_t *boxes;           // [n_runs][6], written by launch_write_block_cubes
    uint32_t n_runs;          // what the record said after the count: no box at or past it is written
};

// Queues the count and the sum of its counts on `stream`: record and set are in the scratch already (copied on the same stream). Afterwards the record is
// final and every workgroup's counts are stored.
hipError_t launch_count_block_cubes(const BlockCubesParams &p, hipStream_t stream);
// Queues the scan of the workgroups' counts and the write of boxes[n_runs][6], sorted by a run's first entry. The grid must be what the count saw.
hipError_t launch_write_block_cubes(const BlockCubesParams &p, hipStream_t stream);

}  // namespace aic
