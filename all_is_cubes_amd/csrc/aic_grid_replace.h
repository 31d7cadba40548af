// aic_grid_replace.h -- the replacement of a layer's whole cube grid from device memory (aic_grid_replace.hip) as the host ABI code sees it: the scratch
// layout, the record read back and the launches.
//
// aic_replace_cube_grid takes the block index of every cube from an array in device memory, reports which cubes changed as runs along z -- the rule and
// the info of aic_find_block_cubes, with "the new index differs from the index the entry held" for its match -- and leaves the grid as aic_upload_space
// of the same indices would. aic_copy_cube_grid is the way back: the grid as plain indices. The exact rule is in DESIGN.md 4.23;
// tests/grid_replace_ref.py is that text in NumPy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aic {

constexpr uint32_t kGridReplaceLanes = 256;   // lanes of a workgroup
constexpr uint32_t kGridReplacePerLane = 8;   // consecutive grid entries of a lane: one 16-byte load from the grid and one from the caller's array
constexpr uint32_t kGridReplaceGroup = kGridReplaceLanes * kGridReplacePerLane;  // entries of a workgroup
constexpr uint32_t kGridReplaceClsWords = 1024;  // the class table of a grid that carries tags, staged in LDS: at most 16384 block indices x 2 bits (4 KB)

// What the count leaves for the host (the first 64 bytes of the scratch). The host writes the initial value -- counts and max_index 0, lo all ones, hi
// 0 --; the count's workgroups move the bounds and the maximum with integer atomics, which are order-free, and one workgroup sums the counts: the same
// bytes on every run.
struct GridReplaceRecord {
    unsigned long long n_cubes, n_runs;
    uint32_t lo[3];  // grid coordinates (0 .. size - 1) of the changed cubes' lowest corner
    uint32_t hi[3];  // ... and of their upper corner, exclusive
    uint32_t max_index;  // the largest entry of the caller's array, changed or not
    uint32_t pad[5];
};
static_assert(sizeof(GridReplaceRecord) == 64, "the record is 64 bytes");

// The scratch, in bytes: the record; per workgroup its count of run starts (low half) and run ends (high half; both at most 2048); per workgroup the
// starts and the ends before it (32 bits each: only made when the runs are written, and then there are at most 2^32 - 1 of them); per workgroup its
// count of changed cubes, which tells the store which workgroups hold a change.
inline uint64_t grid_replace_groups(uint64_t n) { return (n + kGridReplaceGroup - 1u) / kGridReplaceGroup; }
inline size_t grid_replace_counts_offset() { return sizeof(GridReplaceRecord); }
inline size_t grid_replace_offsets_offset(uint64_t n) { return (grid_replace_counts_offset() + 4u * (size_t)grid_replace_groups(n) + 15u) & ~(size_t)15u; }
inline size_t grid_replace_changed_offset(uint64_t n) { return grid_replace_offsets_offset(n) + 8u * (size_t)grid_replace_groups(n); }
inline size_t grid_replace_scratch_bytes(uint64_t n) { return grid_replace_changed_offset(n) + 4u * (size_t)grid_replace_groups(n); }

struct GridReplaceParams {
    uint16_t *grid;           // [n] the layer's cube grid, Z-major; the pool goes on behind it and is neither read nor written
    const uint16_t *fresh;    // [n] the caller's plain block indices, 16-byte aligned
    unsigned long long n;     // sx * sy * sz, not 0; at most 2^31 - 1 workgroups: n <= 2048 x (2^31 - 1)
    uint32_t sx, sy, sz;
    uint32_t index_mask;      // a grid entry's block index = entry & index_mask (kCubeIndexMask when the entries carry tags, else 0xffff)
    const uint32_t *cls;      // the layer's class table, 2 bits per block index, when the entries carry tags; else nullptr: plain indices are stored
    uint32_t cls_words;       // its words: ceil(the layer's block count / 16)
    int32_t lo[3];            // the space's lower corner
    unsigned char *scratch;   // grid_replace_scratch_bytes(n)
    int32_t *boxes;           // [n_runs][6], written by launch_write_grid_replace
    uint32_t n_runs;          // what the record said after the count: no box at or past it is written
};

// Queues the count and the sum of its counts on `stream`: the record's initial value is in the scratch already (copied on the same stream). Afterwards
// the record is final and every workgroup's counts are stored. Nothing is written but scratch.
hipError_t launch_count_grid_replace(const GridReplaceParams &p, hipStream_t stream);
// Queues the scan of the workgroups' counts and the write of boxes[n_runs][6], sorted by a run's first entry. Grid and array must be what the count saw:
// this runs before the store.
hipError_t launch_write_grid_replace(const GridReplaceParams &p, hipStream_t stream);
// Queues the store: grid[i] = fresh[i] | (class + 1) << 14 (never OPEN: launch_open_cubes decides that afterwards), or fresh[i] when the grid carries no
// tags, in the workgroups whose count found a change. An entry whose index stays keeps its bits, which depend on its index and its neighbours' alone.
hipError_t launch_store_grid_replace(const GridReplaceParams &p, hipStream_t stream);
// Queues out[i] = grid[i] & index_mask for i < n (out: 16-byte aligned). Reads the grid only.
hipError_t launch_copy_cube_grid(const uint16_t *grid, unsigned long long n, uint32_t index_mask, uint16_t *out, hipStream_t stream);

}  // namespace aic
