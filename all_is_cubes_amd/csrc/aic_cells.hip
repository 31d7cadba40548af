// aic_cells.hip -- the terminal's character cells behind aic_image_cells and aic_render_cells: image_patch_to_character
// (all-is-cubes-desktop/src/terminal/chars.rs:18-173) and ColorMode::convert (terminal/options.rs:78-139), one lane per cell. The rule is
// aic_cells_rule.h (which tests also build for the host); DESIGN.md 4.22 writes every operation out. Built with -ffp-contract=off.
//
// A cell reads its patch of 1x1, 1x2 or 2x4 pixels with plain loads (16 bytes a pixel, 8 for f16), writes three words, and the waves add up the
// branches taken: no LDS, and the only atomics are a wave's sums into the counters.

#include "aic_cells.h"

namespace aic {
namespace {

__global__ void __launch_bounds__(256) cells_kernel(const CellsParams p) {
    const uint64_t n_cells = (uint64_t)p.cols * p.rows;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    CellsCounts n;
    if (t < n_cells) {
        uint32_t words[3];
        cells_cell(p, (uint32_t)(t % p.cols), (uint32_t)(t / p.cols), words, n);
        uint32_t *o = p.out + t * 3u;
        o[0] = words[0]; o[1] = words[1]; o[2] = words[2];
    }
    // a wave's sums: every lane of the workgroup reaches this point; a field holds at most 2 a lane, 128 a wave
#pragma unroll
    for (int w = 0; w < 4; w++) {
        uint32_t v = n.w[w];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        n.w[w] = v;
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (uint32_t s = 0; s < CELLS_COUNTS; s++) {
            const uint32_t v = n.get(s);
            if (v) atomicAdd(&p.counts[s], v);
        }
    }
}

}  // namespace

hipError_t launch_cells(const CellsParams &p, hipStream_t stream) {
    const uint64_t n_cells = (uint64_t)p.cols * p.rows;
    if (!n_cells) return hipSuccess;
    hipLaunchKernelGGL(cells_kernel, dim3((uint32_t)((n_cells + 255u) / 256u)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace aic
