// aic_present_lines.h -- the line pass of a presentation (aic_present_lines.hip; aic_present_split_lines) as the host ABI code sees it.
//
// The reference draws its line list (the cursor's wireframe, debug lines) into the scene texture after the traced frame and before bloom and tone
// mapping: EverythingRenderer::draw_frame_linear (all-is-cubes-gpu/src/everything.rs:616-658), lines_vertex / lines_fragment
// (shaders/blocks-and-lines.wgsl:902-919), a LineList pipeline with CompareFunction::Less, depth write and no blend (pipelines.rs:453-487), tested
// against the depth the frame copy wrote (shaders/rt-copy.wgsl:55-71). WebGPU leaves line rasterisation to the implementation: the rule is DESIGN's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aic {

constexpr uint32_t kLineVertexWords = 7;  // aic_line_vertex: position[3], color[4]

struct LinesCounts {  // aic_lines_info, as the kernels count it
    unsigned long long n_clipped_away, n_fragments, n_passed, n_pixels;
};

// Where the parts of the context's line scratch start: the key image, the stored scene S, the counters, then the staged vertices of a host list.
struct LinesLayout {
    size_t keys = 0, scene = 0, counts = 0, vertices = 0, bytes = 0;
};
inline LinesLayout lines_layout(uint32_t width, uint32_t height, uint32_t n_staged_lines) {
    LinesLayout l;
    const size_t npix = (size_t)width * height;
    l.scene = npix * 8;
    l.counts = l.scene + npix * 8;
    l.vertices = l.counts + sizeof(LinesCounts);
    l.bytes = l.vertices + (size_t)n_staged_lines * 2 * kLineVertexWords * 4;
    return l;
}

struct LinesParams {
    const float *vertices;      // [2 n_lines][7] on the device, 4-byte aligned
    uint32_t n_lines;
    float m[16];                // view_projection, column-major
    const uint32_t *depth;      // the Split frame's depth plane [src_height][src_width], f32 bit patterns
    uint32_t src_width, src_height;
    uint32_t width, height;     // the output: S, the keys
    unsigned long long *keys;   // [height][width]; all ones wherever no line call is between its draw and its resolve
    uint2 *scene;               // S on entry, S' on return
    LinesCounts *counts;
    bool clear_keys;            // the keys are not known to be all ones: clear them first
    bool reset_keys;            // the resolve puts every key it owns back to all ones (else the next call clears: clear_keys)
};
// Queues the pass on `stream`: the counters' (and on request the keys') clear, the draw and the resolve. At most AIC_LINES_MAX lines.
hipError_t launch_present_lines(const LinesParams &p, hipStream_t stream);

}  // namespace aic
