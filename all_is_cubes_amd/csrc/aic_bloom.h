// aic_bloom.h -- the bloom post-process (aic_bloom.hip) as the host ABI code sees it: the chain's geometry and the launch.
//
// The reference's GPU renderer blooms every frame whose GraphicsOptions ask for it, raytraced frames included
// (all-is-cubes-gpu/src/raytrace_to_texture.rs:644-661 hands the raytracer's ColorBuf to the post-process): a "dual filter" mip chain
// (bloom.rs:41-60, mip_ping.rs:301-420, shaders/resampling.wgsl) mixed into the scene before tone mapping (shaders/postprocess.wgsl:140-158).
// What is restated, and the three decisions taken where the reference leaves room, are in DESIGN.md "Bloom".
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aic {

constexpr uint32_t kBloomMaxLevels = 6;        // bloom.rs:57
constexpr uint32_t kBloomRepetitions = 3;      // bloom.rs:58

// Sizes of one frame's chain (mip_ping.rs:460-481 size_and_mip_levels_for_texture, on the half-size request of bloom.rs:50-53).
struct BloomGeom {
    uint32_t width = 0, height = 0;  // the frame: the scene texture S
    uint32_t levels = 0;             // L
    uint32_t mw[kBloomMaxLevels] = {0}, mh[kBloomMaxLevels] = {0};  // mip k: T0 >> k
    uint32_t off[kBloomMaxLevels] = {0};                            // first texel of mip k in the chain buffer
    uint32_t texels = 0;             // the whole chain
};

inline uint32_t bloom_ilog2(uint32_t v) { uint32_t r = 0; while (v >>= 1) r++; return r; }

inline BloomGeom bloom_geometry(uint32_t width, uint32_t height) {
    BloomGeom g;
    g.width = width;
    g.height = height;
    const uint32_t rx = (width + 1u) / 2u, ry = (height + 1u) / 2u;  // div_ceil(2)
    const uint32_t m = rx < ry ? rx : ry;
    g.levels = m ? bloom_ilog2(m) + 1u : 1u;
    if (g.levels > kBloomMaxLevels) g.levels = kBloomMaxLevels;
    const uint32_t d = 1u << g.levels;
    const uint32_t t0x = (rx + d - 1u) / d * d, t0y = (ry + d - 1u) / d * d;  // next_multiple_of(2^L)
    for (uint32_t k = 0; k < g.levels; k++) {
        g.mw[k] = t0x >> k;
        g.mh[k] = t0y >> k;
        g.off[k] = g.texels;
        g.texels += g.mw[k] * g.mh[k];
    }
    return g;
}

struct BloomParams {
    const float4 *colorbuf;  // [height][width] ColorBuf l0, l1, l2, t: the trace's AIC_FRAME_OUT_COLORBUF output
    uint2 *mips;             // [geom.texels] f16 x 4 per texel
    uint32_t *out;           // [height][width] RGBA8
    float exposure;          // the world camera's
    float intensity;         // GraphicsOptions::bloom_intensity
    int32_t tone_mapping;
    float maximum_intensity;
    const float *srgb_thr;   // the context's 256 sRGB8 thresholds: srgb_thr[k] = smallest linear value whose sRGB8 encoding is >= k
};

// Queues the whole post-process on `stream`: the chain (downsample 0 from the ColorBuf, then the stages of mip_ping.rs:301-420) and the composite into
// p.out. Launches: one per stage, 6 L - 5 of them (31 at L = 6: a 1080p or 4K frame), then the composite.
void launch_bloom(const BloomGeom &g, const BloomParams &p, hipStream_t stream);
// Every stage of the chain but the first: with mip 0 of `mips` already queued as downsample 0 of the scene -- from whatever holds it --, queues
// downsample 1 .. L-1, upsample L-2 .. 0 and the two further repetitions, which read mips only (mip_ping.rs:301-420). 6 L - 6 launches.
void launch_bloom_stages(const BloomGeom &g, uint2 *mips, hipStream_t stream);

// Presentation of a resident Split frame (aic_present_split): the reference's per-frame draw of its resident textures, raytrace_to_texture.rs:546-568 with
// shaders/rt-copy.wgsl:41-71 (the linear ClampToEdge stretch into the scene texture, alpha 1), then the same chain and postprocess.wgsl:140-158, 251-276.
// The info text of a presentation (aic_present_split_text; postprocess.wgsl:160-246): a grid of character codes and the context's
// resident font atlas, composited over the tone-mapped scene. codes == nullptr: no text, and the composite is the one without.
struct PresentText {
    const uint8_t *codes = nullptr;   // [rows][cols], device memory; 0 reads as 0x20
    const uint32_t *atlas = nullptr;  // [16 * cell_h][16 * cell_w] RGBA8, premultiplied alpha, device memory
    float scale[2] = {0.f, 0.f}, origin[2] = {0.f, 0.f};
    uint32_t cols = 0, rows = 0;
    uint32_t cell_w = 0, cell_h = 0, margin = 0;
    // the output pixels [x0, x1) x [y0, y1) outside which no cell can contribute anything but zeros: the lanes there skip the four lookups
    uint32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
};

struct PresentParams {
    const uint2 *src;               // the frame's colour plane [src_height][src_width] f16 x 4 (its depth plane is not read)
    uint32_t src_width, src_height;
    uint2 *scene;                     // S, [geom.height][geom.width]: written and read only when bloomed AND the sizes differ
    uint2 *mips;                      // [geom.texels]: only when bloomed
    void *out;                        // [geom.height][geom.width] RGBA8, or four f16 with out_f16
    float intensity;                  // > 0: bloomed
    int32_t tone_mapping;
    float maximum_intensity;
    const float *srgb_thr;
    bool out_f16;                     // AIC_PRESENT_OUT_F16
    PresentText text;                 // codes != nullptr: the composite's TEXT variant lays the info text over the tone-mapped scene
};
// Queues the presentation on `stream`; `g` = bloom_geometry of the OUTPUT size, at most 2^31 pixels (the kernels' texel indices are 32-bit). Launches:
// the composite alone at intensity 0; else the chain's 6 L - 5 stages before it, and the stretch into S before those when the sizes differ. The text
// adds no launch: it is a variant of the composite.
void launch_present(const BloomGeom &g, const PresentParams &p, hipStream_t stream);
// Queues S alone, stored into p.scene whatever the sizes: the stretch when they differ, the source texels (saturated, alpha 1) when they do not. What a
// pass that draws into the scene before the chain runs (aic_present_lines.h) starts from; launch_present then takes p.scene as a frame of the output's size.
void launch_present_scene(const BloomGeom &g, const PresentParams &p, hipStream_t stream);

// The RGB-D export of a resident Split frame (aic_export_split; all-is-cubes-gpu/src/rerun_image.rs:62-225, shaders/rerun-copy.wgsl): the
// presentation's scene texel at the logged size encoded as sRGB8, and the nearest depth texel unprojected to a view-space distance, 0 where there is
// no surface.
// The statistics are kept in kExportSlots slots, each a 128-byte line of its own, and a wave adds to the slot its index selects: atomics of every wave on
// one address ran one after the other and took 1.1 ms of a 1080p export that otherwise takes 0.01 (profiles/export_split.txt). The host sums the slots.
constexpr uint32_t kExportSlots = 64;
struct alignas(128) ExportCounts { uint32_t n_surface, min_bits, max_bits, pad[29]; };  // min_bits, max_bits: the bit patterns of the least and greatest exported depth
struct ExportParams {
    const uint2 *src;               // the whole Split frame: [src_height][src_width] f16 x 4, then [src_height][src_width] f32 depth
    uint32_t src_width, src_height;
    uint32_t out_width, out_height;  // at most 2^31 pixels
    uint32_t *color;                // [out_height][out_width] RGBA8, or nullptr: not written
    float *depth;                   // [out_height][out_width] f32, or nullptr: not written
    float ipzw[4];                  // aic_export_desc.inverse_projection_zw
    const float *srgb_thr;
    ExportCounts *counts;           // [kExportSlots], device memory at a 128-byte boundary; cleared here, complete when the stream is
};
// Queues the clear of the counters and the one kernel on `stream`: a lane per output pixel. Returns the first failure of what it queued.
hipError_t launch_export(const ExportParams &p, hipStream_t stream);

}  // namespace aic
