// aic_reproject.h -- the reprojection post-process (aic_reproject.hip) as the host ABI code sees it: the gap-fill chain's geometry, the scratch layout
// and the launch.
//
// When the camera has moved since its resident textures were traced, the reference's incremental renderer forward-reprojects every traced pixel into
// the current view as a depth-tested point sprite (all-is-cubes-gpu/src/raytrace_to_texture.rs:433-540, shaders/rt-copy.wgsl:73-223) and fills the
// holes from a nearest-sampled mip pyramid (shaders/resampling.wgsl:119-176, mip_ping.rs:261-400). What is restated, and the five decisions taken
// where the reference leaves room, are in DESIGN.md "Reprojection".
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aic {

constexpr uint32_t kReprojectMaxLevels = 12;  // raytrace_to_texture.rs:331

// Sizes of one frame's chain (mip_ping.rs:460-481 size_and_mip_levels_for_texture on the frame's own size) and where each part lies in the scratch.
struct ReprojectGeom {
    uint32_t width = 0, height = 0;  // both frames
    uint32_t levels = 0;             // L
    uint32_t mw[kReprojectMaxLevels] = {0}, mh[kReprojectMaxLevels] = {0};  // mip k: T0 >> k
    size_t off[kReprojectMaxLevels] = {0};  // first texel of mip k >= 1 among the stored mips (mip 0 is never stored)
    size_t texels = 0;                      // mips 1 .. L-1
    size_t npix() const { return (size_t)width * height; }
    // the scratch: [npix] keys (u64), [npix] splat image R (f16 x 4), [texels] mips, 4 counters (u64)
    size_t keys_bytes() const { return npix() * 8; }
    size_t r_bytes() const { return npix() * 8; }
    size_t scratch_bytes() const { return npix() ? keys_bytes() + r_bytes() + texels * 8 + 32 : 0; }
};

inline uint32_t reproject_ilog2(uint32_t v) { uint32_t r = 0; while (v >>= 1) r++; return r; }

inline ReprojectGeom reproject_geometry(uint32_t width, uint32_t height) {
    ReprojectGeom g;
    g.width = width;
    g.height = height;
    if (!width || !height) return g;
    const uint32_t m = width < height ? width : height;
    g.levels = reproject_ilog2(m) + 1u;
    if (g.levels > kReprojectMaxLevels) g.levels = kReprojectMaxLevels;
    const uint32_t d = 1u << g.levels;
    const uint32_t t0x = (width + d - 1u) / d * d, t0y = (height + d - 1u) / d * d;  // next_multiple_of(2^L)
    for (uint32_t k = 0; k < g.levels; k++) {
        g.mw[k] = t0x >> k;
        g.mh[k] = t0y >> k;
        if (k >= 1u) {
            g.off[k] = g.texels;
            g.texels += (size_t)g.mw[k] * g.mh[k];
        }
    }
    return g;
}

struct ReprojectParams {
    const uint2 *src_color;  // [height][width] f16 x 4
    const float *src_depth;  // [height][width]; sign bit: a UI pixel
    uint2 *dst_color;
    float *dst_depth;
    unsigned char *scratch;  // geom.scratch_bytes()
    float m[16];             // aic_reproject_desc.reprojection: column-major
    float ipzw[4];           // aic_reproject_desc.inverse_projection_zw
    uint32_t keep_splats;
};
struct ReprojectCounts { unsigned long long n_splats, n_dropped, n_gaps, n_unfilled; };  // the last 32 bytes of the scratch

// Queues the whole post-process on `stream`: clear of keys and counters, splat, resolve, the chain's stages (one launch each: 2 L - 3 of them for
// L >= 2, 19 at L = 11: a 1080p frame), the final store. The counters are complete when the stream is. Returns the first failure of what it queued.
hipError_t launch_reproject(const ReprojectGeom &g, const ReprojectParams &p, hipStream_t stream);
inline const ReprojectCounts *reproject_counts(const ReprojectGeom &g, const unsigned char *scratch) {
    return reinterpret_cast<const ReprojectCounts *>(scratch + g.scratch_bytes() - 32);
}

}  // namespace aic
