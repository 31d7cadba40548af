// Test shim: the cells kernel's rule (all_is_cubes_amd/csrc/aic_cells_rule.h, the very source the HIP kernel inlines) compiled for the HOST behind a C
// entry point, so that tests/test_cells_cpu.py can hold it to the restatement cell for cell without a GPU. Built by the test with
// g++ -ffp-contract=off (the kernel's own floating-point contract).
#include <math.h>
#include <stdint.h>

namespace aic {
// aic_encode.h's device helpers, which the rule takes from there in the kernel: the same one-liners for the host
static inline float ps_clamped(float v) { return v > 0.f ? v : 0.f; }
static inline float ps_mul(float a, float b) { return fmaxf(a * b, 0.0f); }
static inline float luminance(float r, float g, float b) { return g * 0.7152f + (r * 0.2126f + b * 0.0722f); }
}  // namespace aic

#include "aic_cells_rule.h"

// the exact sRGB8 encoder's bucket table from thr[0..255]; 1: built
extern "C" int shim_srgb_buckets(const float *thr, uint32_t *table /* [aic::kSrgbBucketWords] */) { return aic::srgb8_bucket_build(thr, table) ? 1 : 0; }
extern "C" uint32_t shim_srgb_bucket_words(void) { return aic::kSrgbBucketWords; }

// every cell of the grid, as the kernel's lanes make them; counts[15] are added to
extern "C" void shim_cells(const void *image, const aic_pixel_aux *aux, const uint32_t *srgb_buckets, uint32_t cols, uint32_t rows, uint32_t width,
                           int32_t characters, int32_t colors, int32_t f16, int32_t postprocessed, float exposure, int32_t tone_mapping,
                           float maximum_intensity, uint32_t *out /* [rows][cols][3] */, uint32_t *counts) {
    aic::CellsParams p = {};
    p.image = image; p.aux = aux; p.out = out; p.counts = counts; p.srgb_buckets = srgb_buckets;
    p.cols = cols; p.rows = rows; p.width = width;
    p.characters = characters; p.colors = colors; p.f16 = f16; p.postprocessed = postprocessed;
    p.exposure = exposure; p.tone_mapping = tone_mapping; p.maximum_intensity = maximum_intensity;
    for (uint32_t cy = 0; cy < rows; cy++)
        for (uint32_t cx = 0; cx < cols; cx++) {
            aic::CellsCounts n;
            aic::cells_cell(p, cx, cy, out + ((size_t)cy * cols + cx) * 3u, n);
            for (uint32_t s = 0; s < aic::CELLS_COUNTS; s++) counts[s] += n.get(s);
        }
}
