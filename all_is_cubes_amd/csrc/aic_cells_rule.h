// aic_cells_rule.h -- one character cell of a terminal frame: image_patch_to_character (all-is-cubes-desktop/src/terminal/chars.rs:18-173) with
// ColorMode::convert (terminal/options.rs:78-139) on pixels made by camera.post_process_color (terminal.rs:355-365). DESIGN.md 4.22 writes every operation
// out; tests/cells_ref.py is that text in NumPy. Every f32 product and sum below is rounded once, in this order: build with -ffp-contract=off.
//
// Plain C++ that the cells kernel (aic_cells.hip) inlines, one lane per cell, and that also compiles for the host: tests/native/cells_rule_shim.cpp
// builds this very source with g++ and tests/test_cells_cpu.py holds it to the restatement without a GPU (as tests/native/lightmath_shim.cpp does for the
// light interpolation). It takes Rgb::luminance, the PositiveSign product and clamp and the exact sRGB8 encoder from aic_encode.h (namespace aic:
// luminance, ps_mul, ps_clamped, srgb8_bucket_channel); that header's first three are device code, so a host build supplies them before including this.
//
// post_process_color's tone map is written out again here (ten lines, from the trace kernels' FINISH, aic_trace.hip): there it is part of the kernel's
// body, not a function, and lifting it into a header would have meant editing the trace kernels' source for a kernel that has nothing to do with them.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/aic_hip.h"
#include "aic_encode.h"

#if defined(__HIPCC__)
#define AIC_CELLS_FN __device__ __forceinline__
#define AIC_CELLS_MEMBER __device__ __forceinline__
#else
#define AIC_CELLS_FN static inline
#define AIC_CELLS_MEMBER inline
#endif

namespace aic {

// the slots of CellsParams::counts, in aic_cells_info's order from n_full on
enum CellsCount : uint32_t {
    CELLS_FULL, CELLS_UPPER, CELLS_LOWER, CELLS_TEXT, CELLS_SPACE, CELLS_SHADE, CELLS_RISING, CELLS_FALLING, CELLS_EQUAL, CELLS_UNEQUAL, CELLS_NAMES,
    CELLS_BRAILLE, CELLS_GRAY, CELLS_CUBE, CELLS_RGB, CELLS_COUNTS
};

struct CellsParams {
    const void *image;            // [height][width] of four f32, or (f16) of four halves
    const aic_pixel_aux *aux;     // [height][width], or nullptr
    uint32_t *out;                // [rows][cols][3]
    uint32_t *counts;             // [CELLS_COUNTS], zero before the launch
    const uint32_t *srgb_buckets; // the exact sRGB8 encoder's bucket table (aic_encode.h)
    uint32_t cols, rows;          // the grid (already raised to 1 x 1)
    uint32_t width;               // pixels in an image row: cols x rays per character
    int32_t characters, colors;
    int32_t f16, postprocessed;
    float exposure;
    int32_t tone_mapping;
    float maximum_intensity;
};

// a lane's branch counts, four 8-bit fields a word: a cell adds at most 2 to a field, a wave of 64 at most 128
struct CellsCounts {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    AIC_CELLS_MEMBER void add(uint32_t slot) { w[slot >> 2] += 1u << ((slot & 3u) * 8u); }
    AIC_CELLS_MEMBER uint32_t get(uint32_t slot) const { return (w[slot >> 2] >> ((slot & 3u) * 8u)) & 0xffu; }
};

namespace cells {

struct Rgb3 { float r, g, b; };

// Camera::post_process_color (camera_struct.rs:376-382): rgb * exposure, then ToneMappingOperator::apply (graphics_options.rs:352-368)
AIC_CELLS_FN Rgb3 post_process(const CellsParams &p, Rgb3 c) {
    float r = ps_mul(c.r, p.exposure), g = ps_mul(c.g, p.exposure), bl = ps_mul(c.b, p.exposure);
    const float m = p.maximum_intensity;
    if (isfinite(m)) {
        if (p.tone_mapping == 0) {
            r = r < 0.f ? 0.f : (r > m ? m : r);
            g = g < 0.f ? 0.f : (g > m ? m : g);
            bl = bl < 0.f ? 0.f : (bl > m ? m : bl);
        } else {
            const float scale = ps_clamped(1.0f / (1.0f + luminance(r, g, bl) / m));
            r = ps_mul(r, scale); g = ps_mul(g, scale); bl = ps_mul(bl, scale);
        }
    }
    return Rgb3{r, g, bl};
}

// an IEEE half's value, exactly (the same integer steps on the host and on the device)
AIC_CELLS_FN float half_bits_to_float(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t bits;
    if (e == 0x1fu) bits = 0x7f800000u | (m << 13);
    else if (e != 0u) bits = ((e + 112u) << 23) | (m << 13);
    else bits = srgb8_float_bits((float)m * 5.9604644775390625e-08f);  // a subnormal: m * 2^-24
    bits |= sign;
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

// the colour of pixel (x, y) as the patch rule sees it: Some(camera.post_process_color(Rgba::from(ColorBuf))) (terminal.rs:355-365)
AIC_CELLS_FN Rgb3 pixel(const CellsParams &p, uint32_t x, uint32_t y) {
    const size_t i = (size_t)y * p.width + x;
    Rgb3 c;
    if (p.f16) {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(p.image) + 2u * i;
        const uint32_t lo = t[0], hi = t[1];
        c = Rgb3{half_bits_to_float(lo & 0xffffu), half_bits_to_float(lo >> 16), half_bits_to_float(hi & 0xffffu)};
    } else {
        const float *t = reinterpret_cast<const float *>(p.image) + 4u * i;
        c = Rgb3{t[0], t[1], t[2]};
    }
    return p.postprocessed ? c : post_process(p, c);
}

// the text of pixel (x, y): the rule HipRtRenderer::draw_text applies to a first-hit record (text.rs:52-128)
AIC_CELLS_FN uint32_t pixel_text(const CellsParams &p, uint32_t x, uint32_t y) {
    if (!p.aux) return (uint32_t)' ';
    const aic_pixel_aux &a = p.aux[(size_t)y * p.width + x];
    const int32_t hit = a.hit;
    const uint32_t steps = a.cubes_traced;
    if (hit == 1) return AIC_CELL_GLYPH_BLOCK | ((a.layer & 0x7fffu) << 16) | ((uint32_t)a.block_index & 0xffffu);
    return steps > 1000u ? (uint32_t)'X' : (steps > 0u ? (uint32_t)' ' : (uint32_t)'.');
}

// srgb_to_216 (options.rs:90-99)
AIC_CELLS_FN uint32_t cube_level(uint32_t v) { return (v >= 48u) + (v >= 115u) + (v >= 155u) + (v >= 195u) + (v >= 235u); }

// ColorMode::convert(Some(rgb)) (options.rs:78-139) as a cell's colour word; 0 for ColorMode::None
AIC_CELLS_FN uint32_t convert(const CellsParams &p, Rgb3 c, CellsCounts &n) {
    if (p.colors == AIC_CELLS_COLOR_NONE) return 0u;
    if (p.colors == AIC_CELLS_COLOR_256) {
        const float lum = luminance(c.r, c.g, c.b);
        const float saturation = (fabsf(c.r - lum) + fabsf(c.g - lum)) + fabsf(c.b - lum);  // Vector3D::dot with (1, 1, 1)
        uint32_t ansi;
        if (saturation < 0.1f) {
            n.add(CELLS_GRAY);
            const uint32_t s = srgb8_bucket_channel(lum, p.srgb_buckets);
            const uint32_t gray = (uint32_t)roundf((float)s / 255.f * 25.f);  // zero to 25
            ansi = gray == 0u ? 16u : (gray == 25u ? 231u : gray + 231u);
        } else {
            n.add(CELLS_CUBE);
            const uint32_t R = srgb8_bucket_channel(c.r, p.srgb_buckets), G = srgb8_bucket_channel(c.g, p.srgb_buckets), B = srgb8_bucket_channel(c.b, p.srgb_buckets);
            ansi = 16u + (cube_level(R) * 6u + cube_level(G)) * 6u + cube_level(B);
        }
        return (AIC_CELL_COLOR_ANSI << 24) | ansi;
    }
    n.add(CELLS_RGB);
    const uint32_t R = srgb8_bucket_channel(c.r, p.srgb_buckets), G = srgb8_bucket_channel(c.g, p.srgb_buckets), B = srgb8_bucket_channel(c.b, p.srgb_buckets);
    return (AIC_CELL_COLOR_RGB << 24) | (R << 16) | (G << 8) | B;
}

// pick_01_from_array's index (chars.rs:175-182): `(position * N as f32) as usize` truncates and saturates (NaN and negatives give 0), then the clamp
AIC_CELLS_FN uint32_t pick_index(float position, uint32_t n) {
    const float v = position * (float)n;
    if (!(v > 0.f)) return 0u;
    return v >= (float)n ? n - 1u : (uint32_t)v;
}
AIC_CELLS_FN uint32_t shade_glyph(float position) {  // " ░▒▓█"
    const uint32_t i = pick_index(position, 5u);
    return i == 0u ? 0x20u : (i == 4u ? 0x2588u : 0x2590u + i);
}

}  // namespace cells

// Cell (cx, cy) of the grid: its three words into out[0..2], the branches it took into n.
AIC_CELLS_FN void cells_cell(const CellsParams &p, uint32_t cx, uint32_t cy, uint32_t out[3], CellsCounts &n) {
    using namespace cells;
    constexpr uint32_t kReset = AIC_CELL_COLOR_RESET << 24, kBlack = AIC_CELL_COLOR_BLACK << 24;
    uint32_t glyph, fg, bg;
    const bool halves = p.characters == AIC_CELLS_SPLIT || p.characters == AIC_CELLS_SHAPES;
    if (halves && p.colors == AIC_CELLS_COLOR_NONE) {
        // "black and white" graphic characters
        const Rgb3 c1 = pixel(p, cx, cy * 2u), c2 = pixel(p, cx, cy * 2u + 1u);
        const float lum1 = luminance(c1.r, c1.g, c1.b), lum2 = luminance(c2.r, c2.g, c2.b);
        if (p.characters == AIC_CELLS_SPLIT) {
            // checkerboard dithering
            const float threshold1 = (cx & 1u) ? 0.7f : 0.5f, threshold2 = (cx & 1u) ? 0.5f : 0.7f;
            const bool up = lum1 > threshold1, down = lum2 > threshold2;
            if (up && down) { glyph = 0x2588u; n.add(CELLS_FULL); }
            else if (up) { glyph = 0x2580u; n.add(CELLS_UPPER); }
            else if (down) { glyph = 0x2584u; n.add(CELLS_LOWER); }
            else if (lum2 > 0.2f) { glyph = pixel_text(p, cx, cy * 2u); n.add(CELLS_TEXT); }
            else { glyph = 0x20u; n.add(CELLS_SPACE); }
        } else {
            float avg = (float)(((double)lum1 + (double)lum2) / 2.0);  // f32::midpoint
            avg = avg < 0.f ? 0.f : (avg > 1.f ? 1.f : avg);           // clamp(0.0, 1.0): NaN stays
            if (fabsf(lum1 - lum2) < 0.05f) { glyph = shade_glyph(avg); n.add(CELLS_SHADE); }
            else {
                const uint32_t i = pick_index(avg, 9u);
                if (lum1 < lum2) { glyph = i == 0u ? 0x20u : 0x2580u + i; n.add(CELLS_RISING); }  // " ▁▂▃▄▅▆▇█"
                else { glyph = i == 0u ? 0x20u : 0x2500u | (uint32_t)((0x889B9B8080989894ull >> ((i - 1u) * 8u)) & 0xffu); n.add(CELLS_FALLING); }  // " ▔▘▘▀▀▛▛█"
            }
        }
        fg = bg = 0u;
    } else if (halves) {
        // an upper and a lower half; compare the two CONVERTED colours
        const uint32_t color1 = convert(p, pixel(p, cx, cy * 2u), n), color2 = convert(p, pixel(p, cx, cy * 2u + 1u), n);
        if (color1 == color2) { glyph = 0x20u; fg = kBlack; bg = color1; n.add(CELLS_EQUAL); }
        else { glyph = 0x2584u; fg = color2; bg = color1; n.add(CELLS_UNEQUAL); }
    } else if (p.characters == AIC_CELLS_NAMES) {
        glyph = pixel_text(p, cx, cy);
        const uint32_t color = convert(p, pixel(p, cx, cy), n);
        fg = color ? kBlack : kReset;
        bg = color ? color : kReset;
        n.add(CELLS_NAMES);
    } else if (p.characters == AIC_CELLS_SHADES) {
        const Rgb3 c = pixel(p, cx, cy);
        glyph = shade_glyph(luminance(c.r, c.g, c.b));
        fg = bg = kReset;
        n.add(CELLS_SHADE);
    } else {
        // Braille: dots 1 4 / 2 5 / 3 6 / 7 8, bit k of the index is dot k + 1
        const float base = (float)cx * 284.1834f + (float)cy * 100.2384f;  // char_pos.to_f32().dot(...)
        uint32_t index = 0u;
        Rgb3 sum{0.f, 0.f, 0.f};
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < 8u; k++) {  // in the order of the dot numbers: one, two, three, four, five, six, seven, eight
            const uint32_t dx = ((k >= 3u && k <= 5u) || k == 7u) ? 1u : 0u;
            const uint32_t dy = k < 3u ? k : (k < 6u ? k - 3u : 3u);
            const Rgb3 c = pixel(p, cx * 2u + dx, cy * 4u + dy);
            const float threshold = (fmodf((float)k + base, 8.0f) + 0.5f) / 8.0f;  // rem_euclid of a sum that is never negative
            index |= (luminance(c.r, c.g, c.b) > threshold ? 1u : 0u) << k;
            if (k == 0u) sum = c;
            else { sum.r += c.r; sum.g += c.g; sum.b += c.b; }
        }
        const float k_hue = ps_clamped(0.75f / fmaxf(luminance(sum.r, sum.g, sum.b), 0.1f));
        const uint32_t color = convert(p, Rgb3{ps_mul(sum.r, k_hue), ps_mul(sum.g, k_hue), ps_mul(sum.b, k_hue)}, n);
        glyph = 0x2800u + index;
        fg = color ? color : kReset;
        bg = color ? kBlack : kReset;
        n.add(CELLS_BRAILLE);
    }
    out[0] = glyph; out[1] = fg; out[2] = bg;
}

}  // namespace aic
