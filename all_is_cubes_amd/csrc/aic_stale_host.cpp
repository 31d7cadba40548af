// aic_stale_host.cpp -- aic_stale_rects of the stale-pixel picker (include/aic_hip.h under aic_pick_stale), which needs no context: boxes
// of changed cubes to screen rectangles, in f64 and in the order the header writes out (-ffp-contract=off: tests/stale_ref.py gives the same bits).
// aic_pick_stale itself, the context's side of aic_stale.hip, is one of aic_split_ops.cpp's operations.
#include <cmath>
#include <cstring>
#include <limits>

#include "../../include/aic_hip.h"

namespace {

// floor(v) clamped to [0, n], for v that may be infinite (never NaN)
uint16_t clamp_cell(double v, uint32_t n) { return v <= 0.0 ? (uint16_t)0 : (v >= (double)n ? (uint16_t)n : (uint16_t)v); }

void stale_rect_of(const double m[16], uint32_t width, uint32_t height, const int32_t box[6], int32_t expand, aic_stale_rect *out) {
    std::memset(out, 0, sizeof(*out));
    for (int a = 0; a < 3; a++)
        if (box[3 + a] <= box[a]) return;
    double e[2][3];
    for (int a = 0; a < 3; a++) {
        e[0][a] = (double)((int64_t)box[a] - (int64_t)expand);
        e[1][a] = (double)((int64_t)box[3 + a] + (int64_t)expand);
    }
    const double inf = std::numeric_limits<double>::infinity();
    double ax = inf, bx = -inf, ay = inf, by = -inf, az = inf;
    bool whole = false;
    for (int k = 0; k < 8; k++) {
        const double x = e[k & 1][0], y = e[(k >> 1) & 1][1], z = e[(k >> 2) & 1][2];
        double clip[4];
        for (int r = 0; r < 4; r++) clip[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r];
        if (!(clip[3] > 0.0) || !std::isfinite(clip[0]) || !std::isfinite(clip[1]) || !std::isfinite(clip[2]) || !std::isfinite(clip[3])) { whole = true; break; }
        const double nx = clip[0] / clip[3], ny = clip[1] / clip[3], nz = clip[2] / clip[3];
        ax = nx < ax ? nx : ax; bx = nx > bx ? nx : bx;
        ay = ny < ay ? ny : ay; by = ny > by ? ny : by;
        az = nz < az ? nz : az;
    }
    if (whole) {
        out->x1 = (uint16_t)width;
        out->y1 = (uint16_t)height;
        out->dmin = -std::numeric_limits<float>::infinity();
        return;
    }
    const double W = (double)width, H = (double)height;
    const uint16_t x0 = clamp_cell(std::floor((ax + 1.0) / 2.0 * W) - 1.0, width), x1 = clamp_cell(std::floor((bx + 1.0) / 2.0 * W) + 2.0, width);
    const uint16_t y0 = clamp_cell(std::floor((1.0 - by) / 2.0 * H) - 1.0, height), y1 = clamp_cell(std::floor((1.0 - ay) / 2.0 * H) + 2.0, height);
    if (x0 >= x1 || y0 >= y1) return;
    out->x0 = x0; out->y0 = y0; out->x1 = x1; out->y1 = y1;
    const double lowered = az - 1.0 / 16777216.0;
    float d = (float)lowered;  // to nearest; then down if that went up
    if ((double)d > lowered) d = std::nextafterf(d, -std::numeric_limits<float>::infinity());
    out->dmin = d;
}

}  // namespace

extern "C" int aic_stale_rects(const double view_projection[16], uint32_t width, uint32_t height, uint32_t n_boxes, const int32_t *boxes, int32_t expand,
                               aic_stale_rect *out) {
    if (!view_projection || (n_boxes && (!boxes || !out)) || expand < 0 || width > 65535u || height > 65535u) return AIC_ERR_INVALID;
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(view_projection[i])) return AIC_ERR_INVALID;
    for (uint32_t i = 0; i < n_boxes; i++) stale_rect_of(view_projection, width, height, boxes + (size_t)i * 6, expand, out + i);
    return AIC_OK;
}
