// aic_stale_host.cpp -- aic_stale_rects of the stale-pixel picker (include/aic_hip.h under aic_pick_stale), which needs no context: boxes
// of changed cubes to screen rectangles, in f64 and in the order the header writes out (-ffp-contract=off: tests/stale_ref.py gives the same bits).
// aic_pick_stale itself, the context's side of aic_stale.hip, is one of aic_split_ops.cpp's operations.
#include <cmath>
#include <cstring>

#include "../../include/aic_hip.h"
#include "aic_stale_rect_math.h"

namespace {

// one box through the shared arithmetic (aic_stale_rect_math.h); aic_stale_rect has no dmax
void stale_rect_of(const double m[16], uint32_t width, uint32_t height, const int32_t box[6], int32_t expand, aic_stale_rect *out) {
    std::memset(out, 0, sizeof(*out));
    const aic::StaleBounds b = aic::stale_bounds_of(m, width, height, box[0], box[1], box[2], box[3], box[4], box[5], expand);
    out->x0 = b.x0; out->y0 = b.y0; out->x1 = b.x1; out->y1 = b.y1;
    out->dmin = b.dmin;
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
