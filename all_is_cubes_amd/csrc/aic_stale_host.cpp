// aic_stale_host.cpp -- the host side of the stale-pixel picker (include/aic_hip.h under aic_pick_stale): aic_stale_rects, which needs no
// context -- boxes of changed cubes to screen rectangles, in f64 and in the order the header writes out (-ffp-contract=off: tests/stale_ref.py gives the
// same bits) --, and aic_pick_stale, the context's side of aic_stale.hip, written to the pattern of aic_split_ops.cpp's operations: check the arguments,
// slot 0 free, size the context's scratch, fill the launcher's parameters, then ev0, the launches, ev1, the record's copy back and one synchronise.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "aic_ctx.h"
#include "aic_stale.h"

static_assert(sizeof(aic_stale_rect) == sizeof(StaleRect) && sizeof(aic_stale_rect) == 16, "the device reads aic_stale_rect as it is");

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

extern "C" int aic_pick_stale(aic_ctx *c, const aic_stale_desc *d, const void *src, const uint32_t *order, uint32_t *pixels_out, aic_stale_info *info) {
    if (!c || !d || !info) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: bad argument");
    std::memset(info, 0, sizeof(*info));
    if (d->width > 65535u || d->height > 65535u) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: frame dimensions above 65535 are not supported");
    if (d->flags & ~AIC_STALE_DEPTH_TEST) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: unknown flag bits");
    if (d->n > 2048u * 65535u) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: more than 2048 x 65535 picks");
    if (d->n && !pixels_out) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: no list to write the picks to");
    if (((uintptr_t)pixels_out & 3u) || ((uintptr_t)order & 3u)) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: a list starts at a 4-byte boundary");
    if ((uintptr_t)src & 7u) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: a Split frame starts at an 8-byte boundary");
    const uint64_t count = (uint64_t)d->width * d->height;
    if (d->n && !count) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: an empty frame has no pixel to pick");
    if (d->n_rects > AIC_STALE_MAX_RECTS) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: more than AIC_STALE_MAX_RECTS rectangles");
    if (d->n_rects && !d->rects) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: no rectangles");
    std::vector<aic_stale_rect> rects;  // the ones that hold a pixel
    for (uint32_t i = 0; i < d->n_rects; i++) {
        const aic_stale_rect &r = d->rects[i];
        if (r.x0 > r.x1 || r.y0 > r.y1 || r.x1 > d->width || r.y1 > d->height) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: a rectangle is inside out or leaves the frame");
        if (std::isnan(r.dmin)) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: a rectangle's dmin is NaN");
        if (r.x0 < r.x1 && r.y0 < r.y1) rects.push_back(r);
    }
    const bool depth_test = (d->flags & AIC_STALE_DEPTH_TEST) != 0;
    const uint32_t n_rects = (uint32_t)rects.size();
    // whether anything is looked at (no rectangle that holds a pixel: the kernels would count nothing, the answer is known)
    const bool look = d->n && n_rects && d->max_stale;
    if (d->n && d->n_rects && d->max_stale && depth_test && !src) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: no frame to test the depths of");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->slots[0].busy) return fail(c, AIC_ERR_INVALID, "aic_pick_stale: a submitted frame still occupies slot 0 (aic_render_wait it first)");
    if (!d->n) return AIC_OK;  // (and so count == 0)
    hipError_t e;
    if (look && (e = c->stale_scratch.ensure(stale_scratch_bytes(count, n_rects))) != hipSuccess) return hip_fail(c, "alloc stale scratch", e);
    aic_ctx::FrameSlot &fs = c->slots[0];
    StaleParams sp;
    sp.color = look && depth_test ? (const uint2 *)src : nullptr;
    sp.depth = look && depth_test ? (const float *)((const unsigned char *)src + count * 8u) : nullptr;
    sp.order = order;
    sp.out = pixels_out;
    sp.scratch = look ? c->stale_scratch.p : nullptr;
    sp.rects = look ? (const StaleRect *)(c->stale_scratch.p + stale_rects_offset(count)) : nullptr;
    sp.width = d->width;
    sp.count = (uint32_t)count;  // at most 65535^2
    sp.n = d->n;
    sp.max_stale = look ? d->max_stale : 0u;
    sp.n_rects = look ? n_rects : 0u;
    sp.depth_test = depth_test ? 1u : 0u;
    sp.skip_stale = d->skip_stale;
    sp.cursor = d->cursor;
    if (look) HIP_TRY(c, hipMemcpyAsync(c->stale_scratch.p + stale_rects_offset(count), rects.data(), sizeof(aic_stale_rect) * (size_t)n_rects, hipMemcpyHostToDevice, fs.stream));
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));
    if ((e = launch_pick_stale(sp, fs.stream)) != hipSuccess) return hip_fail(c, "launch pick stale", e);
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    StaleRecord rec = {};
    if (look) {
        HIP_TRY(c, hipMemcpyAsync(&rec, c->stale_scratch.p, sizeof(rec), hipMemcpyDeviceToHost, fs.stream));
    } else {  // nothing was looked at: the whole list is the picker's
        rec.n_from_order = d->n;
        rec.next_cursor = d->cursor + d->n;
    }
    HIP_TRY(c, hipStreamSynchronize(fs.stream));  // (`rects` goes out of scope)
    info->n_stale = rec.n_stale;
    info->next_cursor = rec.next_cursor;
    info->n_from_stale = rec.n_from_stale;
    info->n_from_order = rec.n_from_order;
    HIP_TRY(c, hipEventElapsedTime(&info->kernel_ms, fs.ev0, fs.ev1));
    return AIC_OK;
}
