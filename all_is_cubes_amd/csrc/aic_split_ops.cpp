// aic_split_ops.cpp -- the operations of the C ABI declared in include/aic_hip.h that act on a resident Split frame: reproject it (aic_reproject_split),
// pick the next pixels to trace (aic_pick_pixels; aic_pick_stale: the pixels a scene change made stale first; aic_pick_stale_cubes: the same from any number of changed boxes and light cubes; aic_find_block_cubes and aic_pick_stale_blocks: the same for a re-evaluated block, whose cubes the device finds), present it (aic_present_split), present it with a line list drawn in (aic_present_split_lines) and
// with the info text laid over it (aic_present_split_text, aic_set_text_font), export it as sRGB8 colour and metric depth (aic_export_split), with the size
// queries and host-only helpers that go with them (aic_reproject_geometry, aic_present_geometry, aic_present_lines_scratch, aic_text_geometry,
// aic_text_layout, aic_export_size).
//
// The operations run on slot 0's stream, synchronously, and are written to one pattern: check the arguments, `begin`, size the context's scratch, fill the
// launcher's parameters, then ev0, the launches, ev1, the copies back to the host and one synchronise, then the context's state and the caller's info.
// Each rule they share is written once, in the anonymous namespace below. Of aic_abi.cpp it uses what aic_ctx.h declares; aic_cursor_wireframe,
// which needs no context, is aic_cursor.cpp, and aic_stale_rects aic_stale_host.cpp. tools/submit_record/split_ops_record.cpp (aic_pick_stale:
// listed_ops_record.cpp) drives every path of this file against a recording fake of the HIP runtime.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aic_hip.h"
#include "aic_bloom.h"
#include "aic_ctx.h"
#include "aic_pick.h"
#include "aic_present_lines.h"
#include "aic_reproject.h"
#include "aic_stale.h"
#include "aic_stale_blocks.h"
#include "aic_stale_cubes.h"

using namespace aic;

static_assert(sizeof(aic_stale_rect) == sizeof(StaleRect) && sizeof(aic_stale_rect) == 16, "the device reads aic_stale_rect as it is");
static_assert(sizeof(aic_stale_cube_rect) == sizeof(StaleCubeRect) && sizeof(aic_stale_cube_rect) == 24, "the probe copies the device's rectangles back as they are");

namespace {

// the kernels address a frame's pixels by 16-bit coordinates
bool above_65535(uint32_t w, uint32_t h) { return w > 65535u || h > 65535u; }

// where a resident Split frame may start: its colour texels are read as 8-byte words; 0: the pointers are fine
int split_frame_rule(aic_ctx *c, const char *who, const void *a, const void *b = nullptr) { return (((uintptr_t)a | (uintptr_t)b) & 7u) ? reject(c, who, "a Split frame starts at an 8-byte boundary") : 0; }

// what the two pickers reject of the arguments they share, up to where a list of pixels may start; unknown_flags: the flag bits the entry point does not know
int pick_args_invalid(aic_ctx *c, const char *who, uint32_t w, uint32_t h, uint32_t unknown_flags, uint32_t n, const uint32_t *pixels_out, const uint32_t *order) {
    if (above_65535(w, h)) return reject(c, who, "frame dimensions above 65535 are not supported");
    if (unknown_flags) return reject(c, who, "unknown flag bits");
    if (n > 2048u * 65535u) return reject(c, who, "more than 2048 x 65535 picks");
    if (n && !pixels_out) return reject(c, who, "no list to write the picks to");
    return (((uintptr_t)pixels_out | (uintptr_t)order) & 3u) ? reject(c, who, "a list starts at a 4-byte boundary") : 0;
}

// How every picker ends once its launcher's parameters are filled: ev0, what `launch` queues, ev1, the picker's 32-byte record back from the head of
// `scratch` -- or, with scratch == nullptr, nothing was looked at and the whole list is the picker's --, one synchronise and the time between the events.
template <class Record, class Launch>
int pick_finish(aic_ctx *c, const char *what, Launch launch, const void *scratch, uint32_t n, unsigned long long cursor, Record &rec, float *kernel_ms) {
    static_assert(sizeof(Record) == 32 && offsetof(Record, head) == 0, "a picker's record: aic_rank_list.h's head and two words of its own");
    aic_ctx::FrameSlot &fs = c->slots[0];
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));
    const hipError_t e = launch(fs.stream);
    if (e != hipSuccess) return hip_fail(c, what, e);
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    rec = Record{};
    if (scratch) {
        HIP_TRY(c, hipMemcpyAsync(&rec, scratch, sizeof(rec), hipMemcpyDeviceToHost, fs.stream));
    } else {
        rec.head.n_from_order = n;
        rec.head.next_cursor = cursor + n;
    }
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    HIP_TRY(c, hipEventElapsedTime(kernel_ms, fs.ev0, fs.ev1));
    return AIC_OK;
}

// What every operation opens with once its arguments are checked: slot 0's stream is the one it queues on. `who` is the entry point the message names.
int begin(aic_ctx *c, const char *who) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->slots[0].busy) return reject(c, who, "a submitted frame still occupies slot 0 (aic_render_wait it first)");
    return AIC_OK;
}

// the checks every size query and presentation shares; nullptr: the sizes are fine
const char *present_sizes_invalid(uint32_t sw, uint32_t sh, uint32_t ow, uint32_t oh) {
    if (above_65535(sw, sh) || above_65535(ow, oh)) return "dimensions above 65535 are not supported";
    if ((uint64_t)ow * oh > AIC_PRESENT_MAX_PIXELS) return "an output of more than 2^31 pixels is not supported";
    if (ow && oh && (!sw || !sh)) return "a source of zero size cannot fill an output";
    return nullptr;
}
size_t present_scratch_texels(const BloomGeom &g, uint32_t sw, uint32_t sh) {
    return (size_t)g.texels + ((sw != g.width || sh != g.height) ? (size_t)g.width * g.height : 0);
}

// two ranges of device memory that share a byte (an empty range shares none)
bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// a presentation's rejections of its arguments, in the order the header lists them, under the entry point's name; 0: none
int present_args_invalid(aic_ctx *c, const aic_present_desc *d, const void *src, const void *out, int out_is_device, aic_present_info *info, const char *who) {
    if (!c || !d || !src || !out) return reject(c, who, "bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    if (const char *why = present_sizes_invalid(d->src_width, d->src_height, d->out_width, d->out_height)) return reject(c, who, why);
    if (d->flags & ~AIC_PRESENT_OUT_F16) return reject(c, who, "unknown flag bits");
    if (!(d->bloom_intensity >= 0.f) || std::isinf(d->bloom_intensity)) return reject(c, who, "bloom_intensity is NaN, negative or infinite");
    if (!(d->maximum_intensity >= 0.f)) return reject(c, who, "maximum_intensity is NaN or negative");
    if (d->tone_mapping != 0 && d->tone_mapping != 1) return reject(c, who, "tone_mapping is neither 0 (Clamp) nor 1 (Reinhard)");
    const size_t px_bytes = (d->flags & AIC_PRESENT_OUT_F16) ? 8 : 4;
    const size_t src_bytes = (size_t)d->src_width * d->src_height * 12, out_bytes = (size_t)d->out_width * d->out_height * px_bytes;
    if (const int rc = split_frame_rule(c, who, src)) return rc;
    if (out_is_device) {
        const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out;
        if (o0 & (px_bytes - 1)) return reject(c, who, "a device out starts at its element's boundary (4 bytes for RGBA8, 8 for f16)");
        if (s0 < o0 + out_bytes && o0 < s0 + src_bytes) return reject(c, who, "out overlaps src");
    }
    return 0;
}

// what aic_present_split_lines adds to a presentation's rejections, under the entry point's name; 0: none
int lines_args_invalid(aic_ctx *c, const aic_lines_desc *ld, const char *who) {
    if (ld->flags & ~AIC_LINES_DEVICE) return reject(c, who, "unknown line flag bits");
    if (ld->n_lines > AIC_LINES_MAX) return reject(c, who, "more than AIC_LINES_MAX lines");
    if (ld->n_lines && !ld->vertices) return reject(c, who, "no vertices");
    if (ld->n_lines && (ld->flags & AIC_LINES_DEVICE) && ((uintptr_t)ld->vertices & 3u)) return reject(c, who, "device vertices start at a 4-byte boundary");
    for (float v : ld->view_projection)
        if (!std::isfinite(v)) return reject(c, who, "a component of view_projection is not finite");
    return 0;
}

// a font cell's rejections, shared by aic_set_text_font and aic_text_geometry
bool text_cell_invalid(uint32_t cw, uint32_t ch, uint32_t margin) {
    return cw < 1u || cw > 1024u || ch < 1u || ch > 1024u || 2ull * margin >= (cw < ch ? cw : ch);
}
// what aic_present_split_text adds
int text_args_invalid(aic_ctx *c, const aic_text_desc *td, const char *who) {
    if (td->flags & ~AIC_TEXT_DEVICE) return reject(c, who, "unknown text flag bits");
    if (!c->text_atlas.n) return reject(c, who, "no font set (aic_set_text_font)");
    if (!td->codes) return reject(c, who, "no codes");
    if (!td->cols || !td->rows || above_65535(td->cols, td->rows)) return reject(c, who, "cols or rows of 0 or above 65535");
    for (float v : {td->scale[0], td->scale[1], td->origin[0], td->origin[1]})
        if (!std::isfinite(v)) return reject(c, who, "a component of scale or origin is not finite");
    return 0;
}

// [lo, hi) of the n output pixels along one axis outside which the cells [c_lo, c_hi) of `cells` cannot be among a pixel's four: a pixel centre at
// tc (in cells) reaches the cells floor(tc - 0.5) and the next, so cell k is in reach of tc in [k - 0.5, k + 1.5), and the range is grown to whole
// cells on both sides. tc = ((x + 0.5) / n - origin) * scale * cells is inverted in f64; the slack covers the kernel's f32 roundings, which are 2^-23
// relative to 1 + |origin| + |a| in window units, eight times over, and two pixels. Anything that is not a plain increasing map gives the whole axis.
void text_reach(uint32_t n, float scale, float origin, uint32_t cells, uint32_t c_lo, uint32_t c_hi, uint32_t *lo, uint32_t *hi) {
    *lo = 0u;
    *hi = n;
    const double k = (double)scale * (double)cells;
    if (!(k > 0.0)) return;
    const double a_lo = ((double)c_lo - 1.0) / k, a_hi = ((double)c_hi + 1.0) / k;
    const double slack = 2.0 + (double)n * (1.0 / 1048576.0) * (1.0 + std::fabs((double)origin) + std::fmax(std::fabs(a_lo), std::fabs(a_hi)));
    const double x_lo = std::floor((a_lo + (double)origin) * (double)n - 0.5 - slack), x_hi = std::ceil((a_hi + (double)origin) * (double)n - 0.5 + slack) + 1.0;
    if (!std::isfinite(x_lo) || !std::isfinite(x_hi)) return;
    *lo = x_lo <= 0.0 ? 0u : (x_lo >= (double)n ? n : (uint32_t)x_lo);
    *hi = x_hi <= 0.0 ? 0u : (x_hi >= (double)n ? n : (uint32_t)x_hi);
    if (*hi < *lo) *hi = *lo;
}

// A presentation, with the lines of `ld` drawn into the scene or (ld == nullptr) without, and with the text of `td` laid over the tone-mapped scene or
// (td == nullptr) without: the body of aic_present_split, aic_present_split_lines and aic_present_split_text.
// Without lines the frame goes through launch_present as it is. With lines launch_present_scene stores the scene S in the line scratch, the line pass
// draws into it, and launch_present shows that S' at its own size -- so the presentation scratch then holds the chain's mips alone.
int present(aic_ctx *c, const aic_present_desc *d, const aic_lines_desc *ld, const aic_text_desc *td, const void *src, void *out, int out_is_device,
            aic_present_info *info, aic_lines_info *lines_info, const char *who) {
    if (const int rc = present_args_invalid(c, d, src, out, out_is_device, info, who)) return rc;
    const bool f16 = (d->flags & AIC_PRESENT_OUT_F16) != 0;
    const size_t npix = (size_t)d->out_width * d->out_height, out_bytes = npix * (f16 ? 8 : 4);
    if (const int rc = begin(c, who)) return rc;
    if (!npix) return AIC_OK;
    const BloomGeom g = bloom_geometry(d->out_width, d->out_height);
    const bool bloomed = d->bloom_intensity > 0.f, staged = ld && !(ld->flags & AIC_LINES_DEVICE);
    hipError_t e;
    if (bloomed && (e = c->present_scratch.ensure(ld ? g.texels : present_scratch_texels(g, d->src_width, d->src_height))) != hipSuccess)
        return hip_fail(c, "alloc presentation scratch", e);
    LinesLayout lay;
    if (ld) {
        lay = lines_layout(d->out_width, d->out_height, staged ? ld->n_lines : 0u);
        const unsigned char *scratch_before = c->lines_scratch.p;
        if ((e = c->lines_scratch.ensure(lay.bytes)) != hipSuccess) return hip_fail(c, "alloc line scratch", e);
        if (c->lines_scratch.p != scratch_before) c->lines_keys_clean = 0;
    }
    if (!out_is_device && (e = c->out.ensure(out_bytes / 4)) != hipSuccess) return hip_fail(c, "alloc output", e);
    const bool text_staged = td && !(td->flags & AIC_TEXT_DEVICE);
    const size_t n_codes = td ? (size_t)td->cols * td->rows : 0;
    if (text_staged && (e = c->text_codes.ensure(n_codes)) != hipSuccess) return hip_fail(c, "alloc text staging", e);
    aic_ctx::FrameSlot &fs = c->slots[0];
    unsigned char *const ls = c->lines_scratch.p;
    PresentParams pp;
    pp.src = (const uint2 *)src;
    pp.src_width = d->src_width;
    pp.src_height = d->src_height;
    pp.mips = bloomed ? c->present_scratch.p : nullptr;
    pp.scene = ld ? (uint2 *)(ls + lay.scene) : (bloomed ? c->present_scratch.p + g.texels : nullptr);
    pp.out = out_is_device ? out : (void *)c->out.p;
    pp.intensity = d->bloom_intensity;
    pp.tone_mapping = d->tone_mapping;
    pp.maximum_intensity = d->maximum_intensity;
    pp.srgb_thr = c->srgb_thr.p;
    pp.out_f16 = f16;
    if (td) {
        PresentText &tx = pp.text;
        tx.codes = text_staged ? c->text_codes.p : td->codes;
        tx.atlas = c->text_atlas.p;
        std::memcpy(tx.scale, td->scale, sizeof(tx.scale));
        std::memcpy(tx.origin, td->origin, sizeof(tx.origin));
        tx.cols = td->cols;
        tx.rows = td->rows;
        tx.cell_w = c->text_cell_w;
        tx.cell_h = c->text_cell_h;
        tx.margin = c->text_margin;
        // the pixels in reach of a cell that can hold a non-zero code; every other cell shows the atlas's cell 0x20, which must then be blank
        uint32_t used[2] = {td->cols, td->rows};
        if (text_staged) {
            used[0] = used[1] = 0u;
            for (uint32_t y = 0; y < td->rows; y++)
                for (uint32_t x = 0; x < td->cols; x++)
                    if (td->codes[(size_t)y * td->cols + x]) { used[0] = used[0] > x + 1u ? used[0] : x + 1u; used[1] = y + 1u; }
        }
        tx.x0 = tx.y0 = 0u;
        tx.x1 = d->out_width;
        tx.y1 = d->out_height;
        if (c->text_space_blank) {
            if (!used[0]) tx.x1 = tx.y1 = 0u;
            else {
                text_reach(d->out_width, td->scale[0], td->origin[0], td->cols, 0u, used[0], &tx.x0, &tx.x1);
                text_reach(d->out_height, td->scale[1], td->origin[1], td->rows, 0u, used[1], &tx.y0, &tx.y1);
            }
        }
        if (text_staged) HIP_TRY(c, hipMemcpyAsync(c->text_codes.p, td->codes, n_codes, hipMemcpyHostToDevice, fs.stream));
    }
    LinesParams lp = {};
    if (ld) {
        lp.vertices = staged ? (const float *)(ls + lay.vertices) : (const float *)ld->vertices;
        lp.n_lines = ld->n_lines;
        std::memcpy(lp.m, ld->view_projection, sizeof(lp.m));
        lp.depth = (const uint32_t *)((const unsigned char *)src + (size_t)d->src_width * d->src_height * 8);
        lp.src_width = d->src_width;
        lp.src_height = d->src_height;
        lp.width = d->out_width;
        lp.height = d->out_height;
        lp.keys = (unsigned long long *)(ls + lay.keys);
        lp.scene = pp.scene;
        lp.counts = (LinesCounts *)(ls + lay.counts);
        lp.reset_keys = !c->sw.lines_clear_keys;
        lp.clear_keys = !lp.reset_keys || c->lines_keys_clean < npix;
        c->lines_keys_clean = 0;  // until the call has finished
        if (staged) HIP_TRY(c, hipMemcpyAsync(ls + lay.vertices, ld->vertices, (size_t)ld->n_lines * sizeof(aic_line_vertex) * 2, hipMemcpyHostToDevice, fs.stream));
    }
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));
    if (ld) {
        launch_present_scene(g, pp, fs.stream);
        if ((e = launch_present_lines(lp, fs.stream)) != hipSuccess) return hip_fail(c, "launch line pass", e);
        pp.src = pp.scene;  // S' shown at its own size
        pp.src_width = d->out_width;
        pp.src_height = d->out_height;
    }
    launch_present(g, pp, fs.stream);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(c, "launch presentation", e);
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    LinesCounts counts;
    if (ld) HIP_TRY(c, hipMemcpyAsync(&counts, lp.counts, sizeof(counts), hipMemcpyDeviceToHost, fs.stream));
    if (!out_is_device) HIP_TRY(c, hipMemcpyAsync(out, c->out.p, out_bytes, hipMemcpyDeviceToHost, fs.stream));
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    if (ld && lp.reset_keys) c->lines_keys_clean = npix;
    if (ld && lines_info) {
        lines_info->n_clipped_away = counts.n_clipped_away;
        lines_info->n_fragments = counts.n_fragments;
        lines_info->n_passed = counts.n_passed;
        lines_info->n_pixels = counts.n_pixels;
    }
    if (info) {
        HIP_TRY(c, hipEventElapsedTime(&info->kernel_ms, fs.ev0, fs.ev1));
        info->levels = g.levels;
        info->t0[0] = g.mw[0];
        info->t0[1] = g.mh[0];
        info->bloomed = bloomed ? 1u : 0u;
    }
    return AIC_OK;
}

}  // namespace

extern "C" {

int aic_reproject_geometry(uint32_t width, uint32_t height, uint32_t *levels, uint32_t t0[2], uint64_t *scratch_bytes) {
    if (above_65535(width, height)) return AIC_ERR_INVALID;
    const ReprojectGeom g = reproject_geometry(width, height);
    if (levels) *levels = g.levels;
    if (t0) { t0[0] = g.mw[0]; t0[1] = g.mh[0]; }
    if (scratch_bytes) *scratch_bytes = g.scratch_bytes();
    return AIC_OK;
}

int aic_reproject_split(aic_ctx *c, const aic_reproject_desc *d, const void *src, void *dst, aic_reproject_info *info) {
    if (!c || !d || !src || !dst) return fail(c, AIC_ERR_INVALID, "aic_reproject_split: bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    if (above_65535(d->width, d->height)) return fail(c, AIC_ERR_INVALID, "aic_reproject_split: frame dimensions above 65535 are not supported");
    if (d->flags & ~AIC_REPROJECT_KEEP_SPLATS) return fail(c, AIC_ERR_INVALID, "aic_reproject_split: unknown flag bits");
    if (const int rc = split_frame_rule(c, "aic_reproject_split", src, dst)) return rc;
    for (float v : d->reprojection)
        if (!std::isfinite(v)) return fail(c, AIC_ERR_INVALID, "aic_reproject_split: a component of the reprojection matrix is not finite");
    for (float v : d->inverse_projection_zw)
        if (!std::isfinite(v)) return fail(c, AIC_ERR_INVALID, "aic_reproject_split: a component of inverse_projection_zw is not finite");
    const ReprojectGeom g = reproject_geometry(d->width, d->height);
    const size_t npix = g.npix(), frame_bytes = npix * 12;
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    if (s0 == d0 || (s0 < d0 + frame_bytes && d0 < s0 + frame_bytes)) return fail(c, AIC_ERR_INVALID, "aic_reproject_split: src and dst overlap");
    if (const int rc = begin(c, "aic_reproject_split")) return rc;
    if (!npix) return AIC_OK;  // (nothing written: the splat image of an earlier call stays what aic_pick_pixels reads)
    const unsigned char *scratch_before = c->reproject_scratch.p;
    hipError_t e = c->reproject_scratch.ensure(g.scratch_bytes());
    if (e != hipSuccess) return hip_fail(c, "alloc reprojection scratch", e);
    // a new allocation has lost the splat image aic_pick_pixels reads: if this call then fails, there is none
    if (c->reproject_scratch.p != scratch_before) c->reproject_valid_w = c->reproject_valid_h = 0u;
    aic_ctx::FrameSlot &fs = c->slots[0];
    ReprojectParams rp;
    rp.src_color = (const uint2 *)src;
    rp.src_depth = (const float *)((const unsigned char *)src + npix * 8);
    rp.dst_color = (uint2 *)dst;
    rp.dst_depth = (float *)((unsigned char *)dst + npix * 8);
    rp.scratch = c->reproject_scratch.p;
    std::memcpy(rp.m, d->reprojection, sizeof(rp.m));
    std::memcpy(rp.ipzw, d->inverse_projection_zw, sizeof(rp.ipzw));
    rp.keep_splats = (d->flags & AIC_REPROJECT_KEEP_SPLATS) ? 1u : 0u;
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));
    if ((e = launch_reproject(g, rp, fs.stream)) != hipSuccess) return hip_fail(c, "launch reprojection", e);
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    ReprojectCounts counts;
    HIP_TRY(c, hipMemcpyAsync(&counts, reproject_counts(g, c->reproject_scratch.p), sizeof(counts), hipMemcpyDeviceToHost, fs.stream));
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    c->reproject_valid_w = d->width;
    c->reproject_valid_h = d->height;
    if (info) {
        info->n_splats = counts.n_splats;
        info->n_dropped = counts.n_dropped;
        info->n_gaps = counts.n_gaps;
        info->n_unfilled = counts.n_unfilled;
        HIP_TRY(c, hipEventElapsedTime(&info->kernel_ms, fs.ev0, fs.ev1));
        info->levels = g.levels;
        info->t0[0] = g.mw[0];
        info->t0[1] = g.mh[0];
    }
    return AIC_OK;
}

int aic_pick_pixels(aic_ctx *c, const aic_pick_desc *d, const uint32_t *order, uint32_t *pixels_out, aic_pick_info *info) {
    if (!c || !d || !info) return fail(c, AIC_ERR_INVALID, "aic_pick_pixels: bad argument");
    std::memset(info, 0, sizeof(*info));
    if (const int rc = pick_args_invalid(c, "aic_pick_pixels", d->width, d->height, d->flags, d->n, pixels_out, order)) return rc;
    const uint64_t count = (uint64_t)d->width * d->height;
    if (d->n && !count) return fail(c, AIC_ERR_INVALID, "aic_pick_pixels: an empty frame has no pixel to pick");
    if (const int rc = begin(c, "aic_pick_pixels")) return rc;
    if (!d->n) return AIC_OK;  // (and so count == 0)
    if (d->max_unknown && (!c->reproject_scratch.p || c->reproject_valid_w != d->width || c->reproject_valid_h != d->height))
        return fail(c, AIC_ERR_INVALID, "aic_pick_pixels: max_unknown needs the context's last successful aic_reproject_split to be of this size");
    hipError_t e;
    if (d->max_unknown && (e = c->pick_scratch.ensure(pick_scratch_words(count))) != hipSuccess) return hip_fail(c, "alloc pick scratch", e);
    PickParams pp;
    pp.R = d->max_unknown ? (const uint2 *)(c->reproject_scratch.p + reproject_geometry(d->width, d->height).keys_bytes()) : nullptr;
    pp.order = order;
    pp.out = pixels_out;
    pp.scratch = d->max_unknown ? c->pick_scratch.p : nullptr;
    pp.count = (uint32_t)count;  // at most 65535^2
    pp.n = d->n;
    pp.max_unknown = d->max_unknown;
    pp.skip_unknown = d->skip_unknown;
    pp.cursor = d->cursor;
    PickRecord rec;
    if (const int rc = pick_finish(c, "launch pick", [&](hipStream_t s) { return launch_pick(pp, s); }, pp.scratch, d->n, d->cursor, rec, &info->kernel_ms)) return rc;
    info->n_unknown = rec.head.n_set;
    info->next_cursor = rec.head.next_cursor;
    info->n_from_unknown = rec.head.n_from_set;
    info->n_from_order = rec.head.n_from_order;
    return AIC_OK;
}

int aic_pick_stale(aic_ctx *c, const aic_stale_desc *d, const void *src, const uint32_t *order, uint32_t *pixels_out, aic_stale_info *info) {
    const char *who = "aic_pick_stale";
    if (!c || !d || !info) return reject(c, who, "bad argument");
    std::memset(info, 0, sizeof(*info));
    if (const int rc = pick_args_invalid(c, who, d->width, d->height, d->flags & ~AIC_STALE_DEPTH_TEST, d->n, pixels_out, order)) return rc;
    if (const int rc = split_frame_rule(c, who, src)) return rc;
    const uint64_t count = (uint64_t)d->width * d->height;
    if (d->n && !count) return reject(c, who, "an empty frame has no pixel to pick");
    if (d->n_rects > AIC_STALE_MAX_RECTS) return reject(c, who, "more than AIC_STALE_MAX_RECTS rectangles");
    if (d->n_rects && !d->rects) return reject(c, who, "no rectangles");
    std::vector<aic_stale_rect> rects;  // the ones that hold a pixel
    for (uint32_t i = 0; i < d->n_rects; i++) {
        const aic_stale_rect &r = d->rects[i];
        if (r.x0 > r.x1 || r.y0 > r.y1 || r.x1 > d->width || r.y1 > d->height) return reject(c, who, "a rectangle is inside out or leaves the frame");
        if (std::isnan(r.dmin)) return reject(c, who, "a rectangle's dmin is NaN");
        if (r.x0 < r.x1 && r.y0 < r.y1) rects.push_back(r);
    }
    const bool depth_test = (d->flags & AIC_STALE_DEPTH_TEST) != 0;
    const uint32_t n_rects = (uint32_t)rects.size();
    // whether anything is looked at (no rectangle that holds a pixel: the kernels would count nothing, the answer is known)
    const bool look = d->n && n_rects && d->max_stale;
    if (d->n && d->n_rects && d->max_stale && depth_test && !src) return reject(c, who, "no frame to test the depths of");
    if (const int rc = begin(c, who)) return rc;
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
    StaleRecord rec;  // (pick_finish synchronises before `rects` goes out of scope)
    if (const int rc = pick_finish(c, "launch pick stale", [&](hipStream_t s) { return launch_pick_stale(sp, s); }, sp.scratch, d->n, d->cursor, rec, &info->kernel_ms)) return rc;
    info->n_stale = rec.head.n_set;
    info->next_cursor = rec.head.next_cursor;
    info->n_from_stale = rec.head.n_from_set;
    info->n_from_order = rec.head.n_from_order;
    return AIC_OK;
}

namespace {

// what aic_pick_stale_cubes and its probe reject of the boxes, the light cubes and the camera; 0: none
int stale_cubes_args_invalid(aic_ctx *c, const char *who, const aic_stale_cubes_desc *d) {
    if (above_65535(d->width, d->height)) return reject(c, who, "frame dimensions above 65535 are not supported");
    if (d->n_boxes && !d->boxes) return reject(c, who, "no boxes");
    if (d->n_light_cubes && !d->light_cubes) return reject(c, who, "no light cubes");
    if ((uint64_t)d->n_boxes + d->n_light_cubes > 0xFFFFFFFFull) return reject(c, who, "more than 2^32 - 1 boxes and light cubes");
    if (d->expand < 0) return reject(c, who, "a negative expand");
    for (double v : d->view_projection)
        if (!std::isfinite(v)) return reject(c, who, "a component of view_projection is not finite");
    return 0;
}

// sizes the scratch for the desc's boxes and cubes and for n_found more boxes behind the desc's own (aic_pick_stale_blocks: the device writes those),
// fills the launcher's parameters that describe them and queues the copy of the desc's to the device
int stale_cubes_stage(aic_ctx *c, const aic_stale_cubes_desc *d, StaleCubesParams &sp, hipStream_t stream, uint32_t n_found = 0u) {
    const uint32_t n_boxes = d->n_boxes + n_found;  // (the entry points have checked the sums)
    hipError_t e = c->stale_cubes_scratch.ensure(stale_cubes_scratch_bytes(d->width, d->height, n_boxes, d->n_light_cubes));
    if (e != hipSuccess) return hip_fail(c, "alloc stale cubes scratch", e);
    unsigned char *s = c->stale_cubes_scratch.p;
    const size_t in0 = stale_cubes_input_offset(d->width, d->height, (uint64_t)n_boxes + d->n_light_cubes), own_bytes = 24u * (size_t)d->n_boxes, box_bytes = 24u * (size_t)n_boxes;
    sp.scratch = s;
    sp.rects = (StaleCubeRect *)(s + stale_cubes_rects_offset(d->width, d->height));
    sp.boxes = (const int32_t *)(s + in0);
    sp.light_cubes = (const int32_t *)(s + in0 + box_bytes);
    std::memcpy(sp.m, d->view_projection, sizeof(sp.m));
    sp.width = d->width;
    sp.height = d->height;
    sp.n_boxes = n_boxes;
    sp.n_light_cubes = d->n_light_cubes;
    sp.expand = d->expand;
    if (d->n_boxes) HIP_TRY(c, hipMemcpyAsync(s + in0, d->boxes, own_bytes, hipMemcpyHostToDevice, stream));
    if (d->n_light_cubes) HIP_TRY(c, hipMemcpyAsync(s + in0 + box_bytes, d->light_cubes, 12u * (size_t)d->n_light_cubes, hipMemcpyHostToDevice, stream));
    return AIC_OK;
}

// A find of the cubes that hold given blocks (aic_find_block_cubes, and aic_pick_stale_blocks' part of it)
struct BlockFind {
    int layer;
    uint32_t n_blocks;
    const uint32_t *indices;
    uint32_t capacity;
};

// what both entry points reject of a find; 0: nothing
int block_find_invalid(aic_ctx *c, const char *who, const BlockFind &f) {
    if (!valid_layer(f.layer)) return reject(c, who, "a layer that is neither 0 nor 1");
    const Layer &l = c->layers[f.layer];
    if (!l.present) return reject(c, who, "no space uploaded for the layer");
    if (f.n_blocks && !f.indices) return reject(c, who, "no block indices");
    for (uint32_t i = 0; i < f.n_blocks; i++)
        if (f.indices[i] >= l.host_blocks.size()) return reject(c, who, "a block index at or above the layer's block count");
    if (block_cubes_groups(l.n_cubes()) > 0x7FFFFFFFull) return reject(c, who, "a grid of more than 2048 x (2^31 - 1) cubes");
    return 0;
}

// whether the find has anything to scan
bool block_find_scans(const aic_ctx *c, const BlockFind &f) { return f.n_blocks && c->layers[f.layer].n_cubes(); }

// the events around the write of a pick's find, whose own two are taken by the pick's launches
int block_find_events(aic_ctx *c) {
    for (hipEvent_t &ev : c->stale_blocks_ev)
        if (!ev) HIP_TRY(c, hipEventCreate(&ev));
    return AIC_OK;
}

// The count of a find that scans: the set and the record's initial value go to the scratch, the count runs, the stream is synchronised and the record
// read: *info is complete but for the time of the write, and bp describes the grid for launch_write_block_cubes (boxes and n_runs are the caller's to
// fill in).
int block_find_count(aic_ctx *c, const BlockFind &f, aic_ctx::FrameSlot &fs, BlockCubesParams &bp, aic_block_cubes_info *info) {
    const Layer &l = c->layers[f.layer];
    const uint32_t set_words = (uint32_t)((l.host_blocks.size() + 31u) / 32u);  // at most kBlockSetWords: a table holds at most 65536 blocks
    std::vector<uint32_t> head(sizeof(BlockCubesRecord) / 4u + set_words, 0u);  // the record, then the set
    BlockCubesRecord rec = {};
    rec.lo[0] = rec.lo[1] = rec.lo[2] = 0xFFFFFFFFu;
    std::memcpy(head.data(), &rec, sizeof(rec));
    for (uint32_t i = 0; i < f.n_blocks; i++) head[sizeof(rec) / 4u + (f.indices[i] >> 5)] |= 1u << (f.indices[i] & 31u);
    hipError_t e = c->stale_blocks_scratch.ensure(block_cubes_scratch_bytes(set_words, l.n_cubes()));
    if (e != hipSuccess) return hip_fail(c, "alloc stale blocks scratch", e);
    bp = BlockCubesParams{};
    bp.grid = l.pool.p;
    bp.n = l.n_cubes();
    bp.sx = (uint32_t)l.size[0];
    bp.sy = (uint32_t)l.size[1];
    bp.sz = (uint32_t)l.size[2];
    bp.index_mask = l.cls_in_code ? kCubeIndexMask : 0xffffu;
    bp.set_words = set_words;
    for (int a = 0; a < 3; a++) bp.lo[a] = l.lo[a];
    bp.scratch = c->stale_blocks_scratch.p;
    HIP_TRY(c, hipMemcpyAsync(bp.scratch, head.data(), head.size() * 4u, hipMemcpyHostToDevice, fs.stream));
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));
    if ((e = launch_count_block_cubes(bp, fs.stream)) != hipSuccess) return hip_fail(c, "launch count block cubes", e);
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    HIP_TRY(c, hipMemcpyAsync(&rec, bp.scratch, sizeof(rec), hipMemcpyDeviceToHost, fs.stream));
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    HIP_TRY(c, hipEventElapsedTime(&info->kernel_ms, fs.ev0, fs.ev1));
    info->n_cubes = rec.n_cubes;
    info->n_runs = rec.n_runs;
    if (rec.n_cubes)
        for (int a = 0; a < 3; a++) {
            info->bounds[a] = l.lo[a] + (int32_t)rec.lo[a];
            info->bounds[3 + a] = l.lo[a] + (int32_t)rec.hi[a];
        }
    info->merged = rec.n_runs > f.capacity ? 1u : 0u;
    info->n_written = info->merged ? (f.capacity ? 1u : 0u) : (uint32_t)rec.n_runs;
    return AIC_OK;
}

// aic_pick_stale_cubes (find == nullptr), and aic_pick_stale_blocks: the same call with the find's boxes behind the desc's own. info is zeroed.
int pick_stale_cubes_with(aic_ctx *c, const char *who, const aic_stale_cubes_desc *d, const BlockFind *find, const void *src, const uint32_t *order, uint32_t *pixels_out,
                          aic_stale_cubes_info *info, aic_block_cubes_info *found) {
    if (const int rc = pick_args_invalid(c, who, d->width, d->height, d->flags & ~(AIC_STALE_DEPTH_TEST | AIC_STALE_DEPTH_BEHIND), d->n, pixels_out, order)) return rc;
    if (const int rc = split_frame_rule(c, who, src)) return rc;
    const uint64_t count = (uint64_t)d->width * d->height;
    if (d->n && !count) return reject(c, who, "an empty frame has no pixel to pick");
    if (const int rc = stale_cubes_args_invalid(c, who, d)) return rc;
    if (find) {
        if (const int rc = block_find_invalid(c, who, *find)) return rc;
        if ((uint64_t)d->n_boxes + find->capacity + d->n_light_cubes > 0xFFFFFFFFull) return reject(c, who, "more than 2^32 - 1 boxes, runs and light cubes");
    }
    const bool front = (d->flags & AIC_STALE_DEPTH_TEST) != 0, behind = (d->flags & AIC_STALE_DEPTH_BEHIND) != 0;
    // a find runs when anything can be looked at; what it finds is known only once it has run, so a frame that may be read counts as read
    const bool finds = find && d->n && d->max_stale && block_find_scans(c, *find);
    const bool may_look = d->n && d->max_stale && (d->n_boxes || d->n_light_cubes || finds);
    if (may_look && (front || (behind && d->n_light_cubes)) && !src) return reject(c, who, "no frame to test the depths of");
    if (const int rc = begin(c, who)) return rc;
    if (!d->n) return AIC_OK;  // (and so count == 0)
    aic_ctx::FrameSlot &fs = c->slots[0];
    BlockCubesParams bp = {};
    uint32_t n_found = 0u;
    if (finds) {
        if (const int rc = block_find_events(c)) return rc;
        if (const int rc = block_find_count(c, *find, fs, bp, found)) return rc;
        n_found = found->n_written;
    }
    const uint32_t n_total = d->n_boxes + n_found + d->n_light_cubes;
    const bool look = d->n && n_total && d->max_stale;  // whether anything is looked at
    const bool reads_frame = look && (front || (behind && d->n_light_cubes));
    StaleCubesParams sp = {};
    if (look)
        if (const int rc = stale_cubes_stage(c, d, sp, fs.stream, n_found)) return rc;
    hipError_t e;
    if (n_found) {  // the found boxes, behind the desc's own: the one box of a merged find from the host's record, else written where the pick reads them
        int32_t *at = const_cast<int32_t *>(sp.boxes) + 6u * (size_t)d->n_boxes;
        if (found->merged) {
            HIP_TRY(c, hipMemcpyAsync(at, found->bounds, sizeof(found->bounds), hipMemcpyHostToDevice, fs.stream));
        } else {
            bp.boxes = at;
            bp.n_runs = n_found;
            HIP_TRY(c, hipEventRecord(c->stale_blocks_ev[0], fs.stream));
            if ((e = launch_write_block_cubes(bp, fs.stream)) != hipSuccess) return hip_fail(c, "launch write block cubes", e);
            HIP_TRY(c, hipEventRecord(c->stale_blocks_ev[1], fs.stream));
        }
    }
    sp.color = reads_frame ? (const uint2 *)src : nullptr;
    sp.depth = reads_frame ? (const float *)((const unsigned char *)src + count * 8u) : nullptr;
    sp.order = order;
    sp.out = pixels_out;
    sp.width = d->width;
    sp.height = d->height;
    sp.n = d->n;
    sp.max_stale = look ? d->max_stale : 0u;
    sp.depth_front = front ? 1u : 0u;
    sp.depth_behind = behind ? 1u : 0u;
    sp.skip_stale = d->skip_stale;
    sp.cursor = d->cursor;
    StaleCubesRecord rec;
    if (const int rc = pick_finish(c, "launch pick stale cubes", [&](hipStream_t s) { return launch_pick_stale_cubes(sp, s); }, sp.scratch, d->n, d->cursor, rec, &info->kernel_ms)) return rc;
    info->n_stale = rec.head.n_set;
    info->next_cursor = rec.head.next_cursor;
    info->n_from_stale = rec.head.n_from_set;
    info->n_from_order = rec.head.n_from_order;
    info->n_rects = rec.n_rects;
    info->whole_frame = rec.whole_frame ? 1u : 0u;
    if (n_found && !found->merged) {
        float write_ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&write_ms, c->stale_blocks_ev[0], c->stale_blocks_ev[1]));
        found->kernel_ms += write_ms;
    }
    return AIC_OK;
}

}  // namespace

int aic_pick_stale_cubes(aic_ctx *c, const aic_stale_cubes_desc *d, const void *src, const uint32_t *order, uint32_t *pixels_out, aic_stale_cubes_info *info) {
    const char *who = "aic_pick_stale_cubes";
    if (!c || !d || !info) return reject(c, who, "bad argument");
    std::memset(info, 0, sizeof(*info));
    return pick_stale_cubes_with(c, who, d, nullptr, src, order, pixels_out, info, nullptr);
}

int aic_pick_stale_blocks(aic_ctx *c, const aic_stale_blocks_desc *d, const void *src, const uint32_t *order, uint32_t *pixels_out, aic_stale_blocks_info *info) {
    const char *who = "aic_pick_stale_blocks";
    if (!c || !d || !info) return reject(c, who, "bad argument");
    std::memset(info, 0, sizeof(*info));
    const BlockFind find = {d->layer, d->n_blocks, d->block_indices, d->max_runs};
    return pick_stale_cubes_with(c, who, &d->cubes, d->n_blocks ? &find : nullptr, src, order, pixels_out, &info->pick, &info->found);
}

int aic_find_block_cubes(aic_ctx *c, int layer, uint32_t n_blocks, const uint32_t *block_indices, uint32_t capacity, int32_t *out_boxes, aic_block_cubes_info *info) {
    const char *who = "aic_find_block_cubes";
    if (!c || !info) return reject(c, who, "bad argument");
    std::memset(info, 0, sizeof(*info));
    const BlockFind find = {layer, n_blocks, block_indices, capacity};
    if (const int rc = block_find_invalid(c, who, find)) return rc;
    if (capacity && !out_boxes) return reject(c, who, "no boxes to write to");
    if (const int rc = begin(c, who)) return rc;
    if (!block_find_scans(c, find)) return AIC_OK;
    aic_ctx::FrameSlot &fs = c->slots[0];
    BlockCubesParams bp = {};
    if (const int rc = block_find_count(c, find, fs, bp, info)) return rc;
    if (!info->n_written) return AIC_OK;
    if (info->merged) {
        std::memcpy(out_boxes, info->bounds, sizeof(info->bounds));
        return AIC_OK;
    }
    hipError_t e = c->stale_blocks_boxes.ensure(6u * (size_t)info->n_written);
    if (e != hipSuccess) return hip_fail(c, "alloc stale blocks boxes", e);
    bp.boxes = c->stale_blocks_boxes.p;
    bp.n_runs = info->n_written;
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));  // (the count's time has been read)
    if ((e = launch_write_block_cubes(bp, fs.stream)) != hipSuccess) return hip_fail(c, "launch write block cubes", e);
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    HIP_TRY(c, hipMemcpyAsync(out_boxes, bp.boxes, 24u * (size_t)info->n_written, hipMemcpyDeviceToHost, fs.stream));
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    float write_ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&write_ms, fs.ev0, fs.ev1));
    info->kernel_ms += write_ms;
    return AIC_OK;
}

int aic_probe_stale_cube_rects(aic_ctx *c, const aic_stale_cubes_desc *d, aic_stale_cube_rect *out) {
    const char *who = "aic_probe_stale_cube_rects";
    if (!c || !d) return reject(c, who, "bad argument");
    if (const int rc = stale_cubes_args_invalid(c, who, d)) return rc;
    const uint32_t n_total = d->n_boxes + d->n_light_cubes;
    if (n_total && !out) return reject(c, who, "no rectangles to write to");
    if (const int rc = begin(c, who)) return rc;
    if (!n_total) return AIC_OK;
    aic_ctx::FrameSlot &fs = c->slots[0];
    StaleCubesParams sp = {};
    if (const int rc = stale_cubes_stage(c, d, sp, fs.stream)) return rc;
    hipError_t e;
    if ((e = launch_project_stale_cubes(sp, fs.stream)) != hipSuccess) return hip_fail(c, "launch project stale cubes", e);
    HIP_TRY(c, hipMemcpyAsync(out, sp.rects, sizeof(StaleCubeRect) * (size_t)n_total, hipMemcpyDeviceToHost, fs.stream));
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    return AIC_OK;
}

int aic_present_geometry(uint32_t src_w, uint32_t src_h, uint32_t out_w, uint32_t out_h, uint32_t *levels, uint32_t t0[2], uint64_t *scratch_bytes) {
    if (present_sizes_invalid(src_w, src_h, out_w, out_h)) return AIC_ERR_INVALID;
    const bool empty = !out_w || !out_h;
    const BloomGeom g = bloom_geometry(out_w, out_h);
    if (levels) *levels = empty ? 0u : g.levels;
    if (t0) { t0[0] = empty ? 0u : g.mw[0]; t0[1] = empty ? 0u : g.mh[0]; }
    if (scratch_bytes) *scratch_bytes = empty ? 0u : (uint64_t)present_scratch_texels(g, src_w, src_h) * 8u;
    return AIC_OK;
}

int aic_present_split(aic_ctx *c, const aic_present_desc *d, const void *src, void *out, int out_is_device, aic_present_info *info) {
    return present(c, d, nullptr, nullptr, src, out, out_is_device, info, nullptr, "aic_present_split");
}

int aic_present_lines_scratch(uint32_t src_w, uint32_t src_h, uint32_t out_w, uint32_t out_h, uint32_t n_lines, uint64_t *bytes) {
    if (present_sizes_invalid(src_w, src_h, out_w, out_h) || n_lines > AIC_LINES_MAX) return AIC_ERR_INVALID;
    if (bytes) *bytes = (n_lines && out_w && out_h) ? (uint64_t)lines_layout(out_w, out_h, n_lines).bytes : 0u;
    return AIC_OK;
}

int aic_present_split_lines(aic_ctx *c, const aic_present_desc *d, const aic_lines_desc *ld, const void *src, void *out, int out_is_device, aic_present_info *info,
                            aic_lines_info *lines_info) {
    if (lines_info) std::memset(lines_info, 0, sizeof(*lines_info));
    if (c && ld) {  // (the rejections this call adds; a NULL ctx is the presentation's to report)
        if (info) std::memset(info, 0, sizeof(*info));
        if (const int rc = lines_args_invalid(c, ld, "aic_present_split_lines")) return rc;
    }
    if (!c || !ld || !ld->n_lines) return aic_present_split(c, d, src, out, out_is_device, info);  // (and reports under that name)
    return present(c, d, ld, nullptr, src, out, out_is_device, info, lines_info, "aic_present_split_lines");
}

int aic_set_text_font(aic_ctx *c, const uint8_t *atlas, uint32_t cell_w, uint32_t cell_h, uint32_t margin) {
    if (!c) return fail(c, AIC_ERR_INVALID, "aic_set_text_font: bad argument");
    if (atlas && text_cell_invalid(cell_w, cell_h, margin))
        return reject(c, "aic_set_text_font", "a cell dimension outside 1..1024, or 2 * cell_margin >= min(cell_width, cell_height)");
    if (const int rc = begin(c, "aic_set_text_font")) return rc;
    if (!atlas) {
        c->text_atlas.release();
        c->text_cell_w = c->text_cell_h = c->text_margin = 0u;
        c->text_space_blank = false;
        return AIC_OK;
    }
    // (slot 0's stream is idle: every operation of this file leaves it so, and no frame occupies the slot)
    const size_t row = 16u * (size_t)cell_w, texels = row * 16u * cell_h;
    const hipError_t e = c->text_atlas.ensure(texels);
    if (e != hipSuccess) return hip_fail(c, "alloc font atlas", e);  // (the font set before stays)
    c->text_atlas.n = 0;  // no font until the new atlas is whole
    aic_ctx::FrameSlot &fs = c->slots[0];
    HIP_TRY(c, hipMemcpyAsync(c->text_atlas.p, atlas, texels * 4, hipMemcpyHostToDevice, fs.stream));
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    c->text_atlas.n = texels;
    c->text_cell_w = cell_w;
    c->text_cell_h = cell_h;
    c->text_margin = margin;
    bool blank = true;  // cell 0x20: column 0, row 2
    for (uint32_t y = 0; y < cell_h && blank; y++)
        for (size_t b = 0; b < (size_t)cell_w * 4; b++)
            if (atlas[((2u * (size_t)cell_h + y) * row) * 4 + b]) { blank = false; break; }
    c->text_space_blank = blank;
    return AIC_OK;
}

int aic_text_geometry(double nominal_w, double nominal_h, uint32_t cell_w, uint32_t cell_h, uint32_t margin, const double origin_px[2], uint32_t *cols, uint32_t *rows,
                      float scale[2], float origin[2]) {
    if (!origin_px || !std::isfinite(nominal_w) || !std::isfinite(nominal_h) || !(nominal_w > 0.0) || !(nominal_h > 0.0)) return AIC_ERR_INVALID;
    if (text_cell_invalid(cell_w, cell_h, margin)) return AIC_ERR_INVALID;
    const uint32_t logical[2] = {cell_w - 2u * margin, cell_h - 2u * margin};
    const double nominal[2] = {nominal_w, nominal_h};
    uint32_t n[2];
    for (int a = 0; a < 2; a++) {
        const double cells = std::ceil(nominal[a] / (double)logical[a]);
        if (cells > 65535.0) return AIC_ERR_INVALID;
        n[a] = cells < 1.0 ? 1u : (uint32_t)cells;
    }
    if (cols) *cols = n[0];
    if (rows) *rows = n[1];
    for (int a = 0; a < 2; a++) {
        if (scale) scale[a] = (float)nominal[a] / (float)(n[a] * logical[a]);
        if (origin) origin[a] = (float)(origin_px[a] / nominal[a]);
    }
    return AIC_OK;
}

int aic_text_layout(const char *utf8, uint64_t len, uint32_t cols, uint32_t rows, uint8_t *codes, uint32_t used[2]) {
    if (!codes || (len && !utf8) || !cols || !rows || above_65535(cols, rows)) return AIC_ERR_INVALID;
    std::memset(codes, 0, (size_t)cols * rows);
    uint32_t x = 0, y = 0, ux = 0, uy = 0;
    for (uint64_t i = 0; i < len;) {
        // the next scalar value (`str::chars`); malformed input cannot occur in a Rust &str, here it decodes to U+FFFD
        uint32_t ch = (unsigned char)utf8[i];
        uint64_t n = 1;
        if (ch >= 0xf0u) { n = 4; ch &= 0x07u; } else if (ch >= 0xe0u) { n = 3; ch &= 0x0fu; } else if (ch >= 0xc0u) { n = 2; ch &= 0x1fu; } else if (ch >= 0x80u) { ch = 0xfffdu; }
        if (i + n > len) { ch = 0xfffdu; n = 1; }
        else for (uint64_t k = 1; k < n; k++) ch = (ch << 6) | ((unsigned char)utf8[i + k] & 0x3fu);
        i += n;
        if (ch == '\n') {
            x = 0;
            if (y != UINT32_MAX) y++;
            continue;
        }
        if (x < cols && y < rows) {
            const uint8_t code = ch <= 0xffu ? (uint8_t)ch : (uint8_t)'?';
            codes[(size_t)y * cols + x] = code;
            if (code) { ux = ux > x + 1u ? ux : x + 1u; uy = uy > y + 1u ? uy : y + 1u; }
        }
        if (x != UINT32_MAX) x++;
    }
    if (used) { used[0] = ux; used[1] = uy; }
    return AIC_OK;
}

int aic_present_split_text(aic_ctx *c, const aic_present_desc *d, const aic_lines_desc *ld, const aic_text_desc *td, const void *src, void *out, int out_is_device,
                           aic_present_info *info, aic_lines_info *lines_info) {
    if (!td) return aic_present_split_lines(c, d, ld, src, out, out_is_device, info, lines_info);  // (and reports under that name, or aic_present_split's)
    if (lines_info) std::memset(lines_info, 0, sizeof(*lines_info));
    if (c) {
        if (info) std::memset(info, 0, sizeof(*info));
        if (ld)
            if (const int rc = lines_args_invalid(c, ld, "aic_present_split_text")) return rc;
        if (const int rc = text_args_invalid(c, td, "aic_present_split_text")) return rc;
    }
    return present(c, d, (ld && ld->n_lines) ? ld : nullptr, td, src, out, out_is_device, info, lines_info, "aic_present_split_text");
}

int aic_export_size(uint32_t width, uint32_t height, double max_area, uint32_t out[2]) {
    if (!out || !(max_area > 0.0)) return AIC_ERR_INVALID;  // (NaN is not > 0)
    out[0] = width;
    out[1] = height;
    const double area = (double)width * (double)height;
    if (area <= max_area) return AIC_OK;
    const double r = std::sqrt(max_area / area);
    out[0] = (uint32_t)std::ceil((double)width * r);
    out[1] = (uint32_t)std::ceil((double)height * r);
    return AIC_OK;
}

int aic_export_split(aic_ctx *c, const aic_export_desc *d, const void *src, void *color_out, float *depth_out, int out_is_device, aic_export_info *info) {
    const char *who = "aic_export_split";
    if (!c || !d || !src) return reject(c, who, "bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    if (!color_out && !depth_out && !info) return reject(c, who, "neither a plane nor the info is asked for");
    if (const char *why = present_sizes_invalid(d->src_width, d->src_height, d->out_width, d->out_height)) return reject(c, who, why);
    if (d->flags) return reject(c, who, "unknown flag bits");
    for (float v : d->inverse_projection_zw)
        if (!std::isfinite(v)) return reject(c, who, "a component of inverse_projection_zw is not finite");
    if (const int rc = split_frame_rule(c, who, src)) return rc;
    const size_t npix = (size_t)d->out_width * d->out_height, plane_bytes = npix * 4, src_bytes = (size_t)d->src_width * d->src_height * 12;
    if (out_is_device) {
        if (((uintptr_t)color_out | (uintptr_t)depth_out) & 3u) return reject(c, who, "a device plane starts at a 4-byte boundary");
        if (ranges_overlap(color_out, color_out ? plane_bytes : 0, src, src_bytes)) return reject(c, who, "color_out overlaps src");
        if (ranges_overlap(depth_out, depth_out ? plane_bytes : 0, src, src_bytes)) return reject(c, who, "depth_out overlaps src");
        if (ranges_overlap(color_out, color_out ? plane_bytes : 0, depth_out, depth_out ? plane_bytes : 0)) return reject(c, who, "color_out and depth_out overlap");
    }
    if (const int rc = begin(c, who)) return rc;
    if (!npix) return AIC_OK;
    hipError_t e;
    if ((e = c->export_counts.ensure(sizeof(ExportCounts) / 4 * kExportSlots)) != hipSuccess) return hip_fail(c, "alloc export counters", e);
    // a host target's planes are staged in the output buffer: colour first, then depth
    const size_t n_planes = (color_out ? 1u : 0u) + (depth_out ? 1u : 0u);
    if (!out_is_device && n_planes && (e = c->out.ensure(npix * n_planes)) != hipSuccess) return hip_fail(c, "alloc output", e);
    aic_ctx::FrameSlot &fs = c->slots[0];
    uint32_t *const staged_color = c->out.p, *const staged_depth = (!out_is_device && color_out && depth_out) ? c->out.p + npix : c->out.p;
    ExportParams ep;
    ep.src = (const uint2 *)src;
    ep.src_width = d->src_width;
    ep.src_height = d->src_height;
    ep.out_width = d->out_width;
    ep.out_height = d->out_height;
    ep.color = !color_out ? nullptr : (out_is_device ? (uint32_t *)color_out : staged_color);
    ep.depth = !depth_out ? nullptr : (out_is_device ? depth_out : (float *)staged_depth);
    std::memcpy(ep.ipzw, d->inverse_projection_zw, sizeof(ep.ipzw));
    ep.srgb_thr = c->srgb_thr.p;
    ep.counts = (ExportCounts *)c->export_counts.p;
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));
    if ((e = launch_export(ep, fs.stream)) != hipSuccess) return hip_fail(c, "launch export", e);
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    ExportCounts counts[kExportSlots];
    HIP_TRY(c, hipMemcpyAsync(counts, ep.counts, sizeof(counts), hipMemcpyDeviceToHost, fs.stream));
    if (!out_is_device && color_out) HIP_TRY(c, hipMemcpyAsync(color_out, staged_color, plane_bytes, hipMemcpyDeviceToHost, fs.stream));
    if (!out_is_device && depth_out) HIP_TRY(c, hipMemcpyAsync(depth_out, staged_depth, plane_bytes, hipMemcpyDeviceToHost, fs.stream));
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    if (info) {
        HIP_TRY(c, hipEventElapsedTime(&info->kernel_ms, fs.ev0, fs.ev1));
        uint32_t min_bits = 0xffffffffu, max_bits = 0u;
        for (const ExportCounts &slot : counts) {
            info->n_surface += slot.n_surface;
            min_bits = slot.min_bits < min_bits ? slot.min_bits : min_bits;
            max_bits = slot.max_bits > max_bits ? slot.max_bits : max_bits;
        }
        if (info->n_surface) {
            std::memcpy(&info->depth_min, &min_bits, 4);
            std::memcpy(&info->depth_max, &max_bits, 4);
        }
    }
    return AIC_OK;
}

}  // extern "C"
