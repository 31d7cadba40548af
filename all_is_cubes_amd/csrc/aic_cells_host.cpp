// aic_cells_host.cpp -- the host side of the terminal's character cells (include/aic_hip.h "Terminal frames"): the two calls that need no
// context -- aic_cells_geometry (TerminalOptions::viewport_from_terminal_size, all-is-cubes-desktop/src/terminal/options.rs:25-38) and aic_cells_ansi
// (TerminalWindow::write_frame with write_colored_and_measure, terminal/ui.rs:300-360, terminal/chars.rs:205-296, as a byte stream) -- and the context's
// side of the cells kernel (aic_cells.hip): aic_image_cells and aic_render_cells. A translation unit of its own, so that the first two load and run on a
// machine without a GPU; with -DAIC_CELLS_HOST_ONLY it is those two alone and needs no HIP header (a plain C++ compiler builds it for a sanitizer run).

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/aic_hip.h"

namespace {

// rays per character (CharacterMode::rays_per_character, options.rs:177-184); false: not a CharacterMode
bool rays_per_character(int32_t characters, uint32_t *rx, uint32_t *ry) {
    switch (characters) {
        case AIC_CELLS_NAMES: case AIC_CELLS_SHADES: *rx = 1u; *ry = 1u; return true;
        case AIC_CELLS_SPLIT: case AIC_CELLS_SHAPES: *rx = 1u; *ry = 2u; return true;
        case AIC_CELLS_BRAILLE: *rx = 2u; *ry = 4u; return true;
        default: return false;
    }
}

// What aic_cells_ansi writes, counted whether or not it is stored: the stream is made twice, first to measure
struct Sink {
    char *out;
    uint64_t capacity, length = 0;
    void put(const char *s, size_t n) {
        if (out && length + n <= capacity) std::memcpy(out + length, s, n);
        length += n;
    }
    void put(const char *s) { put(s, std::strlen(s)); }
};

// one colour of a pair as SGR parameters; false: kind 0, nothing to write
bool sgr(uint32_t word, bool foreground, char *buf, size_t cap) {
    const uint32_t kind = word >> 24, payload = word & 0xffffffu;
    switch (kind) {
        case AIC_CELL_COLOR_RESET: std::snprintf(buf, cap, "%s", foreground ? "39" : "49"); return true;
        case AIC_CELL_COLOR_BLACK: std::snprintf(buf, cap, "%s;5;0", foreground ? "38" : "48"); return true;
        case AIC_CELL_COLOR_ANSI: std::snprintf(buf, cap, "%s;5;%u", foreground ? "38" : "48", payload & 0xffu); return true;
        case AIC_CELL_COLOR_RGB:
            std::snprintf(buf, cap, "%s;2;%u;%u;%u", foreground ? "38" : "48", (payload >> 16) & 0xffu, (payload >> 8) & 0xffu, payload & 0xffu);
            return true;
        default: return false;
    }
}

// `char::encode_utf8`; a value that is no scalar (a surrogate, above U+10FFFF) is written as U+FFFD
size_t encode_utf8(uint32_t v, char out[4]) {
    if ((v >= 0xd800u && v <= 0xdfffu) || v > 0x10ffffu) v = 0xfffdu;
    if (v < 0x80u) { out[0] = (char)v; return 1; }
    if (v < 0x800u) { out[0] = (char)(0xc0u | (v >> 6)); out[1] = (char)(0x80u | (v & 0x3fu)); return 2; }
    if (v < 0x10000u) { out[0] = (char)(0xe0u | (v >> 12)); out[1] = (char)(0x80u | ((v >> 6) & 0x3fu)); out[2] = (char)(0x80u | (v & 0x3fu)); return 3; }
    out[0] = (char)(0xf0u | (v >> 18)); out[1] = (char)(0x80u | ((v >> 12) & 0x3fu)); out[2] = (char)(0x80u | ((v >> 6) & 0x3fu)); out[3] = (char)(0x80u | (v & 0x3fu));
    return 4;
}

void write_stream(Sink &s, const aic_cell *cells, uint32_t cols, uint32_t rows, const aic_cells_text *text, bool in_rect) {
    char buf[64], fg[24], bg[24];
    s.put("\x1b[?25l");  // cursor::Hide
    s.put("\x1b[0m");    // SetAttribute(Attribute::Reset)
    bool have_color = false;  // current_color: Option<Colors>; in a rectangle it lives on from row to row
    uint32_t cur_fg = 0u, cur_bg = 0u;
    for (uint32_t y = 0; y < rows; y++) {
        if (in_rect) {  // MoveTo(rect.x, rect.y + y), one-based on the wire
            const uint32_t ox = text ? text->origin[0] : 0u, oy = text ? text->origin[1] : 0u;
            std::snprintf(buf, sizeof(buf), "\x1b[%u;%uH", oy + y + 1u, ox + 1u);
            s.put(buf);
        }
        uint32_t x = 0;
        while (x < cols) {
            const aic_cell &c = cells[(size_t)y * cols + x];
            if (!have_color || c.fg != cur_fg || c.bg != cur_bg) {
                have_color = true;
                cur_fg = c.fg;
                cur_bg = c.bg;
                const bool f = sgr(c.fg, true, fg, sizeof(fg)), b = sgr(c.bg, false, bg, sizeof(bg));
                if (f || b) {  // SetColors: both in one escape when both are present
                    std::snprintf(buf, sizeof(buf), "\x1b[%s%s%sm", f ? fg : "", (f && b) ? ";" : "", b ? bg : "");
                    s.put(buf);
                }
            }
            const char *str = nullptr;
            size_t len = 0;
            uint32_t width = 1u;
            char utf8[4];
            if (c.glyph & AIC_CELL_GLYPH_BLOCK) {
                const uint32_t layer = (c.glyph >> 16) & 0x7fffu, index = c.glyph & 0xffffu;
                if (text && layer < 2u && text->names[layer] && index < text->n_names[layer] && text->names[layer][index]) {
                    str = text->names[layer][index];
                    len = std::strlen(str);
                    if (text->widths[layer]) width = text->widths[layer][index];
                } else { str = "#"; len = 1; }
            } else { len = encode_utf8(c.glyph, utf8); str = utf8; }
            if (width <= cols - x) s.put(str, len);
            x += width > 1u ? width : 1u;  // max(1) prevents infinite looping in edge case
        }
        if (!in_rect) {  // don't colorize the rest of the line
            have_color = false;
            s.put("\x1b[0m");
            s.put("\r\n");
        }
    }
    s.put("\x1b[0m");
}

}  // namespace

extern "C" {

int aic_cells_geometry(uint32_t cols, uint32_t rows, int32_t characters, uint32_t *width, uint32_t *height, double nominal[2]) {
    uint32_t rx, ry;
    if (cols > 65535u || rows > 65535u || !rays_per_character(characters, &rx, &ry)) return AIC_ERR_INVALID;
    // max(1) is to keep the projection math from blowing up (options.rs:26-28)
    const uint32_t c = cols ? cols : 1u, r = rows ? rows : 1u;
    if (width) *width = c * rx;
    if (height) *height = r * ry;
    if (nominal) { nominal[0] = (double)c * 0.5; nominal[1] = (double)r * 1.0; }
    return AIC_OK;
}

int aic_cells_ansi(const aic_cell *cells, uint32_t cols, uint32_t rows, const aic_cells_text *text, uint32_t flags, char *out, uint64_t capacity,
                   uint64_t *length) {
    if (!length || (flags & ~AIC_CELLS_ANSI_IN_RECT) || (!out && capacity) || (!cells && (uint64_t)cols * rows > 0)) return AIC_ERR_INVALID;
    const bool in_rect = (flags & AIC_CELLS_ANSI_IN_RECT) != 0;
    Sink measure{nullptr, 0};
    write_stream(measure, cells, cols, rows, text, in_rect);
    *length = measure.length;
    if (measure.length > capacity) return AIC_ERR_INVALID;
    Sink store{out, capacity};
    write_stream(store, cells, cols, rows, text, in_rect);
    return AIC_OK;
}

}  // extern "C"

#ifndef AIC_CELLS_HOST_ONLY

#include <hip/hip_runtime.h>

#include "aic_cells.h"
#include "aic_ctx.h"

using namespace aic;

static_assert(sizeof(aic_cell) == 12, "the kernel writes three words a cell");
static_assert(sizeof(DevAux) == sizeof(aic_pixel_aux) && offsetof(DevAux, cubes_traced) == offsetof(aic_pixel_aux, cubes_traced) && offsetof(DevAux, layer) == offsetof(aic_pixel_aux, layer),
              "the cells kernel reads the trace kernels' records as aic_pixel_aux");
static_assert(sizeof(aic_cells_info) == 18 * 4 && offsetof(aic_cells_info, n_full) == 4 && offsetof(aic_cells_info, n_rgb) == 4 * CELLS_COUNTS,
              "the counters are copied into aic_cells_info from n_full on");

namespace {

constexpr size_t kCountBytes = 64;  // CELLS_COUNTS words, and the staged buffers behind them stay 16-byte aligned
static_assert(CELLS_COUNTS * 4 <= kCountBytes, "the counters fit their slot");

struct CellsGeom {
    uint32_t cols, rows, width, height;
    size_t npix() const { return (size_t)width * height; }
    size_t ncells() const { return (size_t)cols * rows; }
};

// what both entry points reject of a desc, under the entry point's name; 0: fine, and g is the raised grid and its framebuffer
int cells_desc_invalid(aic_ctx *c, const char *who, const aic_cells_desc *d, CellsGeom *g) {
    uint32_t rx, ry;
    if (!rays_per_character(d->characters, &rx, &ry)) return reject(c, who, "characters is no CharacterMode (0..4)");
    if (d->colors < AIC_CELLS_COLOR_NONE || d->colors > AIC_CELLS_COLOR_RGB) return reject(c, who, "colors is no ColorMode (0..2)");
    if (d->cols > 65535u || d->rows > 65535u) return reject(c, who, "cols or rows above 65535");
    g->cols = d->cols ? d->cols : 1u;
    g->rows = d->rows ? d->rows : 1u;
    g->width = g->cols * rx;
    g->height = g->rows * ry;
    return 0;
}

// The cells kernel behind whatever the stream holds, its counters and (to_host) its cells read back: one synchronise. p.out and p.counts are set here.
int run_cells(aic_ctx *c, const char *who, CellsParams &p, aic_cell *out, bool out_is_device, aic_cells_info *info) {
    aic_ctx::FrameSlot &fs = c->slots[0];
    const size_t ncells = (size_t)p.cols * p.rows;
    p.counts = (uint32_t *)c->cells_scratch.p;
    p.srgb_buckets = c->srgb_buckets.p;
    HIP_TRY(c, hipMemsetAsync(p.counts, 0, kCountBytes, fs.stream));
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));
    const hipError_t e = launch_cells(p, fs.stream);
    if (e != hipSuccess) return hip_fail(c, who, e);
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    uint32_t counts[CELLS_COUNTS];
    HIP_TRY(c, hipMemcpyAsync(counts, p.counts, sizeof(counts), hipMemcpyDeviceToHost, fs.stream));
    if (!out_is_device) HIP_TRY(c, hipMemcpyAsync(out, p.out, ncells * sizeof(aic_cell), hipMemcpyDeviceToHost, fs.stream));
    HIP_TRY(c, hipStreamSynchronize(fs.stream));
    if (info) {
        info->n_cells = (uint32_t)ncells;
        std::memcpy(&info->n_full, counts, sizeof(counts));
        HIP_TRY(c, hipEventElapsedTime(&info->kernel_ms, fs.ev0, fs.ev1));
    }
    return AIC_OK;
}

}  // namespace

extern "C" {

int aic_image_cells(aic_ctx *c, const aic_cells_desc *d, const void *image, const aic_pixel_aux *aux, aic_cell *out, aic_cells_info *info) {
    const char *const who = "aic_image_cells";
    if (!c || !d || !image || !out) return fail(c, AIC_ERR_INVALID, "aic_image_cells: bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    CellsGeom g;
    if (const int rc = cells_desc_invalid(c, who, d, &g)) return rc;
    if (d->flags & ~(AIC_CELLS_IMAGE_DEVICE | AIC_CELLS_OUT_DEVICE | AIC_CELLS_IMAGE_F16 | AIC_CELLS_POSTPROCESSED)) return reject(c, who, "unknown flag bits");
    if (d->tone_mapping != 0 && d->tone_mapping != 1) return reject(c, who, "tone_mapping is neither 0 (Clamp) nor 1 (Reinhard)");
    if (!(d->exposure >= 0.f)) return reject(c, who, "exposure is NaN or negative");
    if (!(d->maximum_intensity >= 0.f)) return reject(c, who, "maximum_intensity is NaN or negative");
    if (d->characters == AIC_CELLS_NAMES && !aux) return reject(c, who, "Names needs the first-hit records");
    const bool f16 = (d->flags & AIC_CELLS_IMAGE_F16) != 0, image_device = (d->flags & AIC_CELLS_IMAGE_DEVICE) != 0, out_device = (d->flags & AIC_CELLS_OUT_DEVICE) != 0;
    if (image_device && ((((uintptr_t)image) & (f16 ? 7u : 15u)) || (((uintptr_t)aux) & 7u))) return reject(c, who, "a device image starts at its pixel's boundary (16 bytes, f16: 8) and device records at an 8-byte boundary");
    if (out_device && (((uintptr_t)out) & 3u)) return reject(c, who, "a device out starts at a 4-byte boundary");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->slots[0].busy) return reject(c, who, "a submitted frame still occupies slot 0 (aic_render_wait it first)");
    // the scratch: counters | staged image | staged records | staged cells, each part at a 16-byte boundary
    const size_t image_bytes = g.npix() * (f16 ? 8 : 16), aux_bytes = aux ? g.npix() * sizeof(aic_pixel_aux) : 0, out_bytes = g.ncells() * sizeof(aic_cell);
    auto pad = [](size_t n) { return (n + 15u) & ~(size_t)15u; };
    const size_t off_image = kCountBytes, off_aux = off_image + (image_device ? 0 : pad(image_bytes)), off_out = off_aux + (image_device ? 0 : pad(aux_bytes));
    if (const hipError_t e = c->cells_scratch.ensure(off_out + (out_device ? 0 : pad(out_bytes)))) return hip_fail(c, "alloc cells scratch", e);
    unsigned char *const s = c->cells_scratch.p;
    hipStream_t stream = c->slots[0].stream;
    if (!image_device) {
        HIP_TRY(c, hipMemcpyAsync(s + off_image, image, image_bytes, hipMemcpyHostToDevice, stream));
        if (aux) HIP_TRY(c, hipMemcpyAsync(s + off_aux, aux, aux_bytes, hipMemcpyHostToDevice, stream));
    }
    CellsParams p = {};
    p.image = image_device ? image : (const void *)(s + off_image);
    p.aux = !aux ? nullptr : (image_device ? aux : (const aic_pixel_aux *)(s + off_aux));
    p.out = out_device ? (uint32_t *)out : (uint32_t *)(s + off_out);
    p.cols = g.cols; p.rows = g.rows; p.width = g.width;
    p.characters = d->characters; p.colors = d->colors;
    p.f16 = f16; p.postprocessed = (d->flags & AIC_CELLS_POSTPROCESSED) != 0;
    p.exposure = d->exposure + 0.0f;  // (a PositiveSign never holds -0.0)
    p.tone_mapping = d->tone_mapping; p.maximum_intensity = d->maximum_intensity;
    return run_cells(c, who, p, out, out_device, info);
}

int aic_render_cells(aic_ctx *c, const aic_frame_desc *f, const aic_cells_desc *d, aic_cell *out, int out_is_device, aic_frame_info *frame_info,
                     aic_cells_info *cells_info) {
    const char *const who = "aic_render_cells";
    if (!c || !f || !d || !out) return fail(c, AIC_ERR_INVALID, "aic_render_cells: bad argument");
    if (frame_info) std::memset(frame_info, 0, sizeof(*frame_info));
    if (cells_info) std::memset(cells_info, 0, sizeof(*cells_info));
    CellsGeom g;
    if (const int rc = cells_desc_invalid(c, who, d, &g)) return rc;
    if (d->flags) return reject(c, who, "desc.flags must be 0 (out_is_device says where the cells go)");
    if (f->width != g.width || f->height != g.height) return reject(c, who, "the frame's size is not aic_cells_geometry's of the desc");
    if (f->flags & (AIC_FRAME_AUX | AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF | AIC_FRAME_OUT_SPLIT)) return reject(c, who, "the frame's output is the library's choice: no output flag");
    if (f->flags & AIC_FRAME_BLOOM) return fail(c, AIC_ERR_UNSUPPORTED, "aic_render_cells: AIC_FRAME_BLOOM is not supported");
    if (f->partition.n_parts > 1u && f->partition.strip_rows != 0u) return fail(c, AIC_ERR_UNSUPPORTED, "aic_render_cells: cells need the whole frame (partition.n_parts = 1)");
    if (out_is_device && (((uintptr_t)out) & 3u)) return reject(c, who, "a device out starts at a 4-byte boundary");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->slots[0].busy) return reject(c, who, "a submitted frame still occupies slot 0 (aic_render_wait it first)");
    hipError_t e;
    if ((e = c->cells_frame.ensure(g.npix())) != hipSuccess) return hip_fail(c, "alloc cells frame", e);
    auto pad = [](size_t n) { return (n + 15u) & ~(size_t)15u; };
    if ((e = c->cells_scratch.ensure(kCountBytes + (out_is_device ? 0 : pad(g.ncells() * sizeof(aic_cell))))) != hipSuccess) return hip_fail(c, "alloc cells scratch", e);
    // the frame, as aic_render traces it: the linear colour into cells_frame, the first-hit records into the context's own buffer
    aic_frame_desc traced = *f;
    traced.flags |= AIC_FRAME_OUT_LINEAR | AIC_FRAME_AUX;
    if (const int rc = aic_render(c, &traced, c->cells_frame.p, 1, frame_info)) return rc;
    if (c->aux_records != g.npix()) return fail(c, AIC_ERR_DEVICE, "aic_render_cells: the frame left no first-hit records");
    // post_process_color with the WORLD camera for every pixel (terminal.rs:120-123)
    const Layer &world = c->layers[AIC_LAYER_WORLD];
    const aic_options opt = world.opt_set ? world.opt : default_options();
    CellsParams p = {};
    p.image = c->cells_frame.p;
    p.aux = reinterpret_cast<const aic_pixel_aux *>(c->aux.p);
    p.out = out_is_device ? (uint32_t *)out : (uint32_t *)(c->cells_scratch.p + kCountBytes);
    p.cols = g.cols; p.rows = g.rows; p.width = g.width;
    p.characters = d->characters; p.colors = d->colors;
    p.exposure = f->world.exposure + 0.0f;
    p.tone_mapping = opt.tone_mapping; p.maximum_intensity = opt.maximum_intensity;
    return run_cells(c, who, p, out, out_is_device != 0, cells_info);
}

}  // extern "C"

#endif  // AIC_CELLS_HOST_ONLY
