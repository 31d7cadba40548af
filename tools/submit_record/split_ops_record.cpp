// split_ops_record.cpp -- drives the operations on a resident Split frame (csrc/aic_split_ops.cpp: aic_reproject_split, aic_pick_pixels,
// aic_present_split, aic_present_split_lines, aic_present_split_text with aic_set_text_font, aic_export_split, and their size queries and host-only helpers) through a fixed list of scenarios against the recording fake (fake_hip.cpp) and
// prints the record: every runtime call and launch with its arguments, each call's return code and message, every field of its info structs and what
// the context keeps for these operations afterwards. Two builds of the host code make the same calls exactly when their records are byte-identical
// (build.sh, tests/test_split_ops_record_cpu.py). A scenario named "reject: ..." is one refused call on a context an earlier scenario made; every
// other scenario starts with ordinals from zero and frees what it allocates.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "aic_ctx.h"
#include "record.h"

namespace {

int n_scenarios = 0;

void *dev(size_t bytes) {  // a caller's device buffer
    void *p = nullptr;
    (void)hipMalloc(&p, bytes ? bytes : 1);
    return p;
}

// a context with driver.cpp's 8 x 8 x 8 world (aic_render_submit needs one to occupy slot 0); AIC_LINES_CLEAR_KEYS is read when the context is made
aic_ctx *make_ctx(bool lines_clear_keys = false) {
    if (lines_clear_keys) setenv("AIC_LINES_CLEAR_KEYS", "1", 1); else unsetenv("AIC_LINES_CLEAR_KEYS");
    int st = 0;
    aic_ctx *c = aic_create(0, &st);
    unsetenv("AIC_LINES_CLEAR_KEYS");
    static const std::vector<uint16_t> cubes(512, 1);
    static const std::vector<uint8_t> light(512 * 4, 0);
    static const float palette[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.5f, 0.5f, 1.f, 0, 0, 0, 0};
    static const uint16_t voxels[1] = {0};
    aic_block_desc blocks[2];
    std::memset(blocks, 0, sizeof(blocks));
    for (int i = 0; i < 2; i++) { blocks[i].resolution = 1; blocks[i].pal_off = (uint32_t)i; blocks[i].pal_len = 1; blocks[i].flags = AIC_BLOCK_ONE | (i ? 0u : AIC_BLOCK_AIR); }
    aic_space_desc s;
    std::memset(&s, 0, sizeof(s));
    s.size[0] = s.size[1] = s.size[2] = 8;
    s.block_index = cubes.data(); s.light = light.data(); s.n_blocks = 2; s.blocks = blocks; s.voxels = voxels; s.n_voxels = 1; s.palette = palette; s.n_palette = 2;
    if (aic_upload_space(c, 0, &s) != AIC_OK) rec("aic_upload_space FAILED : %s", aic_last_error(c));
    return c;
}

void submit_to_slot0(aic_ctx *c, void *out) {  // out: 8 x 8 x 4 bytes on the device
    aic_frame_desc f;
    std::memset(&f, 0, sizeof(f));
    f.width = f.height = 8;
    for (int i = 0; i < 4; i++) f.world.inverse_projection_view[5 * i] = f.ui.inverse_projection_view[5 * i] = 1.0;
    f.world.exposure = f.ui.exposure = 1.f;
    if (aic_render_submit(c, &f, out, 0) != AIC_OK) rec("aic_render_submit FAILED : %s", aic_last_error(c));
}

aic_reproject_desc reproject_desc(uint32_t w, uint32_t h, uint32_t flags = 0) {
    aic_reproject_desc d;
    std::memset(&d, 0, sizeof(d));
    d.width = w; d.height = h; d.flags = flags;
    for (int i = 0; i < 16; i++) d.reprojection[i] = i % 5 ? 0.03125f * i : 1.f;
    d.inverse_projection_zw[0] = 0.25f; d.inverse_projection_zw[1] = -1.f; d.inverse_projection_zw[2] = 1.f; d.inverse_projection_zw[3] = 0.5f;
    return d;
}
aic_pick_desc pick_desc(uint32_t w, uint32_t h, uint32_t n, uint32_t max_unknown = 0, uint32_t flags = 0) {
    aic_pick_desc d;
    std::memset(&d, 0, sizeof(d));
    d.width = w; d.height = h; d.n = n; d.max_unknown = max_unknown; d.flags = flags;
    d.skip_unknown = 3; d.cursor = (1ull << 40) + 7;
    return d;
}
aic_present_desc present_desc(uint32_t sw, uint32_t sh, uint32_t ow, uint32_t oh, float bloom = 0.f, uint32_t flags = 0) {
    aic_present_desc d;
    std::memset(&d, 0, sizeof(d));
    d.src_width = sw; d.src_height = sh; d.out_width = ow; d.out_height = oh;
    d.bloom_intensity = bloom; d.tone_mapping = 1; d.maximum_intensity = 2.5f; d.flags = flags;
    return d;
}
aic_lines_desc lines_desc(const aic_line_vertex *v, uint32_t n, uint32_t flags = 0) {
    aic_lines_desc l;
    std::memset(&l, 0, sizeof(l));
    for (int i = 0; i < 16; i++) l.view_projection[i] = i % 5 ? -0.0625f * i : 1.f;
    l.vertices = v; l.n_lines = n; l.flags = flags;
    return l;
}

aic_export_desc export_desc(uint32_t sw, uint32_t sh, uint32_t ow, uint32_t oh, uint32_t flags = 0) {
    aic_export_desc d;
    std::memset(&d, 0, sizeof(d));
    d.src_width = sw; d.src_height = sh; d.out_width = ow; d.out_height = oh; d.flags = flags;
    d.inverse_projection_zw[0] = 0.25f; d.inverse_projection_zw[1] = -1.f; d.inverse_projection_zw[2] = 1.f; d.inverse_projection_zw[3] = 0.5f;
    return d;
}

// ---- what is recorded after every call
void rec_state(const aic_ctx *c) {
    if (!c) return;
    rec("  state reproject_valid %ux%u lines_keys_clean %zu reproject_scratch %zu/%zu pick_scratch %zu/%zu present_scratch %zu/%zu lines_scratch %zu/%zu out %zu/%zu slot0_busy %d",
        c->reproject_valid_w, c->reproject_valid_h, c->lines_keys_clean, c->reproject_scratch.n, c->reproject_scratch.cap, c->pick_scratch.n, c->pick_scratch.cap, c->present_scratch.n,
        c->present_scratch.cap, c->lines_scratch.n, c->lines_scratch.cap, c->out.n, c->out.cap, (int)c->slots[0].busy);
}
void rec_rc(const aic_ctx *c, const char *call, int rc) { rec("%s rc %d%s%s", call, rc, rc ? " : " : "", rc ? aic_last_error(c) : ""); }

// Every info struct is handed over filled with 0xff bytes, so that a field the call leaves alone shows as such.
int reproject(aic_ctx *c, const aic_reproject_desc *d, const void *src, void *dst, bool want_info = true) {
    aic_reproject_info i;
    std::memset(&i, 0xff, sizeof(i));
    const int rc = aic_reproject_split(c, d, src, dst, want_info ? &i : nullptr);
    rec_rc(c, "aic_reproject_split", rc);
    rec("  info splats %llu dropped %llu gaps %llu unfilled %llu kernel_ms %a levels %u t0 %u %u", (unsigned long long)i.n_splats, (unsigned long long)i.n_dropped,
        (unsigned long long)i.n_gaps, (unsigned long long)i.n_unfilled, i.kernel_ms, i.levels, i.t0[0], i.t0[1]);
    rec_state(c);
    return rc;
}
int pick(aic_ctx *c, const aic_pick_desc *d, const uint32_t *order, uint32_t *out, bool want_info = true) {
    aic_pick_info i;
    std::memset(&i, 0xff, sizeof(i));
    const int rc = aic_pick_pixels(c, d, order, out, want_info ? &i : nullptr);
    rec_rc(c, "aic_pick_pixels", rc);
    rec("  info unknown %llu next_cursor %llu from_unknown %u from_order %u kernel_ms %a reserved %u", (unsigned long long)i.n_unknown, (unsigned long long)i.next_cursor, i.n_from_unknown,
        i.n_from_order, i.kernel_ms, i.reserved);
    rec_state(c);
    return rc;
}
// through_lines: aic_present_split_lines with `ld` (which may be NULL); else aic_present_split
int present(aic_ctx *c, const aic_present_desc *d, bool through_lines, const aic_lines_desc *ld, const void *src, void *out, int out_is_device, bool want_info = true) {
    aic_present_info i;
    aic_lines_info li;
    std::memset(&i, 0xff, sizeof(i));
    std::memset(&li, 0xff, sizeof(li));
    const int rc = through_lines ? aic_present_split_lines(c, d, ld, src, out, out_is_device, want_info ? &i : nullptr, want_info ? &li : nullptr)
                                 : aic_present_split(c, d, src, out, out_is_device, want_info ? &i : nullptr);
    rec_rc(c, through_lines ? "aic_present_split_lines" : "aic_present_split", rc);
    rec("  info kernel_ms %a levels %u t0 %u %u bloomed %u reserved %u %u %u", i.kernel_ms, i.levels, i.t0[0], i.t0[1], i.bloomed, i.reserved[0], i.reserved[1], i.reserved[2]);
    if (through_lines)
        rec("  lines_info clipped_away %llu fragments %llu passed %llu pixels %llu", (unsigned long long)li.n_clipped_away, (unsigned long long)li.n_fragments,
            (unsigned long long)li.n_passed, (unsigned long long)li.n_pixels);
    rec_state(c);
    return rc;
}

// aic_export_split; the counters' state is recorded on a line of its own, so that rec_state's stays what it was
int export_split(aic_ctx *c, const aic_export_desc *d, const void *src, void *color, float *depth, int out_is_device, bool want_info = true) {
    aic_export_info i;
    std::memset(&i, 0xff, sizeof(i));
    const int rc = aic_export_split(c, d, src, color, depth, out_is_device, want_info ? &i : nullptr);
    rec_rc(c, "aic_export_split", rc);
    rec("  info kernel_ms %a n_surface %u depth_min %a depth_max %a reserved %u %u %u %u", i.kernel_ms, i.n_surface, i.depth_min, i.depth_max, i.reserved[0], i.reserved[1], i.reserved[2],
        i.reserved[3]);
    rec_state(c);
    if (c) rec("  export state counts %zu/%zu", c->export_counts.n, c->export_counts.cap);
    return rc;
}

// aic_present_split_text with `ld` and `td` (either may be NULL); the text state is recorded on a line of its own, so that rec_state's stays what it was
void rec_text_state(const aic_ctx *c) {
    if (!c) return;
    rec("  text state atlas %zu/%zu cell %ux%u margin %u space_blank %d codes %zu/%zu", c->text_atlas.n, c->text_atlas.cap, c->text_cell_w, c->text_cell_h, c->text_margin,
        (int)c->text_space_blank, c->text_codes.n, c->text_codes.cap);
}
int present_text(aic_ctx *c, const aic_present_desc *d, const aic_lines_desc *ld, const aic_text_desc *td, const void *src, void *out, int out_is_device, bool want_info = true) {
    aic_present_info i;
    aic_lines_info li;
    std::memset(&i, 0xff, sizeof(i));
    std::memset(&li, 0xff, sizeof(li));
    const int rc = aic_present_split_text(c, d, ld, td, src, out, out_is_device, want_info ? &i : nullptr, want_info ? &li : nullptr);
    rec_rc(c, "aic_present_split_text", rc);
    rec("  info kernel_ms %a levels %u t0 %u %u bloomed %u reserved %u %u %u", i.kernel_ms, i.levels, i.t0[0], i.t0[1], i.bloomed, i.reserved[0], i.reserved[1], i.reserved[2]);
    rec("  lines_info clipped_away %llu fragments %llu passed %llu pixels %llu", (unsigned long long)li.n_clipped_away, (unsigned long long)li.n_fragments,
        (unsigned long long)li.n_passed, (unsigned long long)li.n_pixels);
    rec_state(c);
    rec_text_state(c);
    return rc;
}
int set_font(aic_ctx *c, const uint8_t *atlas, uint32_t cw, uint32_t ch, uint32_t margin) {
    const int rc = aic_set_text_font(c, atlas, cw, ch, margin);
    rec_rc(c, "aic_set_text_font", rc);
    rec_text_state(c);
    return rc;
}
// a (9, 18, 1) atlas with every cell but 0x20 (blank_space) or every cell filled; an 8 x 3 grid of codes with "ab" and "c" in its first two rows
std::vector<uint8_t> atlas_9x18(bool blank_space) {
    std::vector<uint8_t> a(16 * 18 * 16 * 9 * 4, 0x80);
    if (blank_space)
        for (int y = 0; y < 18; y++) std::memset(&a[((size_t)(2 * 18 + y) * 16 * 9) * 4], 0, 9 * 4);
    return a;
}
aic_text_desc text_desc(const uint8_t *codes, uint32_t flags = 0) {
    aic_text_desc t;
    std::memset(&t, 0, sizeof(t));
    t.scale[0] = 0.875f; t.scale[1] = 0.75f; t.origin[0] = 0.125f; t.origin[1] = 0.0625f;
    t.cols = 8; t.rows = 3; t.flags = flags; t.codes = codes;
    return t;
}
const uint8_t kCodes[24] = {'a', 'b', 0, 0, 0, 0, 0, 0, 'c', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// one scenario: ordinals from zero, everything it allocates freed at its end -- or (not fresh) one that goes on with what the scenario before left
void scenario(const std::string &name, const std::function<void()> &body, bool fresh = true) {
    if (fresh) fake_reset();
    rec("== %s", name.c_str());
    n_scenarios++;
    body();
}
// one refused call on the context of the scenario before, so that nothing but the call stands between the name and the result
void rejection(const std::string &name, const std::function<void()> &call) { scenario("reject: " + name, call, false); }
std::string str(std::initializer_list<long> v) { std::string s; for (long x : v) s += " " + std::to_string(x); return s; }

const uint32_t kSizes[][2] = {{0, 0}, {1, 1}, {1, 7}, {8, 8}, {33, 17}, {640, 360}};
const uint32_t kPresentShapes[][4] = {{0, 0, 0, 0}, {1, 1, 1, 1}, {1, 7, 1, 7}, {8, 8, 8, 8}, {33, 17, 33, 17}, {640, 360, 640, 360}, {20, 12, 40, 24}, {33, 17, 16, 8}};
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

// ---- shapes
void shapes() {
    for (const auto &wh : kSizes)
        scenario("reproject" + str({wh[0], wh[1]}), [&] {
            aic_ctx *c = make_ctx();
            const size_t bytes = (size_t)wh[0] * wh[1] * 12;
            void *src = dev(bytes), *dst = dev(bytes);
            aic_reproject_desc d = reproject_desc(wh[0], wh[1]);
            reproject(c, &d, src, dst);
            d = reproject_desc(wh[0], wh[1], AIC_REPROJECT_KEEP_SPLATS);
            reproject(c, &d, src, dst);         // (finds its scratch)
            reproject(c, &d, dst, src, false);  // (no info)
            (void)hipFree(src); (void)hipFree(dst);
            aic_destroy(c);
        });
    for (const auto &wh : kSizes)
        scenario("pick" + str({wh[0], wh[1]}), [&] {
            aic_ctx *c = make_ctx();
            const size_t count = (size_t)wh[0] * wh[1];
            const uint32_t n = count ? (uint32_t)(count < 100 ? count + 3 : 100) : 0u;
            void *src = dev(count * 12), *dst = dev(count * 12);
            uint32_t *order = (uint32_t *)dev(count * 4), *out = (uint32_t *)dev((size_t)n * 4);
            aic_pick_desc d = pick_desc(wh[0], wh[1], n);
            pick(c, &d, order, out);
            const aic_reproject_desc rd = reproject_desc(wh[0], wh[1]);
            reproject(c, &rd, src, dst);
            d = pick_desc(wh[0], wh[1], n, n / 2 + 1);
            pick(c, &d, order, out);
            pick(c, &d, nullptr, out);  // (row-major; finds its scratch)
            for (void *p : {src, dst, (void *)order, (void *)out}) (void)hipFree(p);
            aic_destroy(c);
        });
    // form 0: aic_present_split; 1: aic_present_split_lines with a list of no lines; 2: with no list. The three record the same calls.
    for (const auto &s : kPresentShapes)
        for (float bloom : {0.f, 0.125f})
            for (uint32_t flags : {0u, (uint32_t)AIC_PRESENT_OUT_F16})
                for (int to_device = 0; to_device < 2; to_device++)
                    for (int form = 0; form < 3; form++)
                        scenario("present" + str({s[0], s[1], s[2], s[3], (long)(bloom * 1000), flags, to_device, form}), [&] {
                            aic_ctx *c = make_ctx();
                            const size_t out_bytes = (size_t)s[2] * s[3] * (flags ? 8 : 4);
                            void *src = dev((size_t)s[0] * s[1] * 12), *out = to_device ? dev(out_bytes) : std::malloc(out_bytes + 1);
                            const aic_present_desc d = present_desc(s[0], s[1], s[2], s[3], bloom, flags);
                            const aic_lines_desc none = lines_desc(nullptr, 0);
                            for (int n = 0; n < 2; n++) present(c, &d, form != 0, form == 1 ? &none : nullptr, src, out, to_device);  // (the second finds its scratch)
                            (void)hipFree(src);
                            if (to_device) (void)hipFree(out); else std::free(out);
                            aic_destroy(c);
                        });
}

// ---- export: equal, larger, smaller and empty outputs; both planes, one, none (the info alone); to the host and to the device; with and without info
const uint32_t kExportShapes[][4] = {{0, 0, 0, 0}, {8, 8, 0, 8}, {1, 1, 1, 1}, {1, 7, 1, 7}, {33, 17, 33, 17}, {640, 360, 640, 360}, {20, 12, 40, 24}, {33, 17, 16, 8}, {1, 1, 5, 3}};
void exports() {
    for (const auto &s : kExportShapes)
        for (int planes = 0; planes < 4; planes++)  // bit 0: colour, bit 1: depth
            for (int to_device = 0; to_device < 2; to_device++)
                scenario("export" + str({s[0], s[1], s[2], s[3], planes, to_device}), [&] {
                    aic_ctx *c = make_ctx();
                    const size_t plane_bytes = (size_t)s[2] * s[3] * 4;
                    void *src = dev((size_t)s[0] * s[1] * 12);
                    void *color = !(planes & 1) ? nullptr : (to_device ? dev(plane_bytes) : std::malloc(plane_bytes + 1));
                    void *depth = !(planes & 2) ? nullptr : (to_device ? dev(plane_bytes) : std::malloc(plane_bytes + 1));
                    const aic_export_desc d = export_desc(s[0], s[1], s[2], s[3]);
                    for (int n = 0; n < 2; n++) export_split(c, &d, src, color, (float *)depth, to_device);  // (the second finds its counters and staging)
                    if (planes) export_split(c, &d, src, color, (float *)depth, to_device, false);         // (no info)
                    (void)hipFree(src);
                    for (void *p : {color, depth})
                        if (p) { if (to_device) (void)hipFree(p); else std::free(p); }
                    aic_destroy(c);
                });
    scenario("export: size policy", [] {
        const uint32_t sizes[][2] = {{640, 480}, {1920, 1080}, {641, 480}, {65535, 65535}, {0, 7}, {7, 0}, {1, 1}};
        for (const auto &wh : sizes)
            for (double cap : {640.0 * 480.0, 1.0, 0.5, (double)kInf}) {
                uint32_t out[2] = {99, 99};
                const int rc = aic_export_size(wh[0], wh[1], cap, out);
                rec("aic_export_size %ux%u cap %a rc %d -> %ux%u", wh[0], wh[1], cap, rc, out[0], out[1]);
            }
        uint32_t out[2];
        rec("aic_export_size invalid rc %d %d %d %d", aic_export_size(8, 8, 64.0, nullptr), aic_export_size(8, 8, 0.0, out), aic_export_size(8, 8, -1.0, out),
            aic_export_size(8, 8, (double)kNaN, out));
    });
}

// ---- lines: a host list and a device list, on a context that resets the keys it touched and on one that clears them all
void lines() {
    static const std::vector<aic_line_vertex> host(2 * 28);
    for (const auto &s : kPresentShapes)
        for (uint32_t n_lines : {1u, 28u})
            for (uint32_t list_flags : {0u, (uint32_t)AIC_LINES_DEVICE})
                for (int clear_keys = 0; clear_keys < 2; clear_keys++)
                    for (float bloom : {0.f, 0.125f})
                        for (uint32_t flags : {0u, (uint32_t)AIC_PRESENT_OUT_F16})
                            for (int to_device = 0; to_device < 2; to_device++)
                                scenario("lines" + str({s[0], s[1], s[2], s[3], n_lines, list_flags, clear_keys, (long)(bloom * 1000), flags, to_device}), [&] {
                                    aic_ctx *c = make_ctx(clear_keys);
                                    const size_t out_bytes = (size_t)s[2] * s[3] * (flags ? 8 : 4);
                                    void *src = dev((size_t)s[0] * s[1] * 12), *out = to_device ? dev(out_bytes) : std::malloc(out_bytes + 1);
                                    aic_line_vertex *on_device = (aic_line_vertex *)dev(2 * 28 * sizeof(aic_line_vertex));
                                    const aic_present_desc d = present_desc(s[0], s[1], s[2], s[3], bloom, flags);
                                    const aic_lines_desc l = lines_desc(list_flags ? on_device : host.data(), n_lines, list_flags);
                                    for (int n = 0; n < 2; n++) present(c, &d, true, &l, src, out, to_device);  // (the second finds its keys clean, or clears them all)
                                    (void)hipFree(src); (void)hipFree(on_device);
                                    if (to_device) (void)hipFree(out); else std::free(out);
                                    aic_destroy(c);
                                });
}

// ---- text: a host list and a device list, with and without lines, a blank and a non-blank space cell; without text the call is aic_present_split_lines
void text() {
    static const std::vector<aic_line_vertex> host(2 * 28);
    for (const auto &s : kPresentShapes)
        for (int blank = 0; blank < 2; blank++)
            for (uint32_t text_flags : {0u, (uint32_t)AIC_TEXT_DEVICE})
                for (uint32_t n_lines : {0u, 28u})
                    for (float bloom : {0.f, 0.125f})
                        for (uint32_t flags : {0u, (uint32_t)AIC_PRESENT_OUT_F16})
                            for (int to_device = 0; to_device < 2; to_device++)
                                scenario("text" + str({s[0], s[1], s[2], s[3], blank, text_flags, n_lines, (long)(bloom * 1000), flags, to_device}), [&] {
                                    aic_ctx *c = make_ctx();
                                    const std::vector<uint8_t> atlas = atlas_9x18(blank != 0);
                                    set_font(c, atlas.data(), 9, 18, 1);
                                    const size_t out_bytes = (size_t)s[2] * s[3] * (flags ? 8 : 4);
                                    void *src = dev((size_t)s[0] * s[1] * 12), *out = to_device ? dev(out_bytes) : std::malloc(out_bytes + 1);
                                    uint8_t *on_device = (uint8_t *)dev(sizeof(kCodes));
                                    const aic_present_desc d = present_desc(s[0], s[1], s[2], s[3], bloom, flags);
                                    const aic_lines_desc l = lines_desc(host.data(), n_lines);
                                    const aic_text_desc t = text_desc(text_flags ? on_device : kCodes, text_flags);
                                    for (int n = 0; n < 2; n++) present_text(c, &d, n_lines ? &l : nullptr, &t, src, out, to_device);  // (the second finds its staging)
                                    (void)hipFree(src); (void)hipFree(on_device);
                                    if (to_device) (void)hipFree(out); else std::free(out);
                                    aic_destroy(c);
                                });
    scenario("text: sequence on one context", [] {
        aic_ctx *c = make_ctx();
        const uint32_t W = 40, H = 24;
        void *src = dev(W * H * 12), *out = dev(W * H * 8);
        const aic_present_desc d = present_desc(W, H, W, H);
        const aic_lines_desc l = lines_desc(host.data(), 28), none = lines_desc(nullptr, 0);
        aic_text_desc t = text_desc(kCodes);
        rec("-- no text: the call is aic_present_split_lines, with lines, with a list of none and with no list");
        present_text(c, &d, &l, nullptr, src, out, 1);
        present_text(c, &d, &none, nullptr, src, out, 1);
        present_text(c, &d, nullptr, nullptr, src, out, 1);
        rec("-- text before any font is refused; then a font, a text, an empty text, a larger grid");
        present_text(c, &d, nullptr, &t, src, out, 1);
        const std::vector<uint8_t> blank = atlas_9x18(true), full = atlas_9x18(false);
        set_font(c, blank.data(), 9, 18, 1);
        present_text(c, &d, nullptr, &t, src, out, 1);
        static const uint8_t zeros[64 * 8] = {0};
        t = text_desc(zeros);
        present_text(c, &d, &none, &t, src, out, 1);
        t.cols = 64; t.rows = 8;
        present_text(c, &d, nullptr, &t, src, out, 1);
        rec("-- the font replaced by a smaller one whose space is not blank, then by a larger one, then dropped");
        set_font(c, full.data(), 3, 3, 1);
        t = text_desc(kCodes);
        present_text(c, &d, nullptr, &t, src, out, 1);
        set_font(c, full.data(), 9, 18, 1);
        set_font(c, nullptr, 0, 0, 0);
        present_text(c, &d, nullptr, &t, src, out, 1);
        rec("-- an empty output with text");
        set_font(c, blank.data(), 9, 18, 1);
        const aic_present_desc e = present_desc(W, H, 0, H);
        present_text(c, &e, nullptr, &t, src, out, 1);
        (void)hipFree(src); (void)hipFree(out);
        aic_destroy(c);
    });
    scenario("text: host-only helpers", [] {
        const double origin_px[2] = {5.0, 5.0};
        const double sizes[][2] = {{1, 1}, {7, 16}, {8, 17}, {640.5, 480.25}, {1920, 1080}, {65535, 1}};
        const uint32_t cells[][3] = {{9, 18, 1}, {5, 7, 0}, {3, 3, 1}};
        for (const auto &n : sizes)
            for (const auto &cell : cells) {
                uint32_t cols = 99, rows = 99;
                float scale[2] = {99.f, 99.f}, origin[2] = {99.f, 99.f};
                const int rc = aic_text_geometry(n[0], n[1], cell[0], cell[1], cell[2], origin_px, &cols, &rows, scale, origin);
                rec("aic_text_geometry %a x %a cell %u %u %u rc %d grid %ux%u scale %a %a origin %a %a", n[0], n[1], cell[0], cell[1], cell[2], rc, cols, rows, scale[0], scale[1], origin[0],
                    origin[1]);
            }
        rec("aic_text_geometry invalid rc %d %d %d %d %d %d %d %d", aic_text_geometry(0, 1, 9, 18, 1, origin_px, nullptr, nullptr, nullptr, nullptr),
            aic_text_geometry(1, -1, 9, 18, 1, origin_px, nullptr, nullptr, nullptr, nullptr), aic_text_geometry(kInf, 1, 9, 18, 1, origin_px, nullptr, nullptr, nullptr, nullptr),
            aic_text_geometry(1, kNaN, 9, 18, 1, origin_px, nullptr, nullptr, nullptr, nullptr), aic_text_geometry(8, 8, 0, 18, 1, origin_px, nullptr, nullptr, nullptr, nullptr),
            aic_text_geometry(8, 8, 9, 1025, 1, origin_px, nullptr, nullptr, nullptr, nullptr), aic_text_geometry(8, 8, 4, 18, 2, origin_px, nullptr, nullptr, nullptr, nullptr),
            aic_text_geometry(65536, 8, 3, 3, 1, origin_px, nullptr, nullptr, nullptr, nullptr));
        const char *texts[] = {"", "\n\n", "a b\nc d", "a line longer than the grid", "1\n2\n3\n4", "\xc3\xa9\xe2\x82\xac", "\xff\xc3"};
        for (const char *text : texts) {
            uint8_t codes[3 * 8];
            uint32_t used[2] = {99, 99};
            const int rc = aic_text_layout(text, std::strlen(text), 8, 3, codes, used);
            std::string line;
            for (uint8_t code : codes) { char b[4]; std::snprintf(b, sizeof(b), " %02x", code); line += b; }
            rec("aic_text_layout rc %d used %u %u codes%s", rc, used[0], used[1], line.c_str());
        }
        uint8_t one;
        rec("aic_text_layout invalid rc %d %d %d %d", aic_text_layout("a", 1, 1, 1, nullptr, nullptr), aic_text_layout(nullptr, 1, 1, 1, &one, nullptr),
            aic_text_layout("a", 1, 0, 1, &one, nullptr), aic_text_layout("a", 1, 1, 65536, &one, nullptr));
    });
}

// ---- sequences on one context
void sequences() {
    scenario("sequence: reproject, pick, another size, a larger one", [] {
        aic_ctx *c = make_ctx();
        const uint32_t W = 40, H = 24;
        void *src = dev(16 * W * H * 12), *dst = dev(16 * W * H * 12);
        uint32_t *order = (uint32_t *)dev(W * H * 4), *out = (uint32_t *)dev(100 * 4);
        aic_reproject_desc rd = reproject_desc(W, H);
        reproject(c, &rd, src, dst);
        aic_pick_desc d = pick_desc(W, H, 100, 40);
        pick(c, &d, order, out);
        rec("-- a reprojection of another size: the pick of the first size is refused, one of the new size is not");
        rd = reproject_desc(W / 2, H);
        reproject(c, &rd, src, dst);
        pick(c, &d, order, out);
        d = pick_desc(W / 2, H, 100, 40);
        pick(c, &d, nullptr, out);
        rec("-- an empty reprojection leaves the state");
        rd = reproject_desc(0, H);
        reproject(c, &rd, src, dst);
        pick(c, &d, nullptr, out);
        rec("-- a reprojection that grows the scratch");
        rd = reproject_desc(4 * W, 4 * H);
        reproject(c, &rd, src, dst);
        rec("-- picks: without max_unknown, n = 0, no order, no info");
        d = pick_desc(4 * W, 4 * H, 100, 0);
        pick(c, &d, order, out);
        d = pick_desc(4 * W, 4 * H, 0, 5);
        pick(c, &d, nullptr, nullptr);
        d = pick_desc(4 * W, 4 * H, 100, 100);
        pick(c, &d, nullptr, out);
        pick(c, &d, nullptr, out, false);
        for (void *p : {src, dst, (void *)order, (void *)out}) (void)hipFree(p);
        aic_destroy(c);
    });
    for (int clear_keys = 0; clear_keys < 2; clear_keys++)
        scenario("sequence: line calls" + str({clear_keys}), [&] {
            aic_ctx *c = make_ctx(clear_keys);
            const uint32_t W = 40, H = 24;
            static const std::vector<aic_line_vertex> host(2 * 28);
            void *src = dev(W * H * 12), *out = dev(16 * W * H * 8);
            aic_present_desc d = present_desc(W, H, W, H);
            aic_lines_desc l = lines_desc(host.data(), 28);
            present(c, &d, true, &l, src, out, 1);
            rec("-- the second call finds its keys clean");
            present(c, &d, true, &l, src, out, 1);
            rec("-- a call without lines between two with lines");
            present(c, &d, false, nullptr, src, out, 1);
            present(c, &d, true, &l, src, out, 1);
            rec("-- a larger call allocates anew and clears");
            d = present_desc(W, H, 2 * W, 2 * H, 0.125f);
            present(c, &d, true, &l, src, out, 1);
            rec("-- a smaller window after the larger one, then the larger one again");
            d = present_desc(W, H, W, H);
            present(c, &d, true, &l, src, out, 1);
            d = present_desc(W, H, 2 * W, 2 * H);
            present(c, &d, true, &l, src, out, 1);
            rec("-- an empty output with lines");
            d = present_desc(W, H, 0, H);
            present(c, &d, true, &l, src, out, 1);
            (void)hipFree(src); (void)hipFree(out);
            aic_destroy(c);
        });
    scenario("size queries", [] {
        uint32_t levels = 99, t0[2] = {99, 99};
        uint64_t bytes = 99;
        for (const auto &wh : kSizes) {
            const int rc = aic_reproject_geometry(wh[0], wh[1], &levels, t0, &bytes);
            rec("aic_reproject_geometry %ux%u rc %d levels %u t0 %u %u bytes %llu", wh[0], wh[1], rc, levels, t0[0], t0[1], (unsigned long long)bytes);
        }
        rec("aic_reproject_geometry rc %d %d %d", aic_reproject_geometry(65536, 1, &levels, t0, &bytes), aic_reproject_geometry(1, 65536, nullptr, nullptr, nullptr),
            aic_reproject_geometry(65535, 65535, nullptr, nullptr, nullptr));
        for (const auto &s : kPresentShapes) {
            const int rc = aic_present_geometry(s[0], s[1], s[2], s[3], &levels, t0, &bytes);
            rec("aic_present_geometry %ux%u -> %ux%u rc %d levels %u t0 %u %u bytes %llu", s[0], s[1], s[2], s[3], rc, levels, t0[0], t0[1], (unsigned long long)bytes);
            for (uint32_t n : {0u, 1u, 28u}) {
                const int rc2 = aic_present_lines_scratch(s[0], s[1], s[2], s[3], n, &bytes);
                rec("aic_present_lines_scratch %ux%u -> %ux%u n %u rc %d bytes %llu", s[0], s[1], s[2], s[3], n, rc2, (unsigned long long)bytes);
            }
        }
        const uint32_t bad[][4] = {{65536, 1, 8, 8}, {1, 65536, 8, 8}, {8, 8, 65536, 1}, {8, 8, 1, 65536}, {8, 8, 65535, 32769}, {0, 8, 8, 8}, {8, 0, 8, 8}, {0, 0, 8, 0}};
        for (const auto &s : bad)
            rec("invalid sizes %u %u %u %u: rc %d %d", s[0], s[1], s[2], s[3], aic_present_geometry(s[0], s[1], s[2], s[3], nullptr, nullptr, nullptr),
                aic_present_lines_scratch(s[0], s[1], s[2], s[3], 5, nullptr));
        rec("too many lines: rc %d", aic_present_lines_scratch(8, 8, 8, 8, AIC_LINES_MAX + 1u, &bytes));
    });
}

// ---- every rejection, each on its own, on one context; then each entry point's refusal while a frame occupies slot 0
void rejections() {
    const uint32_t W = 40, H = 24, N = 28;
    aic_ctx *c = nullptr;
    char *src = nullptr, *dst = nullptr, *out = nullptr, *lists = nullptr;
    static const std::vector<aic_line_vertex> host(2 * N);
    scenario("rejections: the context they share", [&] {
        c = make_ctx();
        src = (char *)dev(W * H * 12); dst = (char *)dev(W * H * 12); out = (char *)dev(W * H * 8); lists = (char *)dev(2 * N * sizeof(aic_line_vertex) + 8);
    });
    auto arguments = [&] {
        // aic_reproject_split
        auto rp = [&](const char *what, const aic_reproject_desc &d, const void *s, void *o) { rejection(std::string("reproject: ") + what, [&] { reproject(c, &d, s, o); }); };
        auto with = [](aic_reproject_desc d, int at, float v, bool zw = false) { (zw ? d.inverse_projection_zw : d.reprojection)[at] = v; return d; };
        const aic_reproject_desc rd = reproject_desc(W, H);
        rejection("reproject: no context", [&] { reproject(nullptr, &rd, src, dst); });
        rejection("reproject: no desc", [&] { reproject(c, nullptr, src, dst); });
        rp("no src", rd, nullptr, dst);
        rp("no dst", rd, src, nullptr);
        rp("too wide", reproject_desc(65536, 1), src, dst);
        rp("too high", reproject_desc(1, 65536), src, dst);
        rp("unknown flag", reproject_desc(W, H, 2u), src, dst);
        rp("src off by 4", rd, src + 4, dst);
        rp("dst off by 4", rd, src, dst + 4);
        rp("NaN in the matrix", with(rd, 6, kNaN), src, dst);
        rp("infinity in the matrix", with(rd, 15, -kInf), src, dst);
        rp("NaN in ipzw", with(rd, 3, kNaN, true), src, dst);
        rp("src is dst", rd, src, src);
        rp("dst inside src", rd, src, src + W * H * 12 - 8);
        rp("src is dst, empty", reproject_desc(0, H), src, src);
        // aic_pick_pixels
        auto pk = [&](const char *what, const aic_pick_desc &d, const void *order, void *o) {
            rejection(std::string("pick: ") + what, [&] { pick(c, &d, (const uint32_t *)order, (uint32_t *)o); });
        };
        const aic_pick_desc pd = pick_desc(W, H, 10);
        rejection("pick: no context", [&] { pick(nullptr, &pd, nullptr, (uint32_t *)out); });
        rejection("pick: no desc", [&] { pick(c, nullptr, nullptr, (uint32_t *)out); });
        rejection("pick: no info", [&] { pick(c, &pd, nullptr, (uint32_t *)out, false); });
        pk("too wide", pick_desc(65536, 1, 10), nullptr, out);
        pk("too high", pick_desc(1, 65536, 10), nullptr, out);
        pk("a flag", pick_desc(W, H, 10, 0, 1u), nullptr, out);
        pk("too many picks", pick_desc(W, H, 2048u * 65535u + 1u), nullptr, out);
        pk("no list", pd, nullptr, nullptr);
        pk("list off by 2", pd, nullptr, out + 2);
        pk("order off by 1", pd, src + 1, out);
        pk("empty frame", pick_desc(0, H, 10), nullptr, out);
        pk("max_unknown before any reprojection", pick_desc(W, H, 10, 5), nullptr, out);
        // a presentation, through either entry point (form 1: with lines, so under aic_present_split_lines' name)
        for (int form = 0; form < 2; form++) {
            const aic_lines_desc l = lines_desc(host.data(), N);
            auto pr = [&](const char *what, const aic_present_desc &d, const void *s, void *o, int is_device = 1) {
                rejection(std::string("present") + str({form}) + ": " + what, [&] { present(c, &d, form != 0, &l, s, o, is_device); });
            };
            auto with = [](aic_present_desc d, const std::function<void(aic_present_desc &)> &edit) { edit(d); return d; };
            const aic_present_desc d = present_desc(W, H, W, H);
            rejection("present" + str({form}) + ": no context", [&] { present(nullptr, &d, form != 0, &l, src, out, 1); });
            rejection("present" + str({form}) + ": no desc", [&] { present(c, nullptr, form != 0, &l, src, out, 1); });
            pr("no src", d, nullptr, out);
            pr("no out", d, src, nullptr);
            pr("no host out", d, src, nullptr, 0);
            pr("src too wide", present_desc(65536, 1, W, H), src, out);
            pr("src too high", present_desc(1, 65536, W, H), src, out);
            pr("out too wide", present_desc(W, H, 65536, 1), src, out);
            pr("out too high", present_desc(W, H, 1, 65536), src, out);
            pr("more than 2^31 pixels", present_desc(W, H, 65535, 32769), src, out);
            pr("src of no width", present_desc(0, H, W, H), src, out);
            pr("src of no height", present_desc(W, 0, W, H), src, out);
            pr("unknown flag", present_desc(W, H, W, H, 0.f, 2u), src, out);
            pr("negative bloom", present_desc(W, H, W, H, -0.125f), src, out);
            pr("NaN bloom", present_desc(W, H, W, H, kNaN), src, out);
            pr("infinite bloom", present_desc(W, H, W, H, kInf), src, out);
            pr("negative maximum_intensity", with(d, [](aic_present_desc &e) { e.maximum_intensity = -1.f; }), src, out);
            pr("NaN maximum_intensity", with(d, [](aic_present_desc &e) { e.maximum_intensity = kNaN; }), src, out);
            pr("tone_mapping 2", with(d, [](aic_present_desc &e) { e.tone_mapping = 2; }), src, out);
            pr("tone_mapping -1", with(d, [](aic_present_desc &e) { e.tone_mapping = -1; }), src, out);
            pr("src off by 4", d, src + 4, out);
            pr("out off by 2", d, src, out + 2);
            pr("f16 out off by 4", present_desc(W, H, W, H, 0.f, AIC_PRESENT_OUT_F16), src, out + 4);
            pr("out is src", d, src, src);
            pr("out inside src", d, src, src + W * H * 12 - 4);
        }
        // what aic_present_split_lines adds, with lines and (where the list's length allows) without
        const aic_present_desc d = present_desc(W, H, W, H);
        auto ln = [&](const char *what, const aic_lines_desc &l) { rejection(std::string("lines: ") + what, [&] { present(c, &d, true, &l, src, out, 1); }); };
        auto with_vp = [](aic_lines_desc l, int at, float v) { l.view_projection[at] = v; return l; };
        for (uint32_t n : {N, 0u}) {
            ln(("unknown flag, n_lines" + str({n})).c_str(), lines_desc(host.data(), n, 2u));
            ln(("NaN in view_projection, n_lines" + str({n})).c_str(), with_vp(lines_desc(host.data(), n), 6, kNaN));
            ln(("infinity in view_projection, n_lines" + str({n})).c_str(), with_vp(lines_desc(host.data(), n), 15, kInf));
        }
        ln("too many lines", lines_desc(host.data(), AIC_LINES_MAX + 1u));
        ln("no vertices", lines_desc(nullptr, N));
        ln("no device vertices", lines_desc(nullptr, N, AIC_LINES_DEVICE));
        ln("device vertices off by 2", lines_desc((const aic_line_vertex *)(lists + 2), N, AIC_LINES_DEVICE));
        ln("line rejections come before the presentation's", lines_desc(host.data(), N, 2u));
        rejection("lines: line rejections come before the presentation's, no desc", [&] { const aic_lines_desc l = lines_desc(host.data(), N, 2u); present(c, nullptr, true, &l, src, out, 1); });
        // aic_export_split: colour in `out`, depth in `dst`
        auto ex = [&](const char *what, const aic_export_desc &e, const void *s, void *color, void *depth, int is_device = 1, bool want_info = true) {
            rejection(std::string("export: ") + what, [&] { export_split(c, &e, s, color, (float *)depth, is_device, want_info); });
        };
        auto with_zw = [](aic_export_desc e, int at, float v) { e.inverse_projection_zw[at] = v; return e; };
        const aic_export_desc ed = export_desc(W, H, W, H);
        rejection("export: no context", [&] { export_split(nullptr, &ed, src, out, (float *)dst, 1); });
        rejection("export: no desc", [&] { export_split(c, nullptr, src, out, (float *)dst, 1); });
        ex("no src", ed, nullptr, out, dst);
        ex("nothing asked for", ed, src, nullptr, nullptr, 1, false);
        ex("nothing asked for of the host", ed, src, nullptr, nullptr, 0, false);
        ex("src off by 4", ed, src + 4, out, dst);
        ex("color_out off by 2", ed, src, out + 2, dst);
        ex("depth_out off by 1", ed, src, out, dst + 1);
        ex("color_out is src", ed, src, src, dst);
        ex("depth_out inside src", ed, src, out, src + W * H * 12 - 4);
        ex("depth_out is color_out", ed, src, out, out);
        ex("color_out inside depth_out", ed, src, dst + W * H * 4 - 4, dst);
        ex("src too wide", export_desc(65536, 1, W, H), src, out, dst);
        ex("src too high", export_desc(1, 65536, W, H), src, out, dst);
        ex("out too wide", export_desc(W, H, 65536, 1), src, out, dst);
        ex("out too high", export_desc(W, H, 1, 65536), src, out, dst);
        ex("more than 2^31 pixels", export_desc(W, H, 65535, 32769), src, out, dst);
        ex("src of no width", export_desc(0, H, W, H), src, out, dst);
        ex("src of no height", export_desc(W, 0, W, H), src, out, dst);
        ex("NaN in ipzw", with_zw(ed, 2, kNaN), src, out, dst);
        ex("infinity in ipzw", with_zw(ed, 0, -kInf), src, out, dst);
        ex("unknown flag", export_desc(W, H, W, H, 1u), src, out, dst);
    };
    arguments();
    scenario("rejections: the context they shared is released", [&] {
        for (void *p : {src, dst, out, lists}) (void)hipFree(p);
        aic_destroy(c);
    }, false);
    scenario("rejections: a frame occupies slot 0", [&] {
        c = make_ctx();
        src = (char *)dev(W * H * 12); dst = (char *)dev(W * H * 12); out = (char *)dev(W * H * 8); lists = (char *)dev(8 * 8 * 4);
        submit_to_slot0(c, lists);
        rec_state(c);
    });
    const aic_reproject_desc rd = reproject_desc(W, H);
    const aic_pick_desc pd = pick_desc(W, H, 10);
    const aic_present_desc d = present_desc(W, H, W, H);
    const aic_lines_desc l = lines_desc(host.data(), N), none = lines_desc(nullptr, 0);
    rejection("busy: reproject", [&] { reproject(c, &rd, src, dst); });
    rejection("busy: pick", [&] { pick(c, &pd, nullptr, (uint32_t *)out); });
    rejection("busy: present", [&] { present(c, &d, false, nullptr, src, out, 1); });
    rejection("busy: present with lines", [&] { present(c, &d, true, &l, src, out, 1); });
    rejection("busy: present through aic_present_split_lines, no lines", [&] { present(c, &d, true, &none, src, out, 1); });
    const std::vector<uint8_t> busy_atlas = atlas_9x18(true);
    rejection("busy: font", [&] { set_font(c, busy_atlas.data(), 9, 18, 1); });
    const aic_export_desc ed = export_desc(W, H, W, H);
    rejection("busy: export", [&] { export_split(c, &ed, src, out, (float *)dst, 1); });
    scenario("rejections: the frame is waited for, and every entry point runs", [&] {
        aic_frame_info fi;
        rec_rc(c, "aic_render_wait", aic_render_wait(c, 0, &fi));
        reproject(c, &rd, src, dst);
        pick(c, &pd, nullptr, (uint32_t *)out);
        present(c, &d, false, nullptr, src, out, 1);
        present(c, &d, true, &l, src, out, 1);
        for (void *p : {src, dst, out, lists}) (void)hipFree(p);
        aic_destroy(c);
    }, false);
    scenario("export: after a frame was waited for", [&] {
        c = make_ctx();
        src = (char *)dev(W * H * 12); dst = (char *)dev(W * H * 4); out = (char *)dev(W * H * 4); lists = (char *)dev(8 * 8 * 4);
        submit_to_slot0(c, lists);
        aic_frame_info fi;
        rec_rc(c, "aic_render_wait", aic_render_wait(c, 0, &fi));
        export_split(c, &ed, src, out, (float *)dst, 1);
        for (void *p : {src, dst, out, lists}) (void)hipFree(p);
        aic_destroy(c);
    });
}

// ---- what aic_set_text_font and aic_present_split_text refuse, each on its own, on a context of their own
void text_rejections() {
    const uint32_t W = 40, H = 24, N = 28;
    aic_ctx *c = nullptr;
    char *src = nullptr, *out = nullptr;
    static const std::vector<aic_line_vertex> host(2 * N);
    scenario("text rejections: the context they share", [&] {
        c = make_ctx();
        src = (char *)dev(W * H * 12); out = (char *)dev(W * H * 8);
    });
    // what aic_set_text_font and aic_present_split_text add; the font is set by a scenario of its own, then every refusal stands alone
    const std::vector<uint8_t> atlas = atlas_9x18(true);
    rejection("font: no context", [&] { set_font(nullptr, atlas.data(), 9, 18, 1); });
    rejection("font: cell of no width", [&] { set_font(c, atlas.data(), 0, 18, 1); });
    rejection("font: cell too high", [&] { set_font(c, atlas.data(), 9, 1025, 1); });
    rejection("font: margin takes the whole cell", [&] { set_font(c, atlas.data(), 4, 18, 2); });
    {
        const aic_present_desc d = present_desc(W, H, W, H);
        const aic_text_desc t = text_desc(kCodes);
        rejection("text: no font set", [&] { present_text(c, &d, nullptr, &t, src, out, 1); });
    }
    scenario("text rejections: a font for the context they share", [&] { set_font(c, atlas.data(), 9, 18, 1); }, false);
    {
        const aic_present_desc d = present_desc(W, H, W, H);
        const aic_lines_desc l = lines_desc(host.data(), N);
        auto tr = [&](const char *what, const aic_text_desc &t, const aic_lines_desc *ld = nullptr) {
            rejection(std::string("text: ") + what, [&] { present_text(c, &d, ld, &t, src, out, 1); });
        };
        auto with = [](aic_text_desc t, const std::function<void(aic_text_desc &)> &edit) { edit(t); return t; };
        const aic_text_desc t = text_desc(kCodes);
        tr("no codes", text_desc(nullptr));
        tr("no device codes", text_desc(nullptr, AIC_TEXT_DEVICE));
        tr("unknown flag", text_desc(kCodes, 2u));
        tr("no columns", with(t, [](aic_text_desc &e) { e.cols = 0; }));
        tr("no rows", with(t, [](aic_text_desc &e) { e.rows = 0; }));
        tr("too many columns", with(t, [](aic_text_desc &e) { e.cols = 65536; }));
        tr("too many rows", with(t, [](aic_text_desc &e) { e.rows = 65536; }));
        tr("NaN scale", with(t, [](aic_text_desc &e) { e.scale[1] = kNaN; }));
        tr("infinite origin", with(t, [](aic_text_desc &e) { e.origin[0] = -kInf; }));
        tr("a bad line list", t, [&] { static aic_lines_desc bad; bad = lines_desc(host.data(), N, 2u); return &bad; }());
        rejection("text: the presentation's own, no src", [&] { present_text(c, &d, &l, &t, nullptr, out, 1); });
        rejection("text: the presentation's own, no context", [&] { present_text(nullptr, &d, &l, &t, src, out, 1); });
        const aic_present_desc bad = present_desc(W, H, W, H, -0.125f);
        rejection("text: the presentation's own, negative bloom", [&] { present_text(c, &bad, nullptr, &t, src, out, 1); });
    }
    scenario("text rejections: a good call, and the context is released", [&] {
        const aic_present_desc d = present_desc(W, H, W, H);
        const aic_text_desc t = text_desc(kCodes);
        present_text(c, &d, nullptr, &t, src, out, 1);
        for (void *p : {src, out}) (void)hipFree(p);
        aic_destroy(c);
    }, false);
}

// ---- failed runtime calls: every runtime call and launch of one good call per entry point fails in turn, each in a context of its own; the same call
// is then made once more on that context, and is good
struct Buffers { void *src, *dst, *out, *list; };  // the caller's device memory: two 40 x 24 Split frames, an output of up to 80 x 48 f16, a list
void runtime_failures(const std::string &name, bool lines_clear_keys, const std::function<int(aic_ctx *, const Buffers &)> &call,
                      const std::function<void(aic_ctx *, const Buffers &)> &before = nullptr) {
    static const char *fns[] = {"hipSetDevice", "hipMalloc", "hipMemcpyAsync", "hipEventRecord", "hipGetLastError", "hipStreamSynchronize", "hipEventElapsedTime",
                                "launch_reproject", "launch_pick", "launch_present_lines", "launch_export"};
    const size_t n_fns = sizeof(fns) / sizeof(fns[0]);
    // fail < 0: the good call alone, which counts what there is to fail
    auto run = [&](int fn, int nth, int *counts) {
        aic_ctx *c = make_ctx(lines_clear_keys);
        const Buffers b = {dev(40 * 24 * 12), dev(40 * 24 * 12), dev(80 * 48 * 8), dev(2 * 28 * sizeof(aic_line_vertex))};
        if (before) before(c, b);
        if (fn >= 0) fake_fail(fns[fn], nth);
        for (size_t i = 0; counts && i < n_fns; i++) counts[i] = -fake_calls(fns[i]);
        const int rc = call(c, b);
        for (size_t i = 0; counts && i < n_fns; i++) counts[i] += fake_calls(fns[i]);
        if (fn >= 0) {
            if (rc == AIC_OK) rec("FAILED to fail");
            rec("-- the same call again");
            call(c, b);
        }
        for (void *p : {b.src, b.dst, b.out, b.list}) (void)hipFree(p);
        aic_destroy(c);
    };
    int counts[n_fns];
    scenario("failures: " + name + ", the good call", [&] { run(-1, 0, counts); });
    for (size_t i = 0; i < n_fns; i++)
        for (int nth = 0; nth < counts[i]; nth++) scenario("failures: " + name + " " + fns[i] + str({nth}), [&] { run((int)i, nth, nullptr); });
}

void all_runtime_failures() {
    const uint32_t W = 40, H = 24;
    static const std::vector<aic_line_vertex> host(2 * 28);
    static std::vector<char> image(2 * W * 2 * H * 8);
    static const aic_reproject_desc rd = reproject_desc(W, H);
    runtime_failures("reproject", false, [](aic_ctx *c, const Buffers &b) { return reproject(c, &rd, b.src, b.dst); });
    runtime_failures("pick", false, [&](aic_ctx *c, const Buffers &b) { const aic_pick_desc d = pick_desc(W, H, 50, 20); return pick(c, &d, nullptr, (uint32_t *)b.out); },
                     [](aic_ctx *c, const Buffers &b) { reproject(c, &rd, b.src, b.dst); });
    // bloomed and stretched, so that every scratch is allocated; to the host and to the device
    for (int to_device = 0; to_device < 2; to_device++) {
        runtime_failures("present" + str({to_device}), false, [&](aic_ctx *c, const Buffers &b) {
            const aic_present_desc d = present_desc(W, H, 2 * W, 2 * H, 0.125f, to_device ? AIC_PRESENT_OUT_F16 : 0u);
            return present(c, &d, false, nullptr, b.src, to_device ? b.out : (void *)image.data(), to_device);
        });
        for (int clear_keys = 0; clear_keys < 2; clear_keys++)
            runtime_failures("lines" + str({to_device, clear_keys}), clear_keys, [&](aic_ctx *c, const Buffers &b) {
                const aic_present_desc d = present_desc(W, H, 2 * W, 2 * H, 0.125f, to_device ? AIC_PRESENT_OUT_F16 : 0u);
                const aic_lines_desc l = to_device ? lines_desc((const aic_line_vertex *)b.list, 28, AIC_LINES_DEVICE) : lines_desc(host.data(), 28);
                return present(c, &d, true, &l, b.src, to_device ? b.out : (void *)image.data(), to_device);
            });
    }
    // with text: the font set before the counted call; a host list to the host, a device list (in the vertex list's buffer) to the device
    static const std::vector<uint8_t> atlas = atlas_9x18(true);
    for (int to_device = 0; to_device < 2; to_device++)
        runtime_failures("text" + str({to_device}), false, [&](aic_ctx *c, const Buffers &b) {
            const aic_present_desc d = present_desc(W, H, 2 * W, 2 * H, 0.125f, to_device ? AIC_PRESENT_OUT_F16 : 0u);
            const aic_lines_desc l = lines_desc(host.data(), 28);
            const aic_text_desc t = to_device ? text_desc((const uint8_t *)b.list, AIC_TEXT_DEVICE) : text_desc(kCodes);
            return present_text(c, &d, &l, &t, b.src, to_device ? b.out : (void *)image.data(), to_device);
        }, [](aic_ctx *c, const Buffers &) { set_font(c, atlas.data(), 9, 18, 1); });
    runtime_failures("font", false, [](aic_ctx *c, const Buffers &) { return set_font(c, atlas.data(), 9, 18, 1); });
    // stretched, both planes: colour in the output buffer, depth in the second frame's; to the host and to the device
    for (int to_device = 0; to_device < 2; to_device++)
        runtime_failures("export" + str({to_device}), false, [&](aic_ctx *c, const Buffers &b) {
            const aic_export_desc d = export_desc(W, H, 2 * W, 2 * H);
            return export_split(c, &d, b.src, to_device ? b.out : (void *)image.data(), to_device ? (float *)((char *)b.out + 2 * W * 2 * H * 4) : (float *)(image.data() + 2 * W * 2 * H * 4),
                                to_device);
        });
}

}  // namespace

int main() {
    shapes();
    exports();
    lines();
    text();
    sequences();
    rejections();
    text_rejections();
    all_runtime_failures();
    fake_reset();
    rec("total: %d scenarios", n_scenarios);
    return 0;
}
