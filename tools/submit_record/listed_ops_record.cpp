// listed_ops_record.cpp -- drives the calls that take a list and work on it on the device and that driver.cpp, split_ops_record.cpp and
// cursor_raycast_record.cpp leave out: aic_trace_pixels (csrc/aic_frame.cpp), aic_sample_luminance and, for its state, aic_cursor_raycast
// (csrc/aic_ray_queries.cpp) and aic_pick_stale (csrc/aic_split_ops.cpp), through a fixed list of scenarios against the recording fake (fake_hip.cpp), and
// prints the record: every runtime call and launch with its arguments, each call's return code and message, every field of its info struct and what the
// context keeps for these calls afterwards. Two builds of the host code make the same calls exactly when their records are byte-identical (build.sh,
// tests/test_listed_ops_record_cpu.py). A scenario named "reject: ..." is one refused call on a context an earlier scenario made; every other scenario
// starts with ordinals from zero and frees what it allocates. A line that begins with FAILED is an expectation of this file that did not hold.
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

// a context with driver.cpp's 8 x 8 x 8 world
aic_ctx *make_ctx() {
    int st = 0;
    aic_ctx *c = aic_create(0, &st);
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
    s.sky[0][0] = 0.25f; s.sky[0][1] = 0.5f; s.sky[0][2] = 0.75f;
    s.block_index = cubes.data(); s.light = light.data(); s.n_blocks = 2; s.blocks = blocks; s.voxels = voxels; s.n_voxels = 1; s.palette = palette; s.n_palette = 2;
    if (aic_upload_space(c, 0, &s) != AIC_OK) rec("FAILED aic_upload_space : %s", aic_last_error(c));
    return c;
}

aic_frame_desc frame(uint32_t w, uint32_t h, uint32_t flags = 0) {
    aic_frame_desc f;
    std::memset(&f, 0, sizeof(f));
    f.width = w; f.height = h; f.flags = flags;
    for (int i = 0; i < 4; i++) f.world.inverse_projection_view[5 * i] = f.ui.inverse_projection_view[5 * i] = 1.0;
    f.world.exposure = 1.5f; f.ui.exposure = 0.75f;
    return f;
}
void submit(aic_ctx *c, uint32_t slot, void *out) {  // out: 8 x 8 x 4 bytes on the device
    const aic_frame_desc f = frame(8, 8);
    if (aic_render_submit(c, &f, out, slot) != AIC_OK) rec("FAILED aic_render_submit : %s", aic_last_error(c));
}

// ---- what is recorded after every call
void rec_state(const aic_ctx *c) {
    if (!c) return;
    const Layer &l = c->layers[0];
    rec("  state exposure_scratch %zu/%zu cursor_scratch %zu/%zu stale_scratch %zu/%zu out %zu/%zu staging %zu/%zu aux %zu/%zu visible_bits %zu/%zu version %llu visible_version %lld slot0_busy %d",
        c->exposure_scratch.n, c->exposure_scratch.cap, c->cursor_scratch.n, c->cursor_scratch.cap, c->stale_scratch.n, c->stale_scratch.cap, c->out.n, c->out.cap, c->staging.n,
        c->staging.cap, c->aux.n, c->aux.cap, l.visible_bits.n, l.visible_bits.cap, (unsigned long long)l.version, (long long)l.visible_version, (int)c->slots[0].busy);
}
void rec_rc(const aic_ctx *c, const char *call, int rc) { rec("%s rc %d%s%s", call, rc, rc ? " : " : "", rc ? aic_last_error(c) : ""); }

// Every info struct is handed over filled with 0xff bytes, so that a field the call leaves alone shows as such.
int pixels(aic_ctx *c, const aic_frame_desc *f, uint32_t n, const uint32_t *list, uint32_t mode, void *out, aic_pixel_aux *aux, bool want_info = true) {
    aic_frame_info i;
    std::memset(&i, 0xff, sizeof(i));
    const int rc = aic_trace_pixels(c, f, n, list, mode, out, aux, want_info ? &i : nullptr);
    rec_rc(c, "aic_trace_pixels", rc);
    rec("  info cubes %llu outer %llu inner %llu hits %llu light %llu kernel_ms %a rows %u flaws %u variant %u tile_queues %u", (unsigned long long)i.cubes_traced,
        (unsigned long long)i.n_outer, (unsigned long long)i.n_inner, (unsigned long long)i.n_hits, (unsigned long long)i.n_light, i.kernel_ms, i.rows_rendered, i.flaws, i.variant,
        i.tile_queues);
    rec_state(c);
    return rc;
}
int luminance(aic_ctx *c, int layer, uint32_t n, const double *rays, uint32_t max_steps, uint32_t flags, float *out) {
    const int rc = aic_sample_luminance(c, layer, n, rays, max_steps, flags, out);
    rec_rc(c, "aic_sample_luminance", rc);
    rec_state(c);
    return rc;
}
int cursor(aic_ctx *c, int layer, uint32_t n, const double *rays, double maximum_distance, uint32_t flags, aic_cursor_hit *out) {
    const int rc = aic_cursor_raycast(c, layer, n, rays, maximum_distance, flags, out);
    rec_rc(c, "aic_cursor_raycast", rc);
    rec_state(c);
    return rc;
}
int stale(aic_ctx *c, const aic_stale_desc *d, const void *src, const uint32_t *order, uint32_t *out, bool want_info = true) {
    aic_stale_info i;
    std::memset(&i, 0xff, sizeof(i));
    const int rc = aic_pick_stale(c, d, src, order, out, want_info ? &i : nullptr);
    rec_rc(c, "aic_pick_stale", rc);
    rec("  info stale %llu next_cursor %llu from_stale %u from_order %u kernel_ms %a reserved %u", (unsigned long long)i.n_stale, (unsigned long long)i.next_cursor, i.n_from_stale,
        i.n_from_order, i.kernel_ms, i.reserved);
    rec_state(c);
    return rc;
}

aic_stale_rect rect(uint16_t x0, uint16_t y0, uint16_t x1, uint16_t y1, float dmin = 0.25f) {
    aic_stale_rect r;
    std::memset(&r, 0, sizeof(r));
    r.x0 = x0; r.y0 = y0; r.x1 = x1; r.y1 = y1; r.dmin = dmin;
    return r;
}
aic_stale_desc stale_desc(uint32_t w, uint32_t h, uint32_t n, uint32_t max_stale, const std::vector<aic_stale_rect> &rects, uint32_t flags = 0) {
    aic_stale_desc d;
    std::memset(&d, 0, sizeof(d));
    d.width = w; d.height = h; d.n = n; d.max_stale = max_stale; d.flags = flags;
    d.skip_stale = 3; d.cursor = (1ull << 40) + 7;
    d.n_rects = (uint32_t)rects.size(); d.rects = rects.empty() ? nullptr : rects.data();
    return d;
}

// one scenario: ordinals from zero, everything it allocates freed at its end -- or (not fresh) one that goes on with what the scenario before left
void scenario(const std::string &name, const std::function<void()> &body, bool fresh = true) {
    if (fresh) fake_reset();
    rec("== %s", name.c_str());
    n_scenarios++;
    body();
}
// one refused call on the context of the scenario before, so that nothing but the call stands between its name and its result
void rejection(const std::string &name, const std::function<void()> &call) { scenario("reject: " + name, call, false); }
std::string str(std::initializer_list<long> v) { std::string s; for (long x : v) s += " " + std::to_string(x); return s; }

const uint32_t kCounts[] = {0, 1, 63, 64, 65, 2049};  // (2049: the first batch image with a second row)
const uint32_t kOutModes[] = {0, AIC_FRAME_OUT_LINEAR, AIC_FRAME_OUT_COLORBUF, AIC_FRAME_OUT_SPLIT};
const uint32_t kW = 64, kH = 48;
size_t px_bytes(uint32_t flags) { return (flags & (AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) ? 16 : ((flags & AIC_FRAME_OUT_SPLIT) ? 12 : 4); }
std::vector<uint32_t> pixel_list(uint32_t n) {
    std::vector<uint32_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = (i * 7u) % (kW * kH);
    return v;
}

// ---- shapes
void shapes() {
    // layout 0: a host list, compact; 1: a device list, compact; 2: a device list, in place
    for (uint32_t n : kCounts)
        for (uint32_t flags : kOutModes)
            for (int layout = 0; layout < 3; layout++)
                for (int aux = 0; aux < 2; aux++)
                    scenario("pixels" + str({n, flags, layout, aux}), [&] {
                        aic_ctx *c = make_ctx();
                        const aic_frame_desc f = frame(kW, kH, flags | AIC_FRAME_PIXEL_CENTERS);
                        const std::vector<uint32_t> list = pixel_list(n);
                        const size_t out_bytes = (layout == 2 ? (size_t)kW * kH : (size_t)n) * px_bytes(flags), aux_bytes = (size_t)n * sizeof(aic_pixel_aux);
                        if (layout) {
                            void *d_list = dev((size_t)n * 4), *d_out = dev(out_bytes), *d_aux = aux ? dev(aux_bytes) : nullptr;
                            const uint32_t mode = AIC_PIXELS_DEVICE | (layout == 2 ? AIC_PIXELS_IN_PLACE : 0u);
                            const int a0 = fake_calls("hipMemcpy");
                            for (int turn = 0; turn < 2; turn++) pixels(c, &f, n, (const uint32_t *)d_list, mode, d_out, (aic_pixel_aux *)d_aux);  // (the second finds the slot's buffers)
                            pixels(c, &f, n, (const uint32_t *)d_list, mode, d_out, (aic_pixel_aux *)d_aux, false);                                     // (no info)
                            if (fake_calls("hipMemcpy") != a0) rec("FAILED a device list: a blocking copy");
                            for (void *p : {d_list, d_out, d_aux})
                                if (p) (void)hipFree(p);
                        } else {
                            std::vector<char> out(out_bytes + 1);
                            std::vector<aic_pixel_aux> hits(n + 1);
                            for (int turn = 0; turn < 2; turn++) pixels(c, &f, n, list.data(), 0, out.data(), aux ? hits.data() : nullptr);
                            pixels(c, &f, n, list.data(), 0, out.data(), aux ? hits.data() : nullptr, false);
                        }
                        aic_destroy(c);
                    });
    scenario("pixels: an empty viewport", [] {
        aic_ctx *c = make_ctx();
        const aic_frame_desc f = frame(0, 7);
        void *d_list = dev(16), *d_out = dev(16);
        pixels(c, &f, 4, (const uint32_t *)d_list, AIC_PIXELS_DEVICE, d_out, nullptr);
        pixels(c, &f, 0, nullptr, 0, nullptr, nullptr);
        (void)hipFree(d_list); (void)hipFree(d_out);
        aic_destroy(c);
    });
    // two calls with the scene unchanged, then one after a scene write: the bitmap is made once per Layer::version
    for (uint32_t n : kCounts)
        for (int on_device = 0; on_device < 2; on_device++) {
            scenario("luminance" + str({n, on_device}), [&] {
                aic_ctx *c = make_ctx();
                const std::vector<double> rays((size_t)n * 6 + 1, 0.25);
                std::vector<float> out(n + 1);
                void *d_rays = on_device ? dev((size_t)n * 48) : nullptr, *d_out = on_device ? dev((size_t)n * 4) : nullptr;
                auto call = [&] {
                    return on_device ? luminance(c, 0, n, (const double *)d_rays, 40, AIC_RAYS_DEVICE, (float *)d_out) : luminance(c, 0, n, rays.data(), 40, 0, out.data());
                };
                call();
                call();
                const int32_t xyz[3] = {1, 2, 3};
                const uint16_t block = 0;
                rec_rc(c, "aic_update_cubes", aic_update_cubes(c, 0, 1, xyz, &block, nullptr));
                call();
                if (d_rays) { (void)hipFree(d_rays); (void)hipFree(d_out); }
                aic_destroy(c);
            });
            scenario("cursor" + str({n, on_device}), [&] {
                aic_ctx *c = make_ctx();
                const std::vector<double> rays((size_t)n * 6 + 1, 0.25);
                std::vector<aic_cursor_hit> out(n + 1);
                void *d_rays = on_device ? dev((size_t)n * 48) : nullptr, *d_out = on_device ? dev((size_t)n * sizeof(aic_cursor_hit)) : nullptr;
                for (int turn = 0; turn < 2; turn++) {
                    if (on_device) cursor(c, 0, n, (const double *)d_rays, 6.0, AIC_RAYS_DEVICE, (aic_cursor_hit *)d_out);
                    else cursor(c, 0, n, rays.data(), 6.0, 0, out.data());
                }
                if (d_rays) { (void)hipFree(d_rays); (void)hipFree(d_out); }
                aic_destroy(c);
            });
        }
    // what: 0 rectangles that hold pixels (looked at); 1 max_stale 0; 2 no rectangle; 3 rectangles that hold no pixel
    for (uint32_t n : kCounts)
        for (uint32_t depth_test : {0u, (uint32_t)AIC_STALE_DEPTH_TEST})
            for (int what = 0; what < 4; what++)
                scenario("stale" + str({n, depth_test, what}), [&] {
                    aic_ctx *c = make_ctx();
                    const size_t count = (size_t)kW * kH;
                    void *src = dev(count * 12);
                    uint32_t *order = (uint32_t *)dev(count * 4), *out = (uint32_t *)dev((size_t)n * 4);
                    std::vector<aic_stale_rect> rects;
                    if (what == 0 || what == 1) rects = {rect(1, 2, 30, 40), rect(5, 5, 5, 9), rect(0, 0, kW, kH, -std::numeric_limits<float>::infinity())};
                    if (what == 3) rects = {rect(5, 5, 5, 9), rect(7, 3, 20, 3)};
                    const aic_stale_desc d = stale_desc(kW, kH, n, what == 1 ? 0u : n / 2 + 1, rects, depth_test);
                    stale(c, &d, src, order, out);
                    stale(c, &d, src, nullptr, out);  // (row-major; finds its scratch)
                    stale(c, &d, depth_test && what == 0 && n ? src : nullptr, order, out);  // (the frame is only asked for where it is read)
                    for (void *p : {src, (void *)order, (void *)out}) (void)hipFree(p);
                    aic_destroy(c);
                });
    scenario("stale: an empty frame, and a scratch that grows", [] {
        aic_ctx *c = make_ctx();
        void *src = dev(640 * 360 * 12);
        uint32_t *out = (uint32_t *)dev(100 * 4);
        const std::vector<aic_stale_rect> one = {rect(0, 0, 8, 8)}, none;
        aic_stale_desc d = stale_desc(0, 0, 0, 0, none);
        stale(c, &d, nullptr, nullptr, nullptr);
        d = stale_desc(8, 8, 100, 50, one);
        stale(c, &d, src, nullptr, out);
        d = stale_desc(640, 360, 100, 50, one, AIC_STALE_DEPTH_TEST);
        stale(c, &d, src, nullptr, out);
        d = stale_desc(8, 8, 100, 50, one);
        stale(c, &d, src, nullptr, out);
        (void)hipFree(src); (void)hipFree(out);
        aic_destroy(c);
    });
}

// ---- with frames in flight: the ray queries run on the upload stream and touch no slot; the two that use slot 0 refuse while it is busy
void in_flight() {
    scenario("in flight", [] {
        aic_ctx *c = make_ctx();
        void *frame_out = dev(8 * 8 * 4);
        const std::vector<double> rays(6 * 10, 0.25);
        std::vector<float> lum(10);
        std::vector<aic_cursor_hit> hits(10);
        rec("-- submit");
        submit(c, 0, frame_out);
        submit(c, 1, frame_out);
        rec("-- queries");
        if (luminance(c, 0, 10, rays.data(), 40, 0, lum.data()) != AIC_OK) rec("FAILED aic_sample_luminance beside frames in flight");
        if (cursor(c, 0, 10, rays.data(), 6.0, 0, hits.data()) != AIC_OK) rec("FAILED aic_cursor_raycast beside frames in flight");
        rec("-- wait");
        aic_frame_info info;
        rec_rc(c, "aic_render_wait", aic_render_wait(c, 0, &info));
        rec_rc(c, "aic_render_wait", aic_render_wait(c, 1, &info));
        (void)hipFree(frame_out);
        aic_destroy(c);
    });
}

// ---- every refusal, each a scenario of its own on one context
void rejections() {
    static aic_ctx *c;
    static char *d_a, *d_b, *d_c, *frame_out;
    static std::vector<uint32_t> list;
    static std::vector<char> host_out(4096);
    static std::vector<double> rays(6 * 10, 0.25);
    static std::vector<float> lum(10);
    static std::vector<aic_stale_rect> one = {rect(0, 0, 8, 8)};
    scenario("rejections: the context", [] {
        c = make_ctx();
        d_a = (char *)dev(65536); d_b = (char *)dev(65536); d_c = (char *)dev(65536); frame_out = (char *)dev(8 * 8 * 4);
        list = pixel_list(10);
        rec_state(c);
    });
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const uint32_t too_many = 2048u * 65535u + 1u;
    auto with = [](aic_frame_desc f, const std::function<void(aic_frame_desc &)> &edit) { edit(f); return f; };
    // aic_trace_pixels
    struct PixelCase { const char *what; aic_ctx *c; aic_frame_desc f; bool no_frame; uint32_t n; const void *list; uint32_t mode; void *out; void *aux; };
    const aic_frame_desc ok = frame(kW, kH);
    const uint32_t D = AIC_PIXELS_DEVICE;
    const std::vector<uint32_t> outside = {1, 2, kW * kH};
    const PixelCase pixel_cases[] = {
        {"no context", nullptr, ok, false, 10, list.data(), 0, host_out.data(), nullptr},
        {"no frame", c, ok, true, 10, list.data(), 0, host_out.data(), nullptr},
        {"no list", c, ok, false, 10, nullptr, 0, host_out.data(), nullptr},
        {"no out", c, ok, false, 10, list.data(), 0, nullptr, nullptr},
        {"in place without a device list", c, ok, false, 10, list.data(), AIC_PIXELS_IN_PLACE, host_out.data(), nullptr},
        {"bloom", c, frame(kW, kH, AIC_FRAME_BLOOM), false, 10, list.data(), 0, host_out.data(), nullptr},
        {"a partition", c, with(ok, [](aic_frame_desc &f) { f.partition = aic_partition{8, 2, 0, 0}; }), false, 10, list.data(), 0, host_out.data(), nullptr},
        {"split with linear", c, frame(kW, kH, AIC_FRAME_OUT_SPLIT | AIC_FRAME_OUT_LINEAR), false, 10, list.data(), 0, host_out.data(), nullptr},
        {"split with colorbuf", c, frame(kW, kH, AIC_FRAME_OUT_SPLIT | AIC_FRAME_OUT_COLORBUF), false, 10, list.data(), 0, host_out.data(), nullptr},
        {"too wide", c, frame(65536, 1), false, 10, list.data(), 0, host_out.data(), nullptr},
        {"too high", c, frame(1, 65536), false, 10, list.data(), 0, host_out.data(), nullptr},
        {"negative exposure", c, with(ok, [](aic_frame_desc &f) { f.world.exposure = -1.f; }), false, 10, list.data(), 0, host_out.data(), nullptr},
        {"NaN UI exposure", c, with(ok, [&](aic_frame_desc &f) { f.ui.exposure = nan; }), false, 10, list.data(), 0, host_out.data(), nullptr},
        {"device list off by 2", c, ok, false, 10, d_a + 2, D, d_b, nullptr},
        {"device out off by 2", c, ok, false, 10, d_a, D, d_b + 2, nullptr},
        {"device Split out off by 4", c, frame(kW, kH, AIC_FRAME_OUT_SPLIT), false, 10, d_a, D, d_b + 4, nullptr},
        {"device float out off by 8", c, frame(kW, kH, AIC_FRAME_OUT_LINEAR), false, 10, d_a, D, d_b + 8, nullptr},
        {"device aux off by 4", c, ok, false, 10, d_a, D, d_b, d_c + 4},
        {"misaligned with n = 0", c, ok, false, 0, d_a + 2, D, d_b, nullptr},
        {"a listed pixel outside the frame", c, ok, false, 3, outside.data(), 0, host_out.data(), nullptr},
        {"too many pixels", c, ok, false, too_many, d_a, D, d_b, nullptr},
    };
    for (const PixelCase &k : pixel_cases)
        rejection(std::string("pixels: ") + k.what, [&] {
            const int rc = pixels(k.c, k.no_frame ? nullptr : &k.f, k.n, (const uint32_t *)k.list, k.mode, k.out, (aic_pixel_aux *)k.aux);
            if (rc != AIC_ERR_INVALID && rc != AIC_ERR_UNSUPPORTED) rec("FAILED rc %d", rc);
        });
    // aic_sample_luminance
    struct RayCase { const char *what; aic_ctx *c; int layer; uint32_t n; const void *rays; uint32_t flags; void *out; };
    const RayCase ray_cases[] = {
        {"no context", nullptr, 0, 10, rays.data(), 0, lum.data()},
        {"no such layer", c, 2, 10, rays.data(), 0, lum.data()},
        {"no rays", c, 0, 10, nullptr, 0, lum.data()},
        {"no out", c, 0, 10, rays.data(), 0, nullptr},
        {"unknown flag", c, 0, 10, rays.data(), 1, lum.data()},
        {"unknown flag beside AIC_RAYS_DEVICE", c, 0, 10, d_a, AIC_RAYS_DEVICE | 128u, d_b},
        {"unknown flag with n = 0", c, 0, 0, nullptr, 2, nullptr},
        {"too many rays", c, 0, (1u << 20) + 1u, rays.data(), 0, lum.data()},
        {"a layer with no space", c, AIC_LAYER_UI, 10, rays.data(), 0, lum.data()},
        {"a layer with no space, n = 0", c, AIC_LAYER_UI, 0, nullptr, 0, nullptr},
        {"device rays off by 8", c, 0, 10, d_a + 8, AIC_RAYS_DEVICE, d_b},
        {"device out off by 2", c, 0, 10, d_a, AIC_RAYS_DEVICE, d_b + 2},
    };
    for (const RayCase &k : ray_cases)
        rejection(std::string("luminance: ") + k.what, [&] {
            if (luminance(k.c, k.layer, k.n, (const double *)k.rays, 40, k.flags, (float *)k.out) != AIC_ERR_INVALID) rec("FAILED not refused");
        });
    // ... and aic_cursor_raycast's, whose checks are the same code (cursor_raycast_record.cpp has them with what follows each)
    const RayCase cursor_cases[] = {
        {"no context", nullptr, 0, 10, rays.data(), 0, host_out.data()},
        {"no such layer", c, 2, 10, rays.data(), 0, host_out.data()},
        {"no rays", c, 0, 10, nullptr, 0, host_out.data()},
        {"no out", c, 0, 10, rays.data(), 0, nullptr},
        {"unknown flag", c, 0, 10, rays.data(), 1, host_out.data()},
        {"too many rays", c, 0, (1u << 20) + 1u, rays.data(), 0, host_out.data()},
        {"a layer with no space", c, AIC_LAYER_UI, 10, rays.data(), 0, host_out.data()},
        {"device rays off by 4", c, 0, 10, d_a + 4, AIC_RAYS_DEVICE, d_b},
        {"device out off by 4", c, 0, 10, d_a, AIC_RAYS_DEVICE, d_b + 4},
    };
    for (const RayCase &k : cursor_cases)
        rejection(std::string("cursor: ") + k.what, [&] {
            if (cursor(k.c, k.layer, k.n, (const double *)k.rays, 6.0, k.flags, (aic_cursor_hit *)k.out) != AIC_ERR_INVALID) rec("FAILED not refused");
        });
    rejection("cursor: NaN maximum_distance", [&] { cursor(c, 0, 10, rays.data(), std::nan(""), 0, (aic_cursor_hit *)host_out.data()); });
    // aic_pick_stale
    struct StaleCase { const char *what; aic_ctx *c; aic_stale_desc d; bool no_desc; const void *src; const void *order; void *out; bool no_info; };
    const aic_stale_desc sd = stale_desc(8, 8, 10, 5, one, AIC_STALE_DEPTH_TEST);
    auto edit = [](aic_stale_desc d, const std::function<void(aic_stale_desc &)> &e) { e(d); return d; };
    static const std::vector<aic_stale_rect> x_out = {rect(3, 0, 2, 8)}, y_out = {rect(0, 3, 8, 2)}, x_far = {rect(0, 0, 9, 8)}, y_far = {rect(0, 0, 8, 9)}, nan_d = {rect(0, 0, 8, 8, nan)};
    const StaleCase stale_cases[] = {
        {"no context", nullptr, sd, false, d_a, d_b, d_c, false},
        {"no desc", c, sd, true, d_a, d_b, d_c, false},
        {"no info", c, sd, false, d_a, d_b, d_c, true},
        {"too wide", c, edit(sd, [](aic_stale_desc &d) { d.width = 65536; }), false, d_a, d_b, d_c, false},
        {"too high", c, edit(sd, [](aic_stale_desc &d) { d.height = 65536; }), false, d_a, d_b, d_c, false},
        {"unknown flag", c, edit(sd, [](aic_stale_desc &d) { d.flags = 2; }), false, d_a, d_b, d_c, false},
        {"too many picks", c, edit(sd, [&](aic_stale_desc &d) { d.n = too_many; }), false, d_a, d_b, d_c, false},
        {"no list to write to", c, sd, false, d_a, d_b, nullptr, false},
        {"out off by 2", c, sd, false, d_a, d_b, d_c + 2, false},
        {"order off by 2", c, sd, false, d_a, d_b + 2, d_c, false},
        {"frame off by 4", c, sd, false, d_a + 4, d_b, d_c, false},
        {"an empty frame", c, edit(sd, [](aic_stale_desc &d) { d.width = 0; d.n_rects = 0; d.rects = nullptr; }), false, d_a, d_b, d_c, false},
        {"too many rectangles", c, edit(sd, [](aic_stale_desc &d) { d.n_rects = AIC_STALE_MAX_RECTS + 1u; }), false, d_a, d_b, d_c, false},
        {"no rectangles", c, edit(sd, [](aic_stale_desc &d) { d.rects = nullptr; }), false, d_a, d_b, d_c, false},
        {"a rectangle with x0 > x1", c, edit(sd, [](aic_stale_desc &d) { d.rects = x_out.data(); }), false, d_a, d_b, d_c, false},
        {"a rectangle with y0 > y1", c, edit(sd, [](aic_stale_desc &d) { d.rects = y_out.data(); }), false, d_a, d_b, d_c, false},
        {"a rectangle past the width", c, edit(sd, [](aic_stale_desc &d) { d.rects = x_far.data(); }), false, d_a, d_b, d_c, false},
        {"a rectangle past the height", c, edit(sd, [](aic_stale_desc &d) { d.rects = y_far.data(); }), false, d_a, d_b, d_c, false},
        {"a NaN dmin", c, edit(sd, [](aic_stale_desc &d) { d.rects = nan_d.data(); }), false, d_a, d_b, d_c, false},
        {"no frame to test the depths of", c, sd, false, nullptr, d_b, d_c, false},
    };
    for (const StaleCase &k : stale_cases)
        rejection(std::string("stale: ") + k.what, [&] {
            if (stale(k.c, k.no_desc ? nullptr : &k.d, k.src, (const uint32_t *)k.order, (uint32_t *)k.out, !k.no_info) != AIC_ERR_INVALID) rec("FAILED not refused");
        });
    // a frame in slot 0: the two calls that use its stream refuse; the ray queries do not (scenario "in flight")
    scenario("rejections: a frame is submitted to slot 0", [] { submit(c, 0, frame_out); rec_state(c); }, false);
    rejection("busy: pixels", [&] { pixels(c, &ok, 10, list.data(), 0, host_out.data(), nullptr); });
    rejection("busy: pixels, a device list", [&] { pixels(c, &ok, 10, (const uint32_t *)d_a, D, d_b, nullptr); });
    rejection("busy: stale", [&] { stale(c, &sd, d_a, (const uint32_t *)d_b, (uint32_t *)d_c); });
    rejection("busy: stale, n = 0", [&] { const aic_stale_desc e = edit(sd, [](aic_stale_desc &d) { d.n = 0; }); stale(c, &e, d_a, (const uint32_t *)d_b, (uint32_t *)d_c); });
    scenario("rejections: the frame is waited for and every call runs", [&] {
        aic_frame_info info;
        rec_rc(c, "aic_render_wait", aic_render_wait(c, 0, &info));
        if (pixels(c, &ok, 10, list.data(), 0, host_out.data(), nullptr) != AIC_OK) rec("FAILED aic_trace_pixels after the rejections");
        if (luminance(c, 0, 10, rays.data(), 40, 0, lum.data()) != AIC_OK) rec("FAILED aic_sample_luminance after the rejections");
        if (cursor(c, 0, 10, rays.data(), 6.0, 0, (aic_cursor_hit *)host_out.data()) != AIC_OK) rec("FAILED aic_cursor_raycast after the rejections");
        if (stale(c, &sd, d_a, (const uint32_t *)d_b, (uint32_t *)d_c) != AIC_OK) rec("FAILED aic_pick_stale after the rejections");
        for (char *p : {d_a, d_b, d_c, frame_out}) (void)hipFree(p);
        aic_destroy(c);
    }, false);
}

// ---- every runtime call and launcher of one good call fails in turn, each on a fresh context; the same call is then made again on that context
char *d_a, *d_b, *d_c;  // the caller's device buffers of a scenario with a device list: made before the failure is armed
void failures(const std::string &name, bool device_buffers, const std::function<int(aic_ctx *)> &call) {
    static const char *fns[] = {"hipSetDevice", "hipMalloc", "hipHostMalloc", "hipMemcpyAsync", "hipMemcpy", "hipMemsetAsync", "hipStreamCreateWithFlags", "hipStreamSynchronize",
                                "hipStreamWaitEvent", "hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime", "hipGetLastError", "light_visible_bits",
                                "launch_sample_luminance", "launch_cursor_raycast", "launch_pick_stale"};
    auto run = [&](const char *fn, int nth) {  // fn == nullptr: the good call
        aic_ctx *c = make_ctx();
        if (device_buffers) { d_a = (char *)dev(kW * kH * 12); d_b = (char *)dev(kW * kH * 12); d_c = (char *)dev(70 * sizeof(aic_pixel_aux)); }
        bool reached = false;
        if (fn) {
            const int before = fake_calls(fn);
            fake_fail(fn, nth);
            const int rc = call(c);
            reached = fake_calls(fn) - before > nth;
            // (a failed clearing of the counters behind a frame is not the frame's failure: the next frame clears them itself)
            if (reached && rc == AIC_OK && std::strcmp(fn, "hipMemsetAsync")) rec("FAILED the failing call returned AIC_OK");
            if (reached) rec("-- the same call again");
        }
        if (!fn || reached) {  // (a failure that was not reached stays armed: nothing more is called)
            const int rc = call(c);
            if (!fn && rc != AIC_OK) rec("FAILED the good call");
        }
        if (device_buffers)
            for (char *p : {d_a, d_b, d_c}) (void)hipFree(p);
        aic_destroy(c);
        return reached;
    };
    scenario("failures: " + name + ", the good call", [&] { run(nullptr, 0); });
    for (const char *fn : fns)
        for (int nth = 0;; nth++) {
            bool reached = false;
            scenario("failures: " + name + " " + fn + str({nth}), [&] { reached = run(fn, nth); });
            if (!reached) break;
        }
}

void all_failures() {
    static std::vector<uint32_t> list = pixel_list(70);
    static std::vector<char> host_out(70 * 144);
    static std::vector<aic_pixel_aux> hits(70);
    static std::vector<double> rays(6 * 70, 0.25);
    static const std::vector<aic_stale_rect> one = {rect(1, 1, 30, 30)};
    failures("pixels 0", false, [&](aic_ctx *c) { const aic_frame_desc f = frame(kW, kH, AIC_FRAME_OUT_SPLIT); return pixels(c, &f, 70, list.data(), 0, host_out.data(), hits.data()); });
    failures("pixels 1", true, [&](aic_ctx *c) {
        const aic_frame_desc f = frame(kW, kH, AIC_FRAME_OUT_SPLIT);
        return pixels(c, &f, 70, (const uint32_t *)d_a, AIC_PIXELS_DEVICE | AIC_PIXELS_IN_PLACE, d_b, (aic_pixel_aux *)d_c);
    });
    failures("luminance 0", false, [&](aic_ctx *c) { return luminance(c, 0, 70, rays.data(), 40, 0, (float *)host_out.data()); });
    failures("luminance 1", true, [&](aic_ctx *c) { return luminance(c, 0, 70, (const double *)d_a, 40, AIC_RAYS_DEVICE, (float *)d_b); });
    failures("cursor 0", false, [&](aic_ctx *c) { return cursor(c, 0, 70, rays.data(), 6.0, 0, (aic_cursor_hit *)host_out.data()); });
    failures("cursor 1", true, [&](aic_ctx *c) { return cursor(c, 0, 70, (const double *)d_a, 6.0, AIC_RAYS_DEVICE, (aic_cursor_hit *)d_b); });
    failures("stale looked at", true, [&](aic_ctx *c) { const aic_stale_desc d = stale_desc(kW, kH, 70, 30, one, AIC_STALE_DEPTH_TEST); return stale(c, &d, d_a, (const uint32_t *)d_b, (uint32_t *)d_c); });
    failures("stale not looked at", true, [&](aic_ctx *c) { const aic_stale_desc d = stale_desc(kW, kH, 70, 0, one); return stale(c, &d, nullptr, nullptr, (uint32_t *)d_c); });
}

}  // namespace

int main() {
    shapes();
    in_flight();
    rejections();
    all_failures();
    fake_reset();
    rec("total: %d scenarios", n_scenarios);
    return 0;
}
