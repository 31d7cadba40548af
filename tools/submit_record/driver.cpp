// driver.cpp -- drives the host side of the C ABI through a fixed list of frame-path scenarios against the recording fake (fake_hip.cpp) and prints the
// record: every runtime call and launch, each call's return code and message, what aic_frame_info reports and the slot's state afterwards. Two builds of
// the host code make the same calls exactly when their records are byte-identical (build.sh, tests/test_submit_record_cpu.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <functional>
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

// a context with an 8 x 8 x 8 world (and UI) space of two blocks; the kernels never run, so its contents do not matter
aic_ctx *make_ctx(bool ui, int antialiasing = 0, int lighting = 3, float bloom_intensity = 0.125f) {
    int st = 0;
    aic_ctx *c = aic_create(0, &st);
    static const std::vector<uint16_t> cubes(512, 1);
    static const std::vector<uint8_t> light(512 * 4, 0);
    static const float palette[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.5f, 0.5f, 1.f, 0, 0, 0, 0};
    aic_block_desc blocks[2];
    std::memset(blocks, 0, sizeof(blocks));
    for (int i = 0; i < 2; i++) { blocks[i].resolution = 1; blocks[i].pal_off = (uint32_t)i; blocks[i].pal_len = 1; blocks[i].flags = AIC_BLOCK_ONE | (i ? 0u : AIC_BLOCK_AIR); }
    aic_space_desc s;
    std::memset(&s, 0, sizeof(s));
    s.size[0] = s.size[1] = s.size[2] = 8;
    static const uint16_t voxels[1] = {0};
    s.block_index = cubes.data(); s.light = light.data(); s.n_blocks = 2; s.blocks = blocks; s.voxels = voxels; s.n_voxels = 1; s.palette = palette; s.n_palette = 2;
    for (int layer = 0; layer <= (ui ? 1 : 0); layer++) {
        if (aic_upload_space(c, layer, &s) != AIC_OK) rec("aic_upload_space FAILED : %s", aic_last_error(c));
        aic_options o = c->layers[layer].opt;
        o.antialiasing = antialiasing; o.lighting = lighting; o.bloom_intensity = bloom_intensity;
        aic_set_options(c, layer, &o);
    }
    return c;
}

aic_frame_desc frame(uint32_t w, uint32_t h, uint32_t flags = 0, uint32_t tuning = 0, double eye_x = 0.0) {
    aic_frame_desc f;
    std::memset(&f, 0, sizeof(f));
    f.width = w; f.height = h; f.flags = flags; f.tuning = tuning;
    for (int i = 0; i < 4; i++) f.world.inverse_projection_view[5 * i] = f.ui.inverse_projection_view[5 * i] = 1.0;
    f.world.inverse_projection_view[12] = eye_x;  // (beyond a quarter cube: cameras_close says no)
    f.world.exposure = 1.5f; f.ui.exposure = 0.75f;
    return f;
}
size_t frame_bytes(const aic_frame_desc &f) {
    const size_t px = (f.flags & (AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) ? 16 : ((f.flags & AIC_FRAME_OUT_SPLIT) ? 12 : 4);
    return (size_t)f.width * f.height * px;
}

void rec_result(aic_ctx *c, const char *call, int rc, uint32_t slot, const aic_frame_info *info = nullptr) {
    rec("%s rc %d%s%s", call, rc, rc ? " : " : "", rc ? aic_last_error(c) : "");
    if (info)
        rec("  info cubes %llu outer %llu inner %llu hits %llu light %llu kernel_ms %a rows %u flaws %u variant %u tile_queues %u", (unsigned long long)info->cubes_traced,
            (unsigned long long)info->n_outer, (unsigned long long)info->n_inner, (unsigned long long)info->n_hits, (unsigned long long)info->n_light, info->kernel_ms,
            info->rows_rendered, info->flaws, info->variant, info->tile_queues);
    const aic_ctx::FrameSlot &fs = c->slots[slot];
    rec("  slot %u busy %d diag %d variant %u tile_queues %u flaws %u local_rows %u npix %zu n_sub %u light_used %s %s static %d key %u %u %u %u %u %u edges %ux%u aux_records %llu", slot,
        (int)fs.busy, (int)fs.diag, fs.variant, fs.tile_queues, fs.flaws, fs.local_rows, fs.npix, fs.n_sub, rec_ptr(fs.light_used[0]).c_str(), rec_ptr(fs.light_used[1]).c_str(),
        (int)fs.static_ready, fs.static_key[0], fs.static_key[1], fs.static_key[2], fs.static_key[3], fs.static_key[4], fs.static_key[5], fs.edges_w, fs.edges_h,
        (unsigned long long)c->aux_records);
    for (uint32_t j = 0; j < fs.n_sub && j < kMaxSub; j++) {
        const aic_ctx::SubSlot &sb = fs.sub[j];
        rec("  sub %u counters_clean %d cost_clean_n %zu record_ready %d order_key %u %u %u %u %u %u cost_sig %u %u %u %u cost_cam12 %a", j, (int)sb.counters_clean, sb.cost_clean_n,
            (int)sb.record_ready, sb.order_key[0], sb.order_key[1], sb.order_key[2], sb.order_key[3], sb.order_key[4], sb.order_key[5], sb.cost_sig[0], sb.cost_sig[1], sb.cost_sig[2],
            sb.cost_sig[3], sb.cost_cam[12]);
    }
}

// one scenario: ordinals from zero, everything it allocates freed at its end
void scenario(const std::string &name, const std::function<void()> &body) {
    fake_reset();
    rec("== %s", name.c_str());
    n_scenarios++;
    body();
}

// ---- the ways a frame is submitted
void render(aic_ctx *c, const aic_frame_desc &f, bool to_device) {
    aic_frame_info info;
    if (to_device) {
        void *out = dev(frame_bytes(f));
        rec_result(c, "aic_render", aic_render(c, &f, out, 1, &info), 0, &info);
        (void)hipFree(out);
    } else {
        std::vector<char> out(frame_bytes(f) + 1);
        rec_result(c, "aic_render", aic_render(c, &f, out.data(), 0, &info), 0, &info);
    }
}
void submit_wait(aic_ctx *c, const aic_frame_desc &f, uint32_t slot, void *out) {
    aic_frame_info info;
    rec_result(c, "aic_render_submit", aic_render_submit(c, &f, out, slot), slot);
    rec_result(c, "aic_render_wait", aic_render_wait(c, slot, &info), slot, &info);
}
void batch_wait(aic_ctx *c, uint32_t k, const aic_frame_desc &f, uint32_t slot, double eye_x = 0.0) {
    std::vector<aic_frame_desc> frames(k, f);
    std::vector<void *> outs(k);
    for (uint32_t j = 0; j < k; j++) { frames[j].world.inverse_projection_view[12] = eye_x + 0.01 * j; frames[j].backdrop[3] = j & 1 ? 1.f : 0.f; outs[j] = dev(frame_bytes(f)); }
    std::vector<aic_frame_info> infos(k);
    rec_result(c, "aic_render_submit_batch", aic_render_submit_batch(c, k, frames.data(), outs.data(), slot), slot);
    rec_result(c, "aic_render_wait_batch", aic_render_wait_batch(c, slot, k, infos.data()), slot, &infos[k - 1]);
    for (void *p : outs) (void)hipFree(p);
}
std::string str(std::initializer_list<long> v) { std::string s; for (long x : v) s += " " + std::to_string(x); return s; }

const uint32_t kFlags[] = {0, AIC_FRAME_COUNTERS, AIC_FRAME_AUX, AIC_FRAME_PIXEL_CENTERS, AIC_FRAME_OUT_LINEAR, AIC_FRAME_OUT_COLORBUF, AIC_FRAME_NO_FEEDBACK, AIC_FRAME_OUT_SPLIT, AIC_FRAME_BLOOM};
const uint32_t kSizes[][2] = {{0, 0}, {1, 1}, {8, 8}, {9, 17}, {640, 360}, {1920, 1080}, {3840, 2160}};

void whole_frames() {
    // every flag under every scene option, two frames each (the second finds the slot as the first left it)
    for (uint32_t flags : kFlags)
        for (int ui = 0; ui < 2; ui++)
            for (int aa : {0, 2})
                for (int lighting : {3, 5})
                    for (float bloom : {0.f, 0.125f}) {
                        if (bloom == 0.f && (flags != AIC_FRAME_BLOOM || aa || lighting != 3)) continue;  // (intensity 0: the bloom flag alone)
                        scenario("render flags" + str({flags, ui, aa, lighting, (long)(bloom * 1000)}), [&] {
                            aic_ctx *c = make_ctx(ui, aa, lighting, bloom);
                            for (int n = 0; n < 2; n++) render(c, frame(9, 17, flags), n == 0);
                            aic_destroy(c);
                        });
                    }
    // every size, whole and as part 1 of 4, rendered and streamed
    for (const auto &wh : kSizes)
        for (uint32_t parts : {1u, 4u})
            scenario("sizes" + str({wh[0], wh[1], parts}), [&] {
                aic_ctx *c = make_ctx(false);
                aic_frame_desc f = frame(wh[0], wh[1]);
                if (parts > 1) f.partition = aic_partition{8, parts, 1, 0};
                render(c, f, true);
                if (wh[0] <= 640) render(c, f, false);
                void *out = dev(frame_bytes(f));
                submit_wait(c, f, 1, out);
                (void)hipFree(out);
                aic_destroy(c);
            });
    // tuning: variant x queues x super-block shift, with and without antialiasing (the exchanging variants' ray_cold)
    for (uint32_t variant : {AIC_VARIANT_AUTO, AIC_VARIANT_PLAIN, AIC_VARIANT_EXCHANGING})
        for (uint32_t queues : {0u, 1u, 8u})
            for (uint32_t super : {0u, 3u})
                for (int aa : {0, 2})
                    scenario("tuning" + str({variant, queues, super, aa}), [&] {
                        aic_ctx *c = make_ctx(true, aa);
                        const uint32_t tuning = (variant << AIC_TUNE_VARIANT_SHIFT) | (queues << AIC_TUNE_QUEUES_SHIFT) | (super << AIC_TUNE_SUPER_SHIFT);
                        for (const auto &wh : {kSizes[3], kSizes[4], kSizes[5]}) render(c, frame(wh[0], wh[1], 0, tuning), true);
                        aic_destroy(c);
                    });
}

void streamed_frames() {
    // the part-grid rule: a streamed frame beside 0, 1, 3 and 5 others in flight
    for (const auto &wh : {kSizes[4], kSizes[5], kSizes[6]})
        for (uint32_t others : {0u, 1u, 3u, 5u})
            scenario("streamed" + str({wh[0], wh[1], others}), [&] {
                aic_ctx *c = make_ctx(false);
                const aic_frame_desc f = frame(wh[0], wh[1]), small = frame(8, 8);
                void *out = dev(frame_bytes(f));
                for (uint32_t i = 0; i < others; i++) rec_result(c, "aic_render_submit", aic_render_submit(c, &small, out, 8 + i), 8 + i);  // (slots past the eighth: made on first use)
                submit_wait(c, f, 2, out);
                for (uint32_t i = 0; i < others; i++) rec_result(c, "aic_render_wait", aic_render_wait(c, 8 + i, nullptr), 8 + i);
                (void)hipFree(out);
                aic_destroy(c);
            });
    for (uint32_t k : {1u, 2u, 4u, 8u})
        for (uint32_t flags : {0u, (uint32_t)AIC_FRAME_COUNTERS, (uint32_t)AIC_FRAME_BLOOM, (uint32_t)AIC_FRAME_OUT_SPLIT, (uint32_t)AIC_FRAME_NO_FEEDBACK})
            for (int ui = 0; ui < 2; ui++)
                scenario("batch" + str({k, flags, ui}), [&] {
                    aic_ctx *c = make_ctx(ui, ui ? 2 : 0);
                    for (const auto &wh : {kSizes[3], kSizes[4]}) batch_wait(c, k, frame(wh[0], wh[1], flags), 3);
                    aic_destroy(c);
                });
}

// three frames on one slot: the same camera; a camera moved past cameras_close; a changed shape and back
void sequences() {
    const double eyes[3][3] = {{0, 0, 0}, {0, 5, 5}, {0, 0, 0}};
    const uint32_t shapes[3][3] = {{640, 640, 640}, {640, 640, 640}, {640, 320, 640}};
    const char *names[3] = {"same camera", "moved camera", "changed shape and back"};
    for (int s = 0; s < 3; s++)
        for (int mode = 0; mode < 3; mode++)
            scenario(std::string("sequence ") + names[s] + str({mode}), [&] {
                aic_ctx *c = make_ctx(mode == 1);
                void *out = dev(640 * 360 * 4);
                for (int n = 0; n < 3; n++) {
                    const aic_frame_desc f = frame(shapes[s][n], 360, 0, 0, eyes[s][n]);
                    rec("-- frame %d", n);
                    if (mode == 0) render(c, f, true);
                    else if (mode == 1) submit_wait(c, f, 1, out);
                    else batch_wait(c, 2, f, 1, eyes[s][n]);
                }
                (void)hipFree(out);
                aic_destroy(c);
            });
}

void trace_patches(aic_ctx *c, uint32_t n, uint32_t flags, bool aux) {
    const std::vector<double> rects((size_t)n * 4, 0.25);
    std::vector<char> out((size_t)n * 16);
    std::vector<aic_pixel_aux> hits(n);
    const aic_frame_desc f = frame(64, 64, flags);
    aic_frame_info info;
    rec_result(c, "aic_trace_patches", aic_trace_patches(c, &f, n, rects.data(), out.data(), aux ? hits.data() : nullptr, &info), 0, &info);
}
void trace_rays(aic_ctx *c, int layer, uint32_t n, uint32_t flags, bool aux) {
    aic_frame_info info;
    if (flags & AIC_RAYS_DEVICE) {
        void *rays = dev((size_t)n * 48), *out = dev((size_t)n * 16), *hits = aux ? dev((size_t)n * sizeof(aic_pixel_aux)) : nullptr;
        rec_result(c, "aic_trace_rays", aic_trace_rays(c, layer, n, (const double *)rays, flags, 1.25f, out, (aic_pixel_aux *)hits, &info), 0, &info);
        (void)hipFree(rays); (void)hipFree(out);
        if (hits) (void)hipFree(hits);
    } else {
        const std::vector<double> rays((size_t)n * 6, 1.0);
        std::vector<char> out((size_t)n * 16);
        std::vector<aic_pixel_aux> hits(n);
        rec_result(c, "aic_trace_rays", aic_trace_rays(c, layer, n, rays.data(), flags, 1.25f, out.data(), aux ? hits.data() : nullptr, &info), 0, &info);
    }
}
void ortho(aic_ctx *c, int layer, bool to_device) {
    uint32_t w = 0, h = 0;
    aic_frame_info info;
    void *out = to_device ? dev(64 * 64 * 4) : std::malloc(64 * 64 * 4);
    rec_result(c, "aic_render_orthographic", aic_render_orthographic(c, layer, 2, out, to_device, &w, &h, &info), 0, &info);
    rec("  image %ux%u", w, h);
    if (to_device) (void)hipFree(out); else std::free(out);
}

void other_traces() {
    for (uint32_t n : {1u, 5000u})
        for (uint32_t flags : {0u, (uint32_t)AIC_FRAME_OUT_LINEAR, (uint32_t)AIC_FRAME_COUNTERS})
            for (int aux = 0; aux < 2; aux++)
                scenario("patches" + str({n, flags, aux}), [&] { aic_ctx *c = make_ctx(true, 2); trace_patches(c, n, flags, aux); trace_patches(c, n, flags, aux); aic_destroy(c); });
    for (uint32_t device : {0u, (uint32_t)AIC_RAYS_DEVICE})
        for (uint32_t no_sky : {0u, (uint32_t)AIC_RAYS_NO_SKY})
            for (int layer = 0; layer < 2; layer++)
                for (int aux = 0; aux < 2; aux++)
                    scenario("rays" + str({device, no_sky, layer, aux}), [&] {
                        aic_ctx *c = make_ctx(true, 2);
                        for (uint32_t n : {1u, 5000u}) trace_rays(c, layer, n, device | no_sky | (aux ? AIC_FRAME_OUT_COLORBUF : 0u), aux);
                        aic_destroy(c);
                    });
    for (int layer = 0; layer < 2; layer++)
        for (int to_device = 0; to_device < 2; to_device++)
            scenario("ortho" + str({layer, to_device}), [&] { aic_ctx *c = make_ctx(true, 2); ortho(c, layer, to_device); ortho(c, layer, to_device); aic_destroy(c); });
    scenario("ortho image size", [] {
        const int32_t lo[3] = {-1, 2, 3}, size[3] = {4, 5, 6}, bad[3] = {4, -5, 6};
        uint32_t w = 0, h = 0;
        rec("aic_ortho_image_size rc %d %ux%u", aic_ortho_image_size(lo, size, 4, &w, &h), w, h);
        rec("aic_ortho_image_size rc %d", aic_ortho_image_size(lo, bad, 4, &w, &h));
        rec("aic_ortho_image_size rc %d", aic_ortho_image_size(lo, size, 3, &w, &h));
    });
}

// ---- every failure of the frame path
void argument_failures() {
    scenario("failures: arguments", [] {
        aic_ctx *c = make_ctx(true);
        void *out = dev(64 * 64 * 16);
        aic_frame_info info;
        auto bad = [&](const char *what, aic_frame_desc f, void *o = nullptr, bool host = false) {
            rec("-- %s", what);
            rec_result(c, "aic_render", aic_render(c, &f, o, host ? 0 : 1, &info), 0);
        };
        auto with = [](aic_frame_desc f, std::function<void(aic_frame_desc &)> edit) { edit(f); return f; };
        rec_result(c, "aic_render", aic_render(c, nullptr, out, 1, nullptr), 0);
        bad("part >= n_parts", with(frame(8, 8), [](aic_frame_desc &f) { f.partition = aic_partition{8, 2, 2, 0}; }), out);
        bad("part >= n_parts, host target", with(frame(8, 8), [](aic_frame_desc &f) { f.partition = aic_partition{8, 2, 2, 0}; }), &info, true);
        bad("bloom with linear", frame(8, 8, AIC_FRAME_BLOOM | AIC_FRAME_OUT_LINEAR), out);
        bad("bloom of a part", with(frame(8, 32, AIC_FRAME_BLOOM), [](aic_frame_desc &f) { f.partition = aic_partition{8, 2, 1, 0}; }), out);
        bad("split with colorbuf", frame(8, 8, AIC_FRAME_OUT_SPLIT | AIC_FRAME_OUT_COLORBUF), out);
        bad("null output", frame(8, 8), nullptr);
        bad("split buffer off by 4", frame(8, 8, AIC_FRAME_OUT_SPLIT), (char *)out + 4);
        bad("too wide", frame(65536, 1), out);
        bad("negative exposure", with(frame(8, 8), [](aic_frame_desc &f) { f.world.exposure = -1.f; }), out);
        bad("NaN UI exposure", with(frame(8, 8), [](aic_frame_desc &f) { f.ui.exposure = NAN; }), out);
        const aic_frame_desc f = frame(8, 8), g = frame(8, 9);
        const aic_frame_desc pair[2] = {f, g};
        void *outs[2] = {out, out};
        rec_result(c, "aic_render_submit", aic_render_submit(c, &f, out, AIC_MAX_IN_FLIGHT), 0);
        rec_result(c, "aic_render_submit_batch", aic_render_submit_batch(c, 2, nullptr, outs, 0), 0);
        rec_result(c, "aic_render_submit_batch", aic_render_submit_batch(c, 3, pair, outs, 0), 0);
        rec_result(c, "aic_render_submit_batch", aic_render_submit_batch(c, 2, pair, outs, 0), 0);
        rec_result(c, "aic_render_wait", aic_render_wait(c, AIC_MAX_IN_FLIGHT, &info), 0);
        rec_result(c, "aic_render_wait_batch", aic_render_wait_batch(c, 0, 2, nullptr), 0);
        // slot 0 busy: every synchronous entry point refuses
        rec_result(c, "aic_render_submit", aic_render_submit(c, &f, out, 0), 0);
        rec_result(c, "aic_render_submit", aic_render_submit(c, &f, out, 0), 0);
        rec_result(c, "aic_render_submit_batch", aic_render_submit_batch(c, 1, &f, outs, 0), 0);
        bad("slot 0 busy", f, out);
        trace_patches(c, 4, 0, false);
        trace_rays(c, 0, 4, 0, false);
        ortho(c, 0, true);
        rec_result(c, "aic_render_wait", aic_render_wait(c, 0, &info), 0, &info);
        // patches, rays and orthographic views: their own checks
        rec_result(c, "aic_trace_patches", aic_trace_patches(c, &f, 4, nullptr, out, nullptr, &info), 0);
        rec_result(c, "aic_trace_patches", aic_trace_patches(c, &f, 0, nullptr, nullptr, nullptr, &info), 0);
        trace_patches(c, 4, AIC_FRAME_BLOOM, false);
        trace_patches(c, 4, AIC_FRAME_OUT_SPLIT, false);
        const double ray[6] = {0, 0, 0, 1, 0, 0};
        auto rays = [&](const char *what, int layer, uint32_t n, const void *r, uint32_t flags, float exposure, void *o, void *aux) {
            rec("-- rays: %s", what);
            rec_result(c, "aic_trace_rays", aic_trace_rays(c, layer, n, (const double *)r, flags, exposure, o, (aic_pixel_aux *)aux, &info), 0);
        };
        rays("bad layer", 2, 1, ray, 0, 1.f, out, nullptr);
        rays("bloom", 0, 1, ray, AIC_FRAME_BLOOM, 1.f, out, nullptr);
        rays("linear and colorbuf", 0, 1, ray, AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF, 1.f, out, nullptr);
        rays("NaN exposure", 0, 1, ray, 0, NAN, out, nullptr);
        rays("none", 0, 0, nullptr, 0, 1.f, nullptr, nullptr);
        rays("device rays off by 8", 0, 1, (char *)out + 8, AIC_RAYS_DEVICE, 1.f, out, nullptr);
        aic_clear_space(c, AIC_LAYER_UI);
        rays("no space", 1, 1, ray, 0, 1.f, out, nullptr);
        rec_result(c, "aic_render_orthographic", aic_render_orthographic(c, 1, 2, out, 1, nullptr, nullptr, &info), 0);
        rec_result(c, "aic_render_orthographic", aic_render_orthographic(c, 0, 3, out, 1, nullptr, nullptr, &info), 0);
        rec_result(c, "aic_render_orthographic", aic_render_orthographic(c, 0, 2, nullptr, 1, nullptr, nullptr, &info), 0);  // size query
        (void)hipFree(out);
        aic_destroy(c);
    });
    // more items than a batch image holds (2048 x 65535): refused before anything is read
    scenario("failures: batch too long", [] {
        aic_ctx *c = make_ctx(false);
        const aic_frame_desc f = frame(8, 8);
        const uint32_t n = 2048u * 65535u + 1u;
        char one[64];
        rec_result(c, "aic_trace_patches", aic_trace_patches(c, &f, n, (const double *)one, one, nullptr, nullptr), 0);
        rec_result(c, "aic_trace_rays", aic_trace_rays(c, 0, n, (const double *)one, 0, 1.f, one, nullptr, nullptr), 0);
        aic_destroy(c);
    });
    scenario("failures: a wave gave up", [] {
        aic_ctx *c = make_ctx(false);
        fake_bail(true);
        render(c, frame(9, 17), true);
        fake_bail(false);
        render(c, frame(9, 17), true);
        aic_destroy(c);
    });
}

// Every runtime call a scenario makes fails in turn, each in a context of its own: the allocations ("alloc ..."), the copies, the events.
void runtime_failures(const std::string &name, bool ui, const std::function<void(aic_ctx *)> &body) {
    static const char *fns[] = {"hipMalloc", "hipHostMalloc", "hipMemcpyAsync", "hipMemcpy", "hipMemsetAsync", "hipStreamCreateWithFlags", "hipStreamSynchronize", "hipStreamWaitEvent",
                                "hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime"};
    for (const char *fn : fns)
        for (int nth = 0;; nth++) {
            bool reached = false;
            scenario("failures: " + name + " " + fn + str({nth}), [&] {
                aic_ctx *c = make_ctx(ui, 2);
                const int before = fake_calls(fn);
                fake_fail(fn, nth);
                body(c);
                reached = fake_calls(fn) - before > nth;
                aic_destroy(c);
            });
            if (!reached) break;
        }
}

void all_runtime_failures() {
    runtime_failures("frame", true, [](aic_ctx *c) {
        render(c, frame(640, 360, AIC_FRAME_OUT_SPLIT), true);
        render(c, frame(640, 360, AIC_FRAME_AUX), false);
        render(c, frame(640, 360, 0, AIC_VARIANT_EXCHANGING << AIC_TUNE_VARIANT_SHIFT), true);
    });
    runtime_failures("bloom", false, [](aic_ctx *c) { render(c, frame(9, 17, AIC_FRAME_BLOOM), true); });
    runtime_failures("streamed", false, [](aic_ctx *c) {
        void *out = dev(64 * 64 * 4);
        submit_wait(c, frame(9, 17), 9, out);
        batch_wait(c, 2, frame(9, 17), 10);
        (void)hipFree(out);
    });
    runtime_failures("patches", false, [](aic_ctx *c) { trace_patches(c, 5, 0, true); });
    runtime_failures("rays", false, [](aic_ctx *c) { trace_rays(c, 0, 5, 0, true); });
    runtime_failures("ortho", false, [](aic_ctx *c) { ortho(c, 0, false); });
}

}  // namespace

int main() {
    whole_frames();
    streamed_frames();
    sequences();
    other_traces();
    argument_failures();
    all_runtime_failures();
    fake_reset();
    rec("total: %d scenarios", n_scenarios);
    return 0;
}
