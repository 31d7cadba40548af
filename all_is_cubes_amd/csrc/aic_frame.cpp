// aic_frame.cpp -- the frame path of the C ABI declared in include/aic_hip.h: everything that submits a trace or waits for one.
//
// submit_frames queues the frames of one launch on a slot's stream as a sequence of named steps (DESIGN.md 4.3 "One frame, step by step"); wait_frame
// collects them. The entry points -- aic_render, aic_render_orthographic, aic_trace_patches, aic_trace_rays, aic_trace_pixels, aic_render_submit(_batch),
// aic_render_wait(_batch) -- say what is traced (Traced) and where the result goes. Of aic_abi.cpp it uses what aic_ctx.h declares.
// What the listed traces (aic_trace_patches, aic_trace_rays, aic_trace_pixels) share is written once, ahead of the entry points (batch_image to
// finish_listed). Each keeps its own order of checks; the copies of its list in and of its results out stay with it too, because a failed one is reported
// by the expression that made it.
// Built with -ffp-contract=off, like the kernels: the pixel-edge table is the reference's own f64 operations (bind_pixel_edges).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/aic_hip.h"
#include "aic_bloom.h"
#include "aic_ctx.h"
#include "aic_device.h"
#include "aic_launch.h"

using namespace aic;

namespace {

// One layer as a launch sees it: the space's device buffers, its options and one of the frame's cameras.
void fill_dev_layer(const Layer &l, const aic_camera &cam, DevLayer *d) {
    std::memset(d, 0, sizeof(*d));
    d->present = l.present ? 1 : 0;
    d->pool = l.pool.p;
    d->cls = l.cls.p;
    d->n_blocks = (uint32_t)l.host_blocks.size();
    d->light = l.light.p;
    d->blocks = l.blocks.p;
    d->palette = l.palette.p;
    for (int a = 0; a < 3; a++) { d->lo[a] = l.lo[a]; d->size[a] = l.size[a]; }
    d->air_index = l.air_index;
    d->sky_kind = l.sky_kind;
    std::memcpy(d->sky, l.sky, sizeof(d->sky));
    std::memcpy(d->block_sky, l.block_sky, sizeof(d->block_sky));
    const aic_options o = l.opt_set ? l.opt : default_options();
    d->opt.fog = o.fog;
    d->opt.transparency = o.transparency;
    d->opt.threshold = o.threshold;
    d->opt.lighting = o.lighting;  // 5 = Bounce: traced as the reference does (surface.rs:119-166; aic_light_bounce.h bounce_secondary_ray)
    d->opt.bounce_samples = o.bounce_samples;
    d->opt.antialiasing = o.antialiasing;
    d->opt.debug_pixel_cost = o.debug_pixel_cost;
    d->opt.tone_mapping = o.tone_mapping;
    d->opt.maximum_intensity = o.maximum_intensity;
    d->opt.view_distance = o.view_distance;
    std::memcpy(d->inv, cam.inverse_projection_view, sizeof(d->inv));
    d->exposure = cam.exposure + 0.0f;
    d->cls_in_code = l.cls_in_code ? 1u : 0u;
}

// Do two cameras see nearly the same picture? Compares the rays through three NDC points.
bool cameras_close(const double a[16], const double b[16]) {
    auto unproject = [](const double m[16], double x, double y, double z, double out[3]) {  // euclid row-vector convention
        const double w = x * m[3] + y * m[7] + z * m[11] + m[15];
        for (int k = 0; k < 3; k++) out[k] = (x * m[k] + y * m[4 + k] + z * m[8 + k] + m[12 + k]) / w;
    };
    static const double pts[3][2] = {{0.0, 0.0}, {1.0, 1.0}, {-1.0, -1.0}};
    for (const auto &p : pts) {
        double na[3], fa[3], nb[3], fb[3];
        unproject(a, p[0], p[1], 0.0, na); unproject(a, p[0], p[1], 1.0, fa);
        unproject(b, p[0], p[1], 0.0, nb); unproject(b, p[0], p[1], 1.0, fb);
        double da[3], db[3], la = 0, lb = 0, dot = 0, move = 0;
        for (int k = 0; k < 3; k++) {
            da[k] = fa[k] - na[k]; db[k] = fb[k] - nb[k];
            la += da[k] * da[k]; lb += db[k] * db[k]; dot += da[k] * db[k];
            move += (na[k] - nb[k]) * (na[k] - nb[k]);
        }
        if (!(la > 0) || !(lb > 0)) return false;
        if (!(dot / std::sqrt(la * lb) >= 0.99985)) return false;  // cos(1 degree)
        if (!(move <= 0.0625)) return false;
    }
    return true;
}

// What one launch traces. Whole frames (k of them: all pointers null) go through the pixel grid, the tile queues and the cost feedback; the other four replace the
// camera (a pixel list: the pixel grid) and take none of those. A patch batch (aic_trace_patches): n NDC rectangles on the device, one per pixel of the batch's image. Orthographic views
// (aic_render_orthographic): ortho_n views on the device. A ray batch (aic_trace_rays): n world-space rays on the device replace the camera; the space traced is
// the launch's world layer (Traced::world_seat names it, as for aic_render_orthographic), labelled `layer` in first-hit records, which go to `aux_target` when the
// caller's own device buffer receives them.
struct RayBatch {
    const double *rays;
    uint32_t n;
    bool no_sky;
    uint32_t layer;
    DevAux *aux_target;
};
// A pixel list (aic_trace_pixels): n pixel indices on the device, one per pixel of the batch's image, each a pixel of the target frame of width x height, whose
// cameras, edge tables and plane layout (in_place) the launch uses; the recording variants only. First-hit records go to `aux_target` as for a ray batch.
struct PixelList {
    const uint32_t *pixels;
    uint32_t n, width, height;
    bool in_place;
    DevAux *aux_target;
};
struct Traced {
    const double *patches = nullptr;
    uint32_t n_patches = 0;
    const DevOrthoView *ortho = nullptr;
    int32_t ortho_n = 0;
    const RayBatch *rb = nullptr;
    const PixelList *px = nullptr;
    int world_seat = AIC_LAYER_WORLD;  // the layer traced as the launch's world layer (ray batches and orthographic views: the layer that holds their space)
    bool whole_frame() const { return !patches && !rb && !px && !ortho_n; }
    DevAux *aux_target() const { return rb ? rb->aux_target : (px ? px->aux_target : nullptr); }
};

// What the steps of one submit hand to each other (submit_frames is the list of steps).
struct FramePlan {
    aic_partition part;   // normalised
    uint32_t local_rows = 0;
    size_t npix = 0;      // of one frame
    bool split = false, bloom = false, diag = false, want_aux = false, ui = false;
    uint32_t flaws = 0;
    uint32_t n_tiles = 0, n_queues = 0, sb_shift = 0;  // macro tiles; XCD tile queues and their super-block shift
    uint32_t sig[4] = {0, 0, 0, 0}, order_key[6] = {0, 0, 0, 0, 0, 0};  // the frame shape a cost record describes; + queues + shift: what a tile order is made for
    bool use_feedback = false, ordered = false;
    size_t ray_cold_bytes = 0;  // trace_ray_cold_bytes for this device, if the library has exchanging variants at all
    uint32_t ray_cold_groups = 0;
    DevLayer hl[2];
    DevFrame F;
};

// A frame descriptor's partition with "no partition" (one part, or no strip height) spelled as one part of the whole height.
aic_partition normalised_partition(const aic_frame_desc &f) {
    aic_partition part = f.partition;
    if (part.n_parts <= 1 || part.strip_rows == 0) {
        part.n_parts = 1;
        part.part = 0;
        part.strip_rows = f.height ? f.height : 1;
    }
    return part;
}

// Step 1: the checks before anything is queued (the context stays as it was); the frames go to the call recorder once their buffers are known to be there.
int validate_frames(aic_ctx *c, uint32_t k, const aic_frame_desc *frames, uint32_t *const *out_devices, uint32_t slot, const Traced &what, FramePlan &P) {
    const aic_frame_desc *f = &frames[0];
    P.part = normalised_partition(*f);
    if (P.part.part >= P.part.n_parts) return fail(c, AIC_ERR_INVALID, "aic_render: partition.part >= n_parts");
    if (f->flags & AIC_FRAME_BLOOM) {
        if (f->flags & (AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) return fail(c, AIC_ERR_INVALID, "aic_render: AIC_FRAME_BLOOM is for RGBA8 output only");
        if (P.part.n_parts > 1u) return fail(c, AIC_ERR_UNSUPPORTED, "aic_render: AIC_FRAME_BLOOM needs the whole frame (partition.n_parts = 1)");
        if (!what.whole_frame()) return fail(c, AIC_ERR_UNSUPPORTED, "AIC_FRAME_BLOOM: not for patches, rays or orthographic views");
    }
    // AIC_FRAME_OUT_SPLIT (whole frames only: patch and ray batches mask the flags they pass on, orthographic views pass none)
    P.split = (f->flags & AIC_FRAME_OUT_SPLIT) != 0;
    if (P.split && (f->flags & (AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF | AIC_FRAME_BLOOM)))
        return fail(c, AIC_ERR_INVALID, "aic_render: AIC_FRAME_OUT_SPLIT excludes AIC_FRAME_OUT_LINEAR, AIC_FRAME_OUT_COLORBUF and AIC_FRAME_BLOOM");
    P.local_rows = aic_partition_rows(f->height, &P.part);
    P.npix = (size_t)f->width * P.local_rows;
    for (uint32_t j = 0; j < k; j++) {
        if (P.npix && !out_devices[j]) return fail(c, AIC_ERR_INVALID, "aic_render: output buffer is null");
        if (P.split && ((uintptr_t)out_devices[j] & 7u)) return fail(c, AIC_ERR_INVALID, "aic_render: an AIC_FRAME_OUT_SPLIT buffer starts at an 8-byte boundary");
    }
    if (!what.patches && !what.rb && !what.px)
        for (uint32_t j = 0; j < k; j++) dump_record(c, DUMP_FRAME, slot, {{&frames[j], sizeof(frames[j])}});
    if (f->width > 65535u || P.local_rows > 65535u) return fail(c, AIC_ERR_INVALID, "aic_render: frame dimensions above 65535 are not supported");
    for (uint32_t j = 0; j < k; j++)  // Camera::exposure() is a PositiveSign<f32> (camera_struct.rs:365-367)
        if (!(frames[j].world.exposure >= 0.f) || !(frames[j].ui.exposure >= 0.f)) return fail(c, AIC_ERR_INVALID, "aic_render: exposure is negative or NaN");
    return AIC_OK;
}

// Tiles per resident wave of a streamed single frame that is submitted while others are in flight.
uint32_t part_grid_tiles_per_wave(const aic_ctx *c, uint32_t slot, const DevFrame &F) {
    // A streamed frame with several tiles per resident wave (a whole 1080p frame has 7.9) that is submitted while others are in flight gets a PART of the
    // chip: a third with three others queued, a quarter from four on -- up to 32 tiles per wave, which a 4K frame has on the whole chip. Full-grid launches
    // run one behind the other and only their tails overlap; part-grid launches are resident side by side, each wave refills its lanes three or four
    // times as often before its frame runs dry, and a frame's ramp and tail are paid on a part of the chip while the others are in full swing: C2 streamed
    // 0.376 -> 0.341 ms with four frames in flight, 0.338 with eight (profiles/r06_experiments.txt R). A frame submitted with nothing else in flight (the
    // first of a stream, or a host that submits slower than the device traces) still takes the whole chip; small frames keep their four tiles per wave.
    uint32_t busy_others = 0;
    for (uint32_t i = 0; i < AIC_MAX_IN_FLIGHT; i++) busy_others += (i != slot && c->slots[i].busy && c->slots[i].npix) ? 1u : 0u;
    const uint32_t resident_waves = (uint32_t)c->n_cus * 16u;
    const uint32_t tpw_full = (F.tiles_x * F.tiles_y + resident_waves - 1u) / resident_waves;
    if (tpw_full >= 4u && busy_others > 0u) {
        const uint32_t t = tpw_full * (busy_others < 4u ? busy_others : 4u);
        return t < 32u ? t : (tpw_full > 32u ? tpw_full : 32u);
    }
    return F.tiles_per_wave;
}

// Step 2a: the layers as the launch sees them, what is traced through them, and the tile geometry. (The plan makes no HIP call and writes nothing to the slot.)
void plan_geometry(const aic_ctx *c, uint32_t k, const aic_frame_desc *f, uint32_t slot, const Traced &what, FramePlan &P) {
    DevFrame &F = P.F;
    DevLayer *hl = P.hl;
    std::memset(&F, 0, sizeof(F));
    const Layer &seated = c->layers[what.world_seat];
    fill_dev_layer(seated, f->world, &hl[0]);
    fill_dev_layer(c->layers[AIC_LAYER_UI], f->ui, &hl[1]);
    // AIC_FRAME_BLOOM: the frame is bloomed as the reference's GPU renderer blooms it (aic_bloom.hip); at intensity 0 the flag changes nothing
    const aic_options &bloom_opt = seated.opt;
    P.bloom = (f->flags & AIC_FRAME_BLOOM) && bloom_opt.bloom_intensity > 0.0f;
    if (bloom_opt.bloom_intensity != 0.0f && !P.bloom) P.flaws |= AIC_FLAW_NO_BLOOM;  // renderer.rs:293-297
    F.width = f->width;
    F.height = f->height;
    F.n_sub = k;
    // the encoder and the sampling pattern follow the WORLD camera's options (renderer.rs:283-291, 426)
    F.pixel_centers = (f->flags & AIC_FRAME_PIXEL_CENTERS) && !what.patches ? 1 : 0;
    F.out_mode = P.split ? 3 : ((f->flags & AIC_FRAME_OUT_LINEAR) ? 1 : ((f->flags & AIC_FRAME_OUT_COLORBUF) || P.bloom ? 2 : 0));  // (a bloomed frame: its ColorBuf, into the slot's scratch)
    std::memcpy(F.depth_zw, c->depth_zw, sizeof(F.depth_zw));
    F.patches = what.patches;
    F.n_patches = what.rb ? what.rb->n : (what.px ? what.px->n : what.n_patches);
    if (what.px) {
        F.pixels = what.px->pixels;
        F.px_width = what.px->width;
        F.px_height = what.px->height;
        F.px_in_place = what.px->in_place ? 1u : 0u;
    }
    F.ortho = what.ortho;
    F.ortho_n = what.ortho_n;
    F.rays = what.rb ? what.rb->rays : nullptr;
    F.bare_trace = (what.ortho_n || what.rb) ? 1 : 0;
    if (what.rb) hl[1].present = 0;  // trace_ray knows one space: no UI layering (and, below, one ray per result whatever `antialiasing` says)
    if (what.ortho_n) {
        // render_orthographic traces with GraphicsOptions::UNALTERED_COLORS and no UI layer (ortho.rs:44, 103-131)
        hl[1].present = 0;
        DevOptions &o = hl[0].opt;
        o.fog = 0; o.transparency = 1; o.lighting = 0; o.antialiasing = 0; o.debug_pixel_cost = 0; o.tone_mapping = 0;
        o.maximum_intensity = INFINITY; o.view_distance = 200.0;
        hl[0].exposure = 1.0f;
        P.flaws = 0;
    }
    P.ui = hl[1].present != 0;
    F.antialias = (hl[0].opt.antialiasing == 2 && !F.pixel_centers && !what.rb) ? 1 : 0;
    F.maximum_intensity = hl[0].opt.maximum_intensity;
    F.tone_mapping = hl[0].opt.tone_mapping;
    F.strip_rows = P.part.strip_rows;
    F.n_parts = P.part.n_parts;
    F.part = P.part.part;
    F.local_rows = P.local_rows;
    {
        // 8x8-pixel tiles: one wave-full of pixels per fetch from the tile counter. Measured against
        // 16x16 (AIC_TILE=16): -24 % frame time at 1080p, -11 % at 4K -- the coarser tiles left the
        // 2048 persistent waves with ~4 work items each and a long unbalanced tail.
        const int forced = c->sw.tile;
        F.tile = (forced == 8 || forced == 16) ? (uint32_t)forced : 8u;
        F.tiles_x = (f->width + F.tile - 1) / F.tile;
        F.tiles_y = (P.local_rows + F.tile - 1) / F.tile;
        const int macro_env = c->sw.macro;
        F.macro = (macro_env == 1 || macro_env == 2 || macro_env == 4 || macro_env == 8 || macro_env == 16) ? (uint32_t)macro_env : 2u;
        F.macros_x = (F.tiles_x + F.macro - 1) / F.macro;
        F.macros_y = (F.tiles_y + F.macro - 1) / F.macro;
    }
    F.light_lut = c->lut.p;
    F.n_cus = c->n_cus;
    F.tiles_per_wave = c->sw.tiles_per_wave ? c->sw.tiles_per_wave : (c->streaming_submit ? 4u : 1u);
    if (!c->sw.tiles_per_wave && c->streaming_submit && k == 1u) F.tiles_per_wave = part_grid_tiles_per_wave(c, slot, F);
    F.srgb_buckets = c->srgb_buckets.p;
}

// Step 2b: what the launch is to be -- recording or production (want_aux, diag), how its tiles are handed out (tile queues, super-blocks, cost feedback)
// and, for production, with or without the lane exchange. Arithmetic only, so an empty frame passes through it too before submit_frames returns.
void plan_dispatch(const aic_ctx *c, uint32_t k, const aic_frame_desc *f, bool allow_aux, const Traced &what, FramePlan &P) {
    DevFrame &F = P.F;
    P.want_aux = allow_aux && (f->flags & AIC_FRAME_AUX) != 0;
    P.diag = P.want_aux || P.split || what.px || (f->flags & AIC_FRAME_COUNTERS) != 0;  // (the Split's depth and layer, and pixel lists, live in the recording variants only)
    P.n_tiles = F.macros_x * F.macros_y;  // the feedback works on macro tiles
    // XCD-local tile queues (aic_scene_kernels.h order_tiles_kernel): one per XCD (32 CUs each on this part), a macro tile in the queue of the
    // 2^sb_shift-macro-tile super-block it lies in. One queue (aic_frame_desc.tuning) is the single dispenser of rounds 1-3.
    // (aic_frame_desc.tuning; environment variables read per frame until round 5)
    const int queues_env = (int)((f->tuning >> AIC_TUNE_QUEUES_SHIFT) & 15u);
    const int super_env = (int)((f->tuning >> AIC_TUNE_SUPER_SHIFT) & 31u) - 1;
    P.n_queues = queues_env > 0 ? (uint32_t)queues_env : (uint32_t)c->n_cus / 32u;
    if (P.n_queues > kMaxTileQueues) P.n_queues = kMaxTileQueues;
    if (P.n_queues < 2u || !what.whole_frame() || !P.n_tiles) P.n_queues = 0u;
    const uint32_t macro_log2 = F.macro >= 16 ? 4u : (F.macro >= 8 ? 3u : (F.macro >= 4 ? 2u : (F.macro >= 2 ? 1u : 0u)));
    const uint32_t tile_log2 = F.tile >= 16 ? 4u : 3u;
    // default super-block edge: the largest power of two within an eighth of the (local) image height -- 128 pixels at 1080p, 256 at 4K, ~135 blocks
    // either way: larger blocks fetch less (s256: 9.0 GB per frame with one dispenser, 5.2 at 128 pixels, 3.6 at 512) but leave a queue with too few
    // blocks to even out a scene that is part sky (profiles/r04_experiments.txt K)
    uint32_t sb_px_log2 = 0;
    while ((2u << sb_px_log2) <= std::max(1u, P.local_rows / 8u)) sb_px_log2++;
    P.sb_shift = super_env >= 0 ? (uint32_t)std::min(super_env, 12) : (sb_px_log2 > macro_log2 + tile_log2 ? sb_px_log2 - macro_log2 - tile_log2 : 0u);
    // tile order for a frame from the cost the sub-frame's previous frame recorded, if that frame
    // had the same shape (else index order); the record was turned into an order, and cleared, behind that frame
    P.use_feedback = c->sw.feedback && P.n_tiles && what.whole_frame() && !(f->flags & AIC_FRAME_NO_FEEDBACK);
    const uint32_t sig[4] = {f->width, P.local_rows, (P.part.n_parts << 16) | P.part.part, (P.part.strip_rows << 8) | (F.macro << 4) | (F.tile >> 3)};
    const uint32_t order_key[6] = {sig[0], sig[1], sig[2], sig[3], P.n_queues, P.sb_shift};
    std::memcpy(P.sig, sig, sizeof(sig));
    std::memcpy(P.order_key, order_key, sizeof(order_key));
    P.ordered = P.use_feedback || P.n_queues;  // the frames take their tiles through an order (else: the plain counter, index order)
    F.n_queues = P.ordered ? P.n_queues : 0u;
    if (!P.diag) {
        // The production variants exist with and without the lane exchange (aic_trace.hip). The exchanging ones keep a pixel's antialiasing sums in global
        // memory -- one region per persistent workgroup, the same for the UI pre-pass and the world pass of a frame (they follow one another on the
        // stream) -- which only a frame traced with antialiasing needs.
        P.ray_cold_bytes = trace_ray_cold_bytes(c->n_cus, &P.ray_cold_groups);
        if (P.ray_cold_bytes) {
            // the exchange (a pool of parked rays per workgroup: more rays in flight than lanes, lanes traded between waves) pays when a wave refills its lanes
            // several times over: from 5 tiles per resident wave for a frame alone (the whole 1080p frame has 7.9 and gains 6.5 %, a rank's share at
            // N = 2 has 4 and gains nothing, at N = 4 / 8 two / one and loses 3-6 % -- profiles/r05_rank_share.txt); the UI pre-pass follows the world pass
            // -- and from 1.9 for frames that are streamed (aic_render_submit), where a share of C3 at N = 8 (4 tiles per wave) gains 9 % by it and, since the
            // scheduler round was trimmed, a share of C2 at N = 4 (2 tiles per wave) 1.8 %; at one tile per wave (N = 8) the plain variant stays 2.5 % ahead).
            // A batch's frames share the resident grid: each has 1 / k of the waves.
            const uint32_t asked = (f->tuning >> AIC_TUNE_VARIANT_SHIFT) & 3u;  // (AIC_XCHG_TILES, an environment variable read per frame, until round 5)
            const double resident_waves = (double)c->n_cus * 16.0 / (double)k;
            const double need = c->streaming_submit ? 1.9 : 5.0;
            F.exchange = asked == AIC_VARIANT_EXCHANGING ? 1u : (asked == AIC_VARIANT_PLAIN ? 0u : (((double)F.tiles_x * (double)F.tiles_y >= need * resident_waves) ? 1u : 0u));
        }
    }
}

// Does the cost order a sub-frame recorded predict this frame? Same shape, queues and super-blocks, and the camera has barely moved since: the view rays
// through the centre and two corners within a degree, the eye within a quarter cube. (A stale order is worse than none.)
bool record_predicts(const FramePlan &P, const aic_ctx::SubSlot &sb, const aic_frame_desc &frame) {
    return P.use_feedback && sb.record_ready && std::memcmp(P.order_key, sb.order_key, sizeof(P.order_key)) == 0 && sb.tile_order.n >= P.n_tiles &&
           cameras_close(frame.world.inverse_projection_view, sb.cost_cam);
}

// Step 3: no record to go by: index order inside each queue, made once per frame shape.
int ensure_static_order(aic_ctx *c, aic_ctx::FrameSlot &fs, uint32_t k, const aic_frame_desc *frames, const FramePlan &P) {
    if (!P.ordered || !P.n_queues) return AIC_OK;
    bool any_static = false;
    for (uint32_t j = 0; j < k; j++) any_static = any_static || !record_predicts(P, fs.sub[j], frames[j]);
    if (!any_static || (fs.static_ready && std::memcmp(P.order_key, fs.static_key, sizeof(P.order_key)) == 0 && fs.tile_static.n >= P.n_tiles)) return AIC_OK;
    fs.static_ready = false;
    hipError_t e;
    if ((e = fs.tile_static.ensure(P.n_tiles)) != hipSuccess || (e = fs.queue_static.ensure(kMaxTileQueues + 1)) != hipSuccess) return hip_fail(c, "alloc tile queues", e);
    launch_order_tiles(nullptr, fs.tile_static.p, P.n_tiles, P.F.macros_x, P.sb_shift, P.n_queues, fs.queue_static.p, fs.stream);
    HIP_TRY(c, hipGetLastError());
    std::memcpy(fs.static_key, P.order_key, sizeof(P.order_key));
    fs.static_ready = true;
    return AIC_OK;
}

// Step 4, per sub-frame: backdrop and exposure, where the trace writes, clean counters, the tile order it takes and the cost record it writes, the UI pre-pass's buffers.
int bind_sub_frame(aic_ctx *c, aic_ctx::FrameSlot &fs, uint32_t j, const aic_frame_desc &frame, uint32_t *out_device, FramePlan &P) {
    aic_ctx::SubSlot &sb = fs.sub[j];
    DevFrame &F = P.F;
    DevSub &S = F.sub[j];
    const uint32_t n_tiles = P.n_tiles;
    hipError_t e;
    std::memcpy(S.backdrop, frame.backdrop, sizeof(S.backdrop));
    S.has_backdrop = !(frame.backdrop[0] == 0.f && frame.backdrop[1] == 0.f && frame.backdrop[2] == 0.f && frame.backdrop[3] == 0.f);
    S.exposure = F.ortho_n ? 1.0f : frame.world.exposure + 0.0f;  // (PositiveSign: checked in validate_frames; -0.0 becomes +0.0)
    S.out = out_device;
    if (P.bloom) {
        if ((e = sb.bloom_cb.ensure(P.npix)) != hipSuccess || (e = sb.bloom_mips.ensure(bloom_geometry(F.width, F.height).texels)) != hipSuccess)
            return hip_fail(c, "alloc bloom scratch", e);
        S.out = reinterpret_cast<uint32_t *>(sb.bloom_cb.p);
    }
    if ((e = sb.counters.ensure(1)) != hipSuccess) return hip_fail(c, "alloc frame counters", e);
    S.counters = sb.counters.p;
    if (!sb.host_counters) {  // (on a sub-frame's first frame: most contexts only ever use slot 0, and a context is cheap to make and drop)
        HIP_TRY(c, hipHostMalloc((void **)&sb.host_counters, sizeof(DevCounters), hipHostMallocDefault));
        std::memset(sb.host_counters, 0, sizeof(DevCounters));
    }
    if (!sb.counters_clean) HIP_TRY(c, hipMemsetAsync(sb.counters.p, 0, sizeof(DevCounters), fs.stream));
    sb.counters_clean = false;
    if (P.ordered) {
        if (record_predicts(P, sb, frame)) {
            S.tile_order = sb.tile_order.p;
            S.queue_start = P.n_queues ? sb.queue_start.p : nullptr;
        } else if (P.n_queues) {
            S.tile_order = fs.tile_static.p;
            S.queue_start = fs.queue_static.p;
        }
        if (P.use_feedback) {
            const uint32_t *const before = sb.tile_cost.p;
            if ((e = sb.tile_cost.ensure(n_tiles)) != hipSuccess) return hip_fail(c, "alloc tile feedback", e);
            if (sb.tile_cost.p != before) sb.cost_clean_n = 0;
            if (sb.cost_clean_n < n_tiles) HIP_TRY(c, hipMemsetAsync(sb.tile_cost.p, 0, (size_t)n_tiles * sizeof(uint32_t), fs.stream));
            sb.cost_clean_n = 0;  // (this frame writes it)
            S.tile_cost = sb.tile_cost.p;
            std::memcpy(sb.cost_sig, P.sig, sizeof(P.sig));
        }
    }
    if (P.ui) {
        const size_t samples = F.antialias ? 4 : 1;
        if ((e = sb.acc.ensure(samples * P.npix)) != hipSuccess) return hip_fail(c, "alloc accumulators", e);
        S.acc_buf = sb.acc.p;
        if (P.split) {  // every sample's DepthBuf, handed from the UI pre-pass to the world pass
            if ((e = sb.split_depth.ensure(samples * P.npix)) != hipSuccess) return hip_fail(c, "alloc sample depths", e);
            F.split_depth[j] = sb.split_depth.p;
        }
    }
    F.split_ui_exposure[j] = frame.ui.exposure + 0.0f;
    return AIC_OK;
}

// Step 5 (whole frames, and pixel lists for their target frame): Viewport's pixel edges (viewport.rs:104-113), once per frame shape: x / width * 2 - 1 and -(y / height * 2 - 1) in the reference's own f64
// operations (this file is built with -ffp-contract=off, like the kernels), so that the kernel reads them instead of dividing per ray
int bind_pixel_edges(aic_ctx *c, aic_ctx::FrameSlot &fs, DevFrame &F, const uint32_t width, const uint32_t height) {
    if (fs.edges_w != width || fs.edges_h != height || !fs.edges.p) {
        std::vector<double> host((size_t)width + 1 + (size_t)height + 1);
        for (uint32_t x = 0; x <= width; x++) host[x] = ((double)x) / (double)width * 2.0 - 1.0;
        for (uint32_t y = 0; y <= height; y++) host[(size_t)width + 1 + y] = -(((double)y) / (double)height * 2.0 - 1.0);
        fs.edges_w = fs.edges_h = 0;
        const hipError_t e = fs.edges.ensure(host.size());
        if (e != hipSuccess) return hip_fail(c, "alloc pixel edges", e);
        // (the slot's stream may still be reading the table of the previous shape: the copy is ordered behind it, and staged before the call returns)
        HIP_TRY(c, hipMemcpyAsync(fs.edges.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, fs.stream));
        HIP_TRY(c, hipStreamSynchronize(fs.stream));
        fs.edges_w = width; fs.edges_h = height;
    }
    F.edge_x = fs.edges.p;
    F.edge_y = fs.edges.p + (size_t)width + 1;
    return AIC_OK;
}

// Step 7a: the UI pre-pass, on a copy of the frame: the UI layer and cameras, one dispenser and no feedback (that describes the world pass). Leaves the
// sub-frames' tile dispensers at zero for the world pass.
int launch_ui_prepass(aic_ctx *c, aic_ctx::FrameSlot &fs, uint32_t k, const aic_frame_desc *frames, const FramePlan &P) {
    DevFrame U = P.F;
    U.pass = 1;
    U.hit_layer = 1u;
    U.use_init = 0;
    U.layer = P.hl[1];
    U.layer_transparency = P.hl[1].opt.transparency;
    U.layer_lighting = P.hl[1].opt.lighting;
    for (uint32_t j = 0; j < k; j++) {
        std::memcpy(U.sub[j].inv, frames[j].ui.inverse_projection_view, sizeof(U.sub[j].inv));
        U.sub[j].tile_order = nullptr;  // the feedback describes the world pass
        U.sub[j].tile_cost = nullptr;
        U.sub[j].queue_start = nullptr;
        U.sub[j].host_counters = nullptr;  // (the world pass hands over the sums of both)
    }
    U.n_queues = 0u;
    launch_trace_image(U, P.diag, fs.stream);
    for (uint32_t j = 0; j < k; j++) HIP_TRY(c, hipMemsetAsync(&fs.sub[j].counters.p->tile_next, 0, sizeof(uint32_t), fs.stream));
    return AIC_OK;
}

// Step 7b: the world pass; what aic_frame_info reports of the slot's frame is settled here.
int launch_world_pass(aic_ctx *c, aic_ctx::FrameSlot &fs, uint32_t k, const aic_frame_desc *frames, const Traced &what, FramePlan &P) {
    DevFrame &F = P.F;
    const DevLayer &world = P.hl[0];
    F.use_init = P.ui ? 1 : 0;
    F.pass = (what.rb && what.rb->no_sky) ? 2 : 0;
    F.hit_layer = what.rb ? what.rb->layer : 0u;
    for (uint32_t j = 0; j < k; j++) {
        std::memcpy(F.sub[j].inv, what.ortho_n ? world.inv : frames[j].world.inverse_projection_view, sizeof(F.sub[j].inv));
#ifndef AIC_PROFILE
        F.sub[j].host_counters = reinterpret_cast<unsigned long long *>(fs.sub[j].host_counters);  // (DevCounters begins with the five sums)
#endif
    }
    F.layer = world;
    F.layer_transparency = world.opt.transparency;
    F.layer_lighting = world.opt.lighting;
    // (Bounce lighting has no exchanging variant: aic_trace.hip launch_trace)
    fs.variant = P.diag ? AIC_VARIANT_RECORDING : ((F.exchange && world.opt.lighting != 5 && (F.ray_cold || !F.antialias)) ? AIC_VARIANT_EXCHANGING : AIC_VARIANT_PLAIN);
    fs.tile_queues = F.n_queues;
    launch_trace_image(F, P.diag, fs.stream);
    HIP_TRY(c, hipGetLastError());
    return AIC_OK;
}

// Step 7c: each frame's ColorBuf through the chain and the composite into the caller's buffer; ev1 (kernel_ms, aic_stream_wait_frame) is behind it
int launch_bloom_chain(aic_ctx *c, aic_ctx::FrameSlot &fs, uint32_t k, uint32_t *const *out_devices, const FramePlan &P) {
    const DevFrame &F = P.F;
    const BloomGeom geom = bloom_geometry(F.width, F.height);
    for (uint32_t j = 0; j < k; j++) {
        BloomParams bp;
        bp.colorbuf = fs.sub[j].bloom_cb.p;
        bp.mips = fs.sub[j].bloom_mips.p;
        bp.out = out_devices[j];
        bp.exposure = F.sub[j].exposure;
        bp.intensity = c->layers[AIC_LAYER_WORLD].opt.bloom_intensity;
        bp.tone_mapping = F.tone_mapping;
        bp.maximum_intensity = F.maximum_intensity;
        bp.srgb_thr = c->srgb_thr.p;
        launch_bloom(geom, bp, fs.stream);
    }
    HIP_TRY(c, hipGetLastError());
    return AIC_OK;
}

// Step 8, behind the frame: the slot is made ready for its next frame: this frame's cost record becomes the tile order of the next frame of the same view, the
// record and the counters are cleared. A failure here costs the next frame its head start (it clears and orders for itself), not this frame its result.
void prepare_next_frame(aic_ctx::FrameSlot &fs, uint32_t k, const aic_frame_desc *frames, const FramePlan &P) {
    bool cleared = false;
    if (P.use_feedback && P.n_tiles) {
        OrderJobs jobs;
        std::memset(&jobs, 0, sizeof(jobs));
        bool ok = true;
        for (uint32_t j = 0; j < k; j++) {
            aic_ctx::SubSlot &sb = fs.sub[j];
            sb.record_ready = false;
            sb.cost_clean_n = 0;
            ok = ok && sb.tile_order.ensure(P.n_tiles) == hipSuccess && sb.queue_start.ensure(kMaxTileQueues + 1) == hipSuccess;
            jobs.cost[j] = sb.tile_cost.p; jobs.order[j] = sb.tile_order.p; jobs.queue_start[j] = sb.queue_start.p;
            jobs.clear_words[j] = reinterpret_cast<uint32_t *>(sb.counters.p);
        }
        if (ok) {
            // (one launch, a workgroup per frame: orders, then clears the record it has read and the counters)
            launch_order_tiles_jobs(jobs, k, P.n_tiles, P.F.macros_x, P.sb_shift, P.n_queues ? P.n_queues : 1u, fs.stream, true, (uint32_t)(sizeof(DevCounters) / 4));
            if (hipGetLastError() == hipSuccess) {
                cleared = true;
                for (uint32_t j = 0; j < k; j++) {
                    aic_ctx::SubSlot &sb = fs.sub[j];
                    sb.cost_clean_n = P.n_tiles;
                    std::memcpy(sb.order_key, P.order_key, sizeof(P.order_key));
                    std::memcpy(sb.cost_cam, frames[j].world.inverse_projection_view, sizeof(sb.cost_cam));
                    sb.record_ready = true;
                }
            }
        }
    }
    if (!cleared) {
        cleared = true;
        for (uint32_t j = 0; j < k; j++) cleared = (hipMemsetAsync(fs.sub[j].counters.p, 0, sizeof(DevCounters), fs.stream) == hipSuccess) && cleared;
    }
    for (uint32_t j = 0; j < k; j++) fs.sub[j].counters_clean = cleared;
}

#define STEP(expr)                         \
    do {                                   \
        const int rc_ = (expr);            \
        if (rc_ != AIC_OK) return rc_;     \
    } while (0)

// Queues the frames of one launch on a slot's stream: counters reset, optional UI pre-pass, the trace. No waiting. k = 1: a plain frame. k = 2, 4, 8
// (aic_render_submit_batch): frames of the same shape, partition and flags under the scene and options as they stand, each with its own cameras, backdrop,
// output buffer, counters and cost record -- traced side by side by ONE launch per pass (DevSub), every persistent workgroup bound to one of them.
int submit_frames(aic_ctx *c, uint32_t k, const aic_frame_desc *frames, uint32_t *const *out_devices, uint32_t slot, bool allow_aux, const Traced &what = Traced()) {
    aic_ctx::FrameSlot &fs = c->slots[slot];
    fs.t_begin = std::chrono::steady_clock::now();
    fs.n_sub = k;
    FramePlan P;
    STEP(validate_frames(c, k, frames, out_devices, slot, what, P));
    plan_geometry(c, k, &frames[0], slot, what, P);
    plan_dispatch(c, k, &frames[0], allow_aux, what, P);
    DevFrame &F = P.F;
    fs.diag = P.diag;
    fs.flaws = P.flaws;
    fs.light_used[0] = P.hl[0].light;
    fs.light_used[1] = P.hl[1].light;
    fs.local_rows = P.local_rows;
    fs.npix = P.npix;
    fs.variant = fs.tile_queues = 0;
    if (allow_aux) c->aux_records = 0;
    if (!P.npix) {  // an empty frame (a partition's part of no rows): nothing is queued, but it occupies its slot until it is waited for like any other
        fs.busy = true;
        return AIC_OK;
    }
    const bool own_aux = P.want_aux && !what.aux_target();  // the first-hit records go to the context's buffer (aic_read_aux)
    hipError_t e;
    if (own_aux && (e = c->aux.ensure(P.npix)) != hipSuccess) return hip_fail(c, "alloc aux", e);
    if (P.want_aux) F.aux = own_aux ? c->aux.p : what.aux_target();
    STEP(ensure_static_order(c, fs, k, frames, P));
    for (uint32_t j = 0; j < k; j++) STEP(bind_sub_frame(c, fs, j, frames[j], out_devices[j], P));
    if (what.whole_frame()) STEP(bind_pixel_edges(c, fs, F, F.width, F.height));
    if (what.px) STEP(bind_pixel_edges(c, fs, F, what.px->width, what.px->height));
    if (F.exchange && F.antialias) {  // the exchanging variants' antialiasing sums (DevFrame::ray_cold)
        if ((e = fs.ray_cold.ensure(P.ray_cold_bytes / sizeof(uint4))) != hipSuccess) return hip_fail(c, "alloc ray state", e);
        F.ray_cold = fs.ray_cold.p;
        F.ray_cold_groups = P.ray_cold_groups;
    }
    HIP_TRY(c, hipEventRecord(fs.ev0, fs.stream));
    if (P.ui) STEP(launch_ui_prepass(c, fs, k, frames, P));
    STEP(launch_world_pass(c, fs, k, frames, what, P));
    if (P.bloom) STEP(launch_bloom_chain(c, fs, k, out_devices, P));
    HIP_TRY(c, hipEventRecord(fs.ev1, fs.stream));
    // behind the trace: the frame's sums are in pinned host memory -- written by the last wave of the trace itself, or (profile builds: the whole
    // counter block) copied there; ev2 is what a wait waits for ...
#ifdef AIC_PROFILE
    for (uint32_t j = 0; j < k; j++) HIP_TRY(c, hipMemcpyAsync(fs.sub[j].host_counters, fs.sub[j].counters.p, sizeof(DevCounters), hipMemcpyDeviceToHost, fs.stream));
#endif
    HIP_TRY(c, hipEventRecord(fs.ev2, fs.stream));
    fs.busy = true;  // the frame is in flight and a wait can collect it; nothing below can fail the call any more
    prepare_next_frame(fs, k, frames, P);  // ... and the slot is made ready for its next frame
    if (own_aux) c->aux_records = P.npix;
    return AIC_OK;
}
#undef STEP
int submit_frame(aic_ctx *c, const aic_frame_desc *f, uint32_t *out_device, uint32_t slot, bool allow_aux, const Traced &what = Traced()) {
    uint32_t *const outs[1] = {out_device};
    return submit_frames(c, 1, f, outs, slot, allow_aux, what);
}

// -DAIC_PROFILE builds (tools/build_variants.sh): a frame's profile counters to stderr, its per-wave clocks to the file AIC_WAVE_PROF names.
void report_profile(const aic_ctx *c, const aic_ctx::FrameSlot &fs, const DevCounters &hc) {
#ifdef AIC_PROFILE
    static const char *names[40] = {"max_lifetime","max_until_dry","cyc_until_dry","cyc_lifetime","shade_ph","shade_ln","enter_ph","enter_ln","ray_ph","ray_ln","step_iters","step_lanes","cyc_step","cyc_shade_rest","cyc_enter","cyc_newray","cyc_finish","cyc_refill","cyc_shade_light","cyc_sched","fast_iters","fast_lanes","trips","trip_lanes","pass_hl_lanes","pass_fast_eligible","leave_blocks","leave_lanes","apply_blocks","apply_lanes","pass_needed_lanes","xchg_rounds","xchg_lanes","cyc_xchg","xchg_picked","xchg_parked","idle_spins","xchg_claims_lost","xchg_empty","-"};
    // (only the production variant's frames: the aux-recording variant is another kernel, at half the occupancy)
    if (!fs.diag) for (int i = 0; i < 39; i++) std::fprintf(stderr, "PROF %s %llu\n", names[i], hc.prof[i]);
    if (const char *path = (fs.diag || c->sw.wave_prof.empty()) ? nullptr : c->sw.wave_prof.c_str()) {
        if (FILE *fp = std::fopen(path, "w")) {
            for (int w = 0; w < 2048; w++) std::fprintf(fp, "%u %u %u %u\n", hc.wave_prof[w][0], hc.wave_prof[w][1], hc.wave_prof[w][2], hc.wave_prof[w][3]);
            std::fclose(fp);
        }
    }
#else
    (void)c; (void)fs; (void)hc;
#endif
}

// Waits for a slot's frame (or batch of frames) and reports it: `info` = the frame's, or the batch's sums; `infos` (may be null) = each frame's.
int wait_frame(aic_ctx *c, uint32_t slot, aic_frame_info *info, bool whole_stream = false, aic_frame_info *infos = nullptr, uint32_t n_infos = 0) {
    aic_ctx::FrameSlot &fs = c->slots[slot];
    if (info) std::memset(info, 0, sizeof(*info));
    for (uint32_t j = 0; infos && j < n_infos; j++) std::memset(&infos[j], 0, sizeof(infos[j]));
    float kernel_ms = 0.f;
    const uint32_t k = fs.n_sub ? fs.n_sub : 1u;
    if (fs.busy && !fs.npix) fs.busy = false;  // an empty frame: no event was recorded for it, the report is all zeros
    if (fs.busy) {
        fs.busy = false;  // released whatever happens below: a frame that failed must not block its slot for good
        // the frame and its counters (ev2), not the slot's housekeeping behind them -- unless the caller has enqueued a copy of its own behind the frame
        if (whole_stream || c->sw.wait_whole_stream) HIP_TRY(c, hipStreamSynchronize(fs.stream));  // (the switch: a measurement)
        else HIP_TRY(c, hipEventSynchronize(fs.ev2));
        HIP_TRY(c, hipEventElapsedTime(&kernel_ms, fs.ev0, fs.ev1));
        for (uint32_t j = 0; j < k; j++) {
            DevCounters hc;
            std::memcpy(&hc, fs.sub[j].host_counters, sizeof(hc));
            if (hc.bailed) return fail(c, AIC_ERR_DEVICE, "trace kernel: a wave gave up waiting for rays in transit between waves; the frame has unwritten pixels");
            if (info) {
                info->cubes_traced += hc.cubes_traced;
                info->n_outer += hc.n_outer;
                info->n_inner += hc.n_inner;
                info->n_hits += hc.n_hits;
                info->n_light += hc.n_light;
            }
            if (infos && j < n_infos) {
                infos[j].cubes_traced = hc.cubes_traced; infos[j].n_outer = hc.n_outer; infos[j].n_inner = hc.n_inner;
                infos[j].n_hits = hc.n_hits; infos[j].n_light = hc.n_light;
            }
            report_profile(c, fs, hc);
        }
    }
    const float total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - fs.t_begin).count();
    auto fill = [&](aic_frame_info *o) {
        o->kernel_ms = kernel_ms;
        o->rows_rendered = fs.local_rows;
        o->flaws = fs.flaws;
        o->variant = fs.npix ? fs.variant : 0u;
        o->tile_queues = fs.npix ? fs.tile_queues : 0u;
        o->total_ms = total_ms;
    };
    if (info) fill(info);
    for (uint32_t j = 0; infos && j < n_infos && j < k; j++) fill(&infos[j]);
    return AIC_OK;
}

// a frame slot's stream, events and counter block (slots past the eighth: on first use)
int ensure_slot(aic_ctx *c, uint32_t slot) {
    aic_ctx::FrameSlot &fs = c->slots[slot];
    if (fs.stream && fs.ev0 && fs.ev1 && fs.ev2 && fs.sub[0].counters.p) return AIC_OK;
    if (!fs.stream) {
        HIP_TRY(c, hipStreamCreateWithFlags(&fs.stream, hipStreamNonBlocking));
        // "Everything the context queues afterwards waits for the event" (aic_wait_event) must hold for a stream made later too: the context's first
        // stream received every such wait, so the new stream is ordered behind where that one stands now (a first frame on slot >= 8
        // after an aic_wait_event raced the gather still reading its strip buffer)
        hipEvent_t ev = nullptr;
        HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e1 = hipEventRecord(ev, c->stream);
        if (e1 == hipSuccess) e1 = hipStreamWaitEvent(fs.stream, ev, 0);
        (void)hipEventDestroy(ev);  // (released once the recorded work is done)
        if (e1 != hipSuccess) return hip_fail(c, "order a new slot's stream behind the context's waits", e1);
    }
    if (!fs.ev0) HIP_TRY(c, hipEventCreate(&fs.ev0));
    if (!fs.ev1) HIP_TRY(c, hipEventCreate(&fs.ev1));
    if (!fs.ev2) HIP_TRY(c, hipEventCreate(&fs.ev2));
    hipError_t e = fs.sub[0].counters.ensure(1);
    if (e != hipSuccess) return hip_fail(c, "alloc frame counters", e);
    return AIC_OK;
}

// raytracer::ortho::OrthoCamera::new / MultiOrthoCamera::new (ortho.rs:147-184, 213-282), on the host: five pixel-perfect
// views (top, left, front, right, bottom) laid out around the front view. Matrices are euclid's row-vector 4x4.
struct Mat4h { double m[16]; };
Mat4h mat_identity() { Mat4h t{}; t.m[0] = t.m[5] = t.m[10] = t.m[15] = 1.0; return t; }
Mat4h mat_then(const Mat4h &a, const Mat4h &b) {  // Transform3D::then
    Mat4h o{};
    for (int r = 0; r < 4; r++)
        for (int cc = 0; cc < 4; cc++)
            o.m[r * 4 + cc] = a.m[r * 4 + 0] * b.m[0 * 4 + cc] + a.m[r * 4 + 1] * b.m[1 * 4 + cc] + a.m[r * 4 + 2] * b.m[2 * 4 + cc] + a.m[r * 4 + 3] * b.m[3 * 4 + cc];
    return o;
}
void ortho_view(int resolution, const int32_t lo[3], const int32_t size[3], int viewed_face /* 1 NX .. 6 PZ */, DevOrthoView *out) {
    const int axis = (viewed_face - 1) % 3;
    const int32_t ub[3] = {lo[0] + size[0], lo[1] + size[1], lo[2] + size[2]};
    out->w = (uint32_t)(axis == 0 ? size[2] : size[0]) * (uint32_t)resolution;
    out->h = (uint32_t)(axis == 1 ? size[2] : size[1]) * (uint32_t)resolution;
    double ot[3];
    // images of +X, +Y, +Z under the view's grid rotation (Face::clockwise / counterclockwise, face.rs:440-465)
    int bx[3], by[3], bz[3];
    auto set = [](int v[3], int x, int y, int z) { v[0] = x; v[1] = y; v[2] = z; };
    switch (viewed_face) {
        case 1: ot[0] = lo[0]; ot[1] = ub[1]; ot[2] = lo[2]; set(bx, 0, 0, 1); set(by, 0, 1, 0); set(bz, -1, 0, 0); break;   // NX: PY.clockwise()
        case 2: ot[0] = lo[0]; ot[1] = lo[1]; ot[2] = ub[2]; set(bx, 1, 0, 0); set(by, 0, 0, 1); set(bz, 0, -1, 0); break;   // NY: PX.clockwise()
        case 3: ot[0] = ub[0]; ot[1] = ub[1]; ot[2] = lo[2]; set(bx, -1, 0, 0); set(by, 0, 1, 0); set(bz, 0, 0, -1); break;  // NZ: 180 degrees about Y
        case 4: ot[0] = ub[0]; ot[1] = ub[1]; ot[2] = ub[2]; set(bx, 0, 0, -1); set(by, 0, 1, 0); set(bz, 1, 0, 0); break;   // PX: PY.counterclockwise()
        case 5: ot[0] = lo[0]; ot[1] = ub[1]; ot[2] = lo[2]; set(bx, 1, 0, 0); set(by, 0, 0, -1); set(bz, 0, 1, 0); break;   // PY: PX.counterclockwise()
        default: ot[0] = lo[0]; ot[1] = ub[1]; ot[2] = ub[2]; set(bx, 1, 0, 0); set(by, 0, 1, 0); set(bz, 0, 0, 1); break;   // PZ: identity
    }
    // translation(0.5, 0.5, 0).then_scale(1, -1, 1).then(scale 1/resolution).then(rotation).then_translate(origin)
    Mat4h t = mat_identity();
    t.m[12] = 0.5; t.m[13] = 0.5;
    Mat4h flip = mat_identity();
    flip.m[5] = -1.0;
    t = mat_then(t, flip);
    Mat4h sc = mat_identity();
    sc.m[0] = sc.m[5] = sc.m[10] = 1.0 / (double)resolution;
    t = mat_then(t, sc);
    Mat4h rot{};
    for (int a = 0; a < 3; a++) { rot.m[0 + a] = bx[a]; rot.m[4 + a] = by[a]; rot.m[8 + a] = bz[a]; }
    rot.m[15] = 1.0;
    t = mat_then(t, rot);
    Mat4h tr = mat_identity();
    tr.m[12] = ot[0]; tr.m[13] = ot[1]; tr.m[14] = ot[2];
    t = mat_then(t, tr);
    std::memcpy(out->m, t.m, sizeof(t.m));
    // transform_vector3d((0, 0, -1)) reduced to its axis (TryFrom<Ray> for AaRay keeps only the direction's axis and sign)
    for (int a = 0; a < 3; a++) { const double d = -t.m[8 + a]; out->dir[a] = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }
}
void multi_ortho(int resolution, const int32_t lo[3], const int32_t size[3], DevOrthoView v[5], uint32_t *w, uint32_t *h) {
    ortho_view(resolution, lo, size, 5, &v[0]);  // top
    ortho_view(resolution, lo, size, 1, &v[1]);  // left
    ortho_view(resolution, lo, size, 6, &v[2]);  // front
    ortho_view(resolution, lo, size, 4, &v[3]);  // right
    ortho_view(resolution, lo, size, 2, &v[4]);  // bottom
    v[0].x0 = v[1].w + 1; v[0].y0 = 0;
    v[1].x0 = 0; v[1].y0 = v[0].h + 1;
    v[2].x0 = v[1].w + 1; v[2].y0 = v[0].h + 1;
    v[3].x0 = v[1].w + v[2].w + 2; v[3].y0 = v[0].h + 1;
    v[4].x0 = v[1].w + 1; v[4].y0 = v[0].h + v[2].h + 2;
    *w = *h = 0;
    for (int i = 0; i < 5; i++) {
        if (v[i].x0 + v[i].w > *w) *w = v[i].x0 + v[i].w;
        if (v[i].y0 + v[i].h > *h) *h = v[i].y0 + v[i].h;
    }
}
bool valid_ortho_resolution(int r) { return r >= 1 && r <= 128 && (r & (r - 1)) == 0; }

// A listed trace's batch is laid out as an image of up to 2048 columns: pixel i of that image traces item i of the list. `what`: the items, for the refusal.
int batch_image(aic_ctx *c, const char *who, const char *what, uint32_t n, aic_frame_desc *g) {
    g->width = n < 2048u ? n : 2048u;
    g->height = (n + g->width - 1u) / g->width;
    g->partition = aic_partition{0, 1, 0, 0};
    return g->height > 65535u ? reject(c, who, ("more than 2048 x 65535 " + std::string(what) + " in one call").c_str()) : AIC_OK;
}
// slot 0's stream is the one a synchronous trace queues on
int begin_on_slot0(aic_ctx *c, const char *who) {
    HIP_TRY(c, hipSetDevice(c->device));
    return c->slots[0].busy ? reject(c, who, "a submitted frame still occupies slot 0 (aic_render_wait it first)") : AIC_OK;
}
// a host list's staging and the results' buffer, which the launch is then aimed at
int size_staging(aic_ctx *c, size_t out_words, size_t list_bytes) {
    hipError_t e;
    if ((e = c->out.ensure(out_words)) != hipSuccess) return hip_fail(c, "alloc output", e);
    if ((e = c->staging.ensure(list_bytes)) != hipSuccess) return hip_fail(c, "alloc staging", e);
    return AIC_OK;
}
// behind the results' copy back: the frame is collected, a host caller's hit records are read back, and the info counts the items
int finish_listed(aic_ctx *c, uint32_t n, bool to_host, aic_pixel_aux *aux, aic_frame_info *info) {
    const int rc = wait_frame(c, 0, info, to_host);
    if (rc != AIC_OK) return rc;
    if (aux && to_host) HIP_TRY(c, hipMemcpy(aux, c->aux.p, (size_t)n * sizeof(aic_pixel_aux), hipMemcpyDeviceToHost));
    if (info) info->rows_rendered = n;
    return AIC_OK;
}

// Rays and orthographic views are traced as the WORLD layer of the launch, whatever layer holds the space: submit_frame with `layer` named for that seat.
// (Until the session fuzz the two Layer objects were swapped around the submit instead. A light update running on the context's worker thread holds a
// reference to its layer all the while -- neither call waits for it, by design -- and found the other layer's space under it: rays on the UI layer beside a
// pending update of the world cut that update short, tests/test_gpu_trace_rays.py.)
int submit_in_world_seat(aic_ctx *c, int layer, const aic_frame_desc *f, uint32_t *target, bool allow_aux, const Traced &what) {
    Traced seated = what;
    seated.world_seat = layer;
    return submit_frame(c, f, target, 0, allow_aux, seated);
}

}  // namespace

extern "C" {

int aic_render(aic_ctx *c, const aic_frame_desc *f, void *out_rgba8, int out_is_device, aic_frame_info *info) {
    if (!c || !f) return fail(c, AIC_ERR_INVALID, "aic_render: bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    if (const int rc = begin_on_slot0(c, "aic_render")) return rc;
    uint32_t *target = (uint32_t *)out_rgba8;
    const size_t px_words = (f->flags & (AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) ? 4 : ((f->flags & AIC_FRAME_OUT_SPLIT) ? 3 : 1);  // 16, 12 or 4 bytes per pixel
    if (!out_is_device && out_rgba8) {
        const aic_partition part = normalised_partition(*f);
        const size_t npix = (size_t)f->width * (part.part < part.n_parts ? aic_partition_rows(f->height, &part) : 0);
        hipError_t e;
        if (npix && (e = c->out.ensure(npix * px_words)) != hipSuccess) return hip_fail(c, "alloc output", e);
        target = c->out.p;
    }
    int rc = submit_frame(c, f, target, 0, true);
    if (rc != AIC_OK) return rc;
    if (!out_is_device && c->slots[0].npix)
        HIP_TRY(c, hipMemcpyAsync(out_rgba8, c->out.p, c->slots[0].npix * px_words * 4, hipMemcpyDeviceToHost, c->slots[0].stream));
    return wait_frame(c, 0, info, !out_is_device);
}

int aic_ortho_image_size(const int32_t lo[3], const int32_t size[3], int resolution, uint32_t *width, uint32_t *height) {
    if (!lo || !size || !width || !height || !valid_ortho_resolution(resolution) || size[0] < 0 || size[1] < 0 || size[2] < 0) return AIC_ERR_INVALID;
    DevOrthoView v[5];
    multi_ortho(resolution, lo, size, v, width, height);
    return AIC_OK;
}

int aic_render_orthographic(aic_ctx *c, int layer, int resolution, void *out_rgba8, int out_is_device, uint32_t *width, uint32_t *height,
                            aic_frame_info *info) {
    if (!c || !valid_layer(layer) || !valid_ortho_resolution(resolution)) return fail(c, AIC_ERR_INVALID, "aic_render_orthographic: bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    Layer &l = c->layers[layer];
    if (!l.present) return fail(c, AIC_ERR_INVALID, "aic_render_orthographic: no space uploaded for this layer");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->slots[0].busy) return fail(c, AIC_ERR_INVALID, "aic_render_orthographic: a submitted frame still occupies slot 0");
    DevOrthoView v[5];
    uint32_t w = 0, h = 0;
    multi_ortho(resolution, l.lo, l.size, v, &w, &h);
    if (width) *width = w;
    if (height) *height = h;
    if (!out_rgba8 || !w || !h) return AIC_OK;  // size query
    hipError_t e;
    if ((e = c->ortho_views.ensure(5)) != hipSuccess) return hip_fail(c, "alloc ortho views", e);
    HIP_TRY(c, hipMemcpy(c->ortho_views.p, v, sizeof(v), hipMemcpyHostToDevice));
    aic_frame_desc f;
    std::memset(&f, 0, sizeof(f));
    f.width = w;
    f.height = h;
    static const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(f.world.inverse_projection_view, ident, sizeof(ident));
    std::memcpy(f.ui.inverse_projection_view, ident, sizeof(ident));
    f.world.exposure = f.ui.exposure = 1.0f;
    uint32_t *target = (uint32_t *)out_rgba8;
    const size_t npix = (size_t)w * h;
    if (!out_is_device) {
        if ((e = c->out.ensure(npix)) != hipSuccess) return hip_fail(c, "alloc output", e);
        target = c->out.p;
    }
    Traced views;
    views.ortho = c->ortho_views.p;
    views.ortho_n = 5;
    const int rc = submit_in_world_seat(c, layer, &f, target, false, views);
    if (rc != AIC_OK) return rc;
    if (!out_is_device) HIP_TRY(c, hipMemcpyAsync(out_rgba8, c->out.p, npix * 4, hipMemcpyDeviceToHost, c->slots[0].stream));
    return wait_frame(c, 0, info, !out_is_device);
}

int aic_trace_patches(aic_ctx *c, const aic_frame_desc *f, uint32_t n, const double *rects, void *out_rgba8, aic_pixel_aux *aux,
                      aic_frame_info *info) {
    if (!c || !f || (n && (!rects || !out_rgba8))) return fail(c, AIC_ERR_INVALID, "aic_trace_patches: bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    if (!n) return AIC_OK;
    if (const int rc = begin_on_slot0(c, "aic_trace_patches")) return rc;
    if (f->flags & AIC_FRAME_BLOOM) return fail(c, AIC_ERR_UNSUPPORTED, "aic_trace_patches: AIC_FRAME_BLOOM needs a whole frame");
    if (f->flags & AIC_FRAME_OUT_SPLIT) return fail(c, AIC_ERR_UNSUPPORTED, "aic_trace_patches: AIC_FRAME_OUT_SPLIT is for whole frames");
    aic_frame_desc g = *f;
    if (const int rc = batch_image(c, "aic_trace_patches", "rectangles", n, &g)) return rc;
    g.flags = (f->flags & (AIC_FRAME_COUNTERS | AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) | (aux ? AIC_FRAME_AUX : 0u);
    const size_t px_words = (f->flags & (AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) ? 4 : 1;
    if (const int rc = size_staging(c, (size_t)g.width * g.height * px_words, (size_t)n * 32)) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->staging.p, rects, (size_t)n * 32, hipMemcpyHostToDevice, c->slots[0].stream));
    Traced batch;
    batch.patches = (const double *)c->staging.p;
    batch.n_patches = n;
    const int rc = submit_frame(c, &g, c->out.p, 0, true, batch);
    if (rc != AIC_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(out_rgba8, c->out.p, (size_t)n * px_words * 4, hipMemcpyDeviceToHost, c->slots[0].stream));
    return finish_listed(c, n, true, aux, info);
}

int aic_trace_rays(aic_ctx *c, int layer, uint32_t n, const double *rays, uint32_t flags, float exposure, void *out, aic_pixel_aux *aux,
                   aic_frame_info *info) {
    if (!c || !valid_layer(layer) || (n && (!rays || !out))) return fail(c, AIC_ERR_INVALID, "aic_trace_rays: bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    if (flags & AIC_FRAME_BLOOM) return fail(c, AIC_ERR_UNSUPPORTED, "aic_trace_rays: AIC_FRAME_BLOOM needs a whole frame");
    if ((flags & AIC_FRAME_OUT_LINEAR) && (flags & AIC_FRAME_OUT_COLORBUF)) return fail(c, AIC_ERR_INVALID, "aic_trace_rays: AIC_FRAME_OUT_LINEAR and AIC_FRAME_OUT_COLORBUF exclude each other");
    if (!(exposure >= 0.f)) return fail(c, AIC_ERR_INVALID, "aic_trace_rays: exposure is negative or NaN");
    if (!n) return AIC_OK;
    if (const int rc = begin_on_slot0(c, "aic_trace_rays")) return rc;
    if (!c->layers[layer].present) return fail(c, AIC_ERR_INVALID, "aic_trace_rays: no space uploaded for this layer");
    const bool on_device = (flags & AIC_RAYS_DEVICE) != 0;
    const size_t px_words = (flags & (AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) ? 4 : 1;
    // (the kernel fetches a ray with 16-byte loads and stores a float result as one: an allocation's start, or any whole number of rays / results into it)
    if (on_device && (((uintptr_t)rays & 15u) || ((uintptr_t)out & (px_words * 4u - 1u)) || ((uintptr_t)aux & 7u)))
        return fail(c, AIC_ERR_INVALID, "aic_trace_rays: AIC_RAYS_DEVICE wants rays at a 16-byte boundary, out and aux at their element's");
    aic_frame_desc g;
    std::memset(&g, 0, sizeof(g));
    if (const int rc = batch_image(c, "aic_trace_rays", "rays", n, &g)) return rc;
    g.flags = (flags & (AIC_FRAME_COUNTERS | AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) | (aux ? AIC_FRAME_AUX : 0u);
    g.tuning = flags & (3u << AIC_TUNE_VARIANT_SHIFT);  // (the variant bits sit above every flag: measurement and tests ask for a production variant here)
    g.world.exposure = exposure;
    g.ui.exposure = 1.0f;
    RayBatch rb{rays, n, (flags & AIC_RAYS_NO_SKY) != 0, (uint32_t)layer, on_device ? reinterpret_cast<DevAux *>(aux) : nullptr};
    hipStream_t stream = c->slots[0].stream;
    if (!on_device) {
        if (const int rc = size_staging(c, (size_t)n * px_words, (size_t)n * 48)) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->staging.p, rays, (size_t)n * 48, hipMemcpyHostToDevice, stream));
        rb.rays = (const double *)c->staging.p;
    }
    uint32_t *const target = on_device ? (uint32_t *)out : c->out.p;
    Traced batch;
    batch.rb = &rb;
    const int rc = submit_in_world_seat(c, layer, &g, target, true, batch);
    if (rc != AIC_OK) return rc;
    if (!on_device) HIP_TRY(c, hipMemcpyAsync(out, c->out.p, (size_t)n * px_words * 4, hipMemcpyDeviceToHost, stream));
    return finish_listed(c, n, !on_device, aux, info);
}

int aic_trace_pixels(aic_ctx *c, const aic_frame_desc *f, uint32_t n, const uint32_t *pixels, uint32_t mode, void *out, aic_pixel_aux *aux,
                     aic_frame_info *info) {
    if (!c || !f || (n && (!pixels || !out))) return fail(c, AIC_ERR_INVALID, "aic_trace_pixels: bad argument");
    if (info) std::memset(info, 0, sizeof(*info));
    const bool on_device = (mode & AIC_PIXELS_DEVICE) != 0, in_place = (mode & AIC_PIXELS_IN_PLACE) != 0;
    const bool split = (f->flags & AIC_FRAME_OUT_SPLIT) != 0, floats = (f->flags & (AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF)) != 0;
    if (in_place && !on_device) return fail(c, AIC_ERR_INVALID, "aic_trace_pixels: AIC_PIXELS_IN_PLACE needs AIC_PIXELS_DEVICE");
    if (f->flags & AIC_FRAME_BLOOM) return fail(c, AIC_ERR_UNSUPPORTED, "aic_trace_pixels: AIC_FRAME_BLOOM needs a whole frame");
    if (f->partition.n_parts > 1u) return fail(c, AIC_ERR_UNSUPPORTED, "aic_trace_pixels: the pixels are those of the whole frame (partition.n_parts <= 1)");
    if (split && floats) return fail(c, AIC_ERR_INVALID, "aic_trace_pixels: AIC_FRAME_OUT_SPLIT excludes AIC_FRAME_OUT_LINEAR and AIC_FRAME_OUT_COLORBUF");
    if (f->width > 65535u || f->height > 65535u) return fail(c, AIC_ERR_INVALID, "aic_trace_pixels: frame dimensions above 65535 are not supported");
    if (!(f->world.exposure >= 0.f) || !(f->ui.exposure >= 0.f)) return fail(c, AIC_ERR_INVALID, "aic_trace_pixels: exposure is negative or NaN");
    const size_t out_align = split ? 8u : (floats ? 16u : 4u);
    if (on_device && (((uintptr_t)pixels & 3u) || ((uintptr_t)out & (out_align - 1u)) || ((uintptr_t)aux & 7u)))
        return fail(c, AIC_ERR_INVALID, "aic_trace_pixels: AIC_PIXELS_DEVICE wants pixels, out and aux at their element's boundary (Split: 8 bytes, float outputs: 16)");
    if (!n) return AIC_OK;
    const uint32_t count = f->width * f->height;  // (< 2^32: both at most 65535)
    if (!on_device)
        for (uint32_t i = 0; i < n; i++)
            if (pixels[i] >= count) return fail(c, AIC_ERR_INVALID, "aic_trace_pixels: a listed pixel is outside the frame");
    aic_frame_desc g = *f;
    if (const int rc = batch_image(c, "aic_trace_pixels", "pixels", n, &g)) return rc;
    if (const int rc = begin_on_slot0(c, "aic_trace_pixels")) return rc;
    if (!count) return AIC_OK;  // (a device list over an empty viewport: every entry is outside it)
    g.flags = (f->flags & (AIC_FRAME_COUNTERS | AIC_FRAME_OUT_LINEAR | AIC_FRAME_OUT_COLORBUF | AIC_FRAME_OUT_SPLIT | AIC_FRAME_PIXEL_CENTERS)) | (aux ? AIC_FRAME_AUX : 0u);
    g.tuning = 0;
    PixelList px{pixels, n, f->width, f->height, in_place, on_device ? reinterpret_cast<DevAux *>(aux) : nullptr};
    hipStream_t stream = c->slots[0].stream;
    const size_t px_words = floats ? 4 : (split ? 3 : 1);  // (compact Split: [n] colour texels, then [n] depths -- contiguous, one copy)
    if (!on_device) {
        if (const int rc = size_staging(c, (size_t)n * px_words, (size_t)n * 4)) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->staging.p, pixels, (size_t)n * 4, hipMemcpyHostToDevice, stream));
        px.pixels = (const uint32_t *)c->staging.p;
    }
    uint32_t *const target = on_device ? (uint32_t *)out : c->out.p;
    Traced batch;
    batch.px = &px;
    const int rc = submit_frame(c, &g, target, 0, true, batch);
    if (rc != AIC_OK) return rc;
    if (!on_device) HIP_TRY(c, hipMemcpyAsync(out, c->out.p, (size_t)n * px_words * 4, hipMemcpyDeviceToHost, stream));
    return finish_listed(c, n, !on_device, aux, info);
}

// PixelPicker::new (raytrace_to_texture.rs:856-891). sort_by_key is stable; the keys are small non-negative integers, so a counting sort gives the same order.
int aic_pixel_order(uint32_t width, uint32_t height, uint32_t *order, uint32_t *central, uint64_t *cycle_length) {
    const uint64_t count = (uint64_t)width * height;
    if (count > 0xffffffffull) return AIC_ERR_INVALID;  // (a pixel index is a uint32_t)
    const uint64_t n_central = std::min<uint64_t>(60000u, count / 4u);
    if (central) *central = (uint32_t)n_central;
    if (cycle_length) *cycle_length = std::max(n_central, count - n_central) * 2u;
    if (!order || !count) return AIC_OK;
    const double cx = (double)width / 2.0 - 0.5, cy = (double)height / 2.0 - 0.5;
    auto key_of = [&](uint32_t x, uint32_t y) -> int64_t {
        const double blend = (double)(((x ^ y) % 4u) * 2u);
        const double square_radius = std::fmax(std::fabs((double)x - cx), std::fabs((double)y - cy));
        return (int64_t)(square_radius + blend);
    };
    std::vector<uint32_t> start((size_t)std::max(width, height) / 2u + 9u, 0u);  // key <= max(cx, cy) + 6
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) start[(size_t)key_of(x, y) + 1u]++;
    for (size_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) order[start[(size_t)key_of(x, y)]++] = y * width + x;
    return AIC_OK;
}

int aic_render_submit(aic_ctx *c, const aic_frame_desc *f, void *out_device, uint32_t slot) {
    if (!c || !f || slot >= AIC_MAX_IN_FLIGHT) return fail(c, AIC_ERR_INVALID, "aic_render_submit: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->slots[slot].busy) return fail(c, AIC_ERR_INVALID, "aic_render_submit: slot busy (aic_render_wait it first)");
    { const int rs = ensure_slot(c, slot); if (rs != AIC_OK) return rs; }
    c->streaming_submit = true;
    const int rc = submit_frame(c, f, (uint32_t *)out_device, slot, false);
    c->streaming_submit = false;
    return rc;
}

int aic_render_submit_batch(aic_ctx *c, uint32_t n_frames, const aic_frame_desc *frames, void *const *out_devices, uint32_t slot) {
    if (!c || !frames || !out_devices || slot >= AIC_MAX_IN_FLIGHT) return fail(c, AIC_ERR_INVALID, "aic_render_submit_batch: bad argument");
    if (n_frames != 1u && n_frames != 2u && n_frames != 4u && n_frames != 8u) return fail(c, AIC_ERR_INVALID, "aic_render_submit_batch: 1, 2, 4 or 8 frames per launch");
    for (uint32_t j = 1; j < n_frames; j++) {
        const aic_frame_desc &a = frames[0], &b = frames[j];
        if (a.width != b.width || a.height != b.height || a.flags != b.flags || a.tuning != b.tuning || std::memcmp(&a.partition, &b.partition, sizeof(a.partition)) != 0)
            return fail(c, AIC_ERR_INVALID, "aic_render_submit_batch: the frames of a batch share size, partition, flags and tuning");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->slots[slot].busy) return fail(c, AIC_ERR_INVALID, "aic_render_submit_batch: slot busy (aic_render_wait it first)");
    { const int rs = ensure_slot(c, slot); if (rs != AIC_OK) return rs; }
    uint32_t *outs[kMaxSub];
    for (uint32_t j = 0; j < n_frames; j++) outs[j] = (uint32_t *)out_devices[j];
    c->streaming_submit = true;
    const int rc = submit_frames(c, n_frames, frames, outs, slot, false);
    c->streaming_submit = false;
    return rc;
}

int aic_render_wait(aic_ctx *c, uint32_t slot, aic_frame_info *info) {
    if (!c || slot >= AIC_MAX_IN_FLIGHT) return fail(c, AIC_ERR_INVALID, "aic_render_wait: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    return wait_frame(c, slot, info);
}

int aic_render_wait_batch(aic_ctx *c, uint32_t slot, uint32_t n_frames, aic_frame_info *infos) {
    if (!c || slot >= AIC_MAX_IN_FLIGHT || (n_frames && !infos)) return fail(c, AIC_ERR_INVALID, "aic_render_wait_batch: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    return wait_frame(c, slot, nullptr, false, infos, n_frames);
}

}  // extern "C"
