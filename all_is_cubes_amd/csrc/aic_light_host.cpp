// aic_light_host.cpp -- the host half of the light updater: the update itself. Of aic_abi.cpp it uses what aic_ctx.h declares; what
// it shares with the light updater's other units (the chart, compute_derived, the entry points) and gives the rest of the library is aic_light_host.h.
//
// What runs where (see aic_light.h): the priority queue, fast_evaluate_light and apply_light_update are sequential
// by definition and run here; compute_light -- the ray-bundle tree walk, all of the arithmetic -- runs on the
// device for a batch of queue entries at a time (aic_light.hip). Follows
//   all-is-cubes/src/space/light/queue.rs             LightUpdateQueue (aic_light_queue.h)
//   all-is-cubes/src/space/light/updater.rs:181-361   update_light_from_queue, apply_light_update
//   all-is-cubes/src/space/light/updater.rs:537-581   fast_evaluate_light

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "aic_light_host.h"

using namespace aic;

namespace {

// data.rs:214-218 PackedLight::scalar_in (f32::log2 is libm's log2f)
inline uint32_t h_scalar_in(float value) {
    const float x = std::round(std::log2(value) * 10.0f + 144.0f);
    if (x != x) return 0u;
    if (x <= 0.f) return 0u;
    if (x >= 255.f) return 255u;
    return (uint32_t)x;
}
inline uint32_t texel_guess(const float v[3]) { return h_scalar_in(v[0]) | (h_scalar_in(v[1]) << 8) | (h_scalar_in(v[2]) << 16); }  // data.rs guess(): status Uninitialized

}  // namespace

namespace aic {

void light_state_cubes_updated(LightState *s, uint64_t version_before, uint64_t version_after, uint32_t n, const int32_t *xyz, const uint16_t *block_index,
                               const uint8_t *light) {
    if (!s || s->version != version_before) return;  // mirrors absent or already stale: light_prepare will re-read everything
    for (uint32_t k = 0; k < n; k++) {
        size_t idx;
        if (!s->geom.index(I3h{xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]}, &idx)) continue;  // the scatter kernel skips these too
        if (block_index) s->grid[idx] = block_index[k];
        if (light) {
            s->light[idx] = (uint32_t)light[4 * k] | ((uint32_t)light[4 * k + 1] << 8) | ((uint32_t)light[4 * k + 2] << 16) | ((uint32_t)light[4 * k + 3] << 24);
            s->report.caller_wrote(s->light, (uint32_t)idx);
        }
    }
    s->version = version_after;
}
void light_state_free(LightState *s) {
    if (!s) return;
    s->release();
    delete s;
}

}  // namespace aic

namespace {

struct LightRun {
    LightState &S;
    LightQueue &queue;
    explicit LightRun(LightState &s) : S(s), queue(*s.queue) {}
    const DevDerived *evaluated(const I3h &c) const {  // UpdateCtx::get_evaluated; null = outside = AIR
        size_t i;
        if (!S.geom.index(c, &i)) return nullptr;
        return &S.derived[S.grid[i]];
    }
    void light_needs_update(const I3h &c, int priority) {
        size_t i;
        if (S.geom.index(c, &i)) queue.insert((uint32_t)i, priority);
    }
};

// updater.rs:537-581 fast_evaluate_light: columns from the top, sky light until something opaque
void fast_evaluate_light_h(LightRun &R, const uint32_t block_sky[7]) {
    LightState &S = R.S;
    R.queue.clear();
    const LightGeom &g = S.geom;
    for (int x = g.lo[0]; x < g.lo[0] + g.size[0]; x++)
        for (int z = g.lo[2]; z < g.lo[2] + g.size[2]; z++) {
            bool covered = false;
            for (int y = g.lo[1] + g.size[1] - 1; y >= g.lo[1]; y--) {
                size_t idx = 0;
                g.index(I3h{x, y, z}, &idx);
                const DevDerived &ev = S.derived[S.grid[idx]];
                uint32_t v;
                if (d_opaque_for_light(ev)) {
                    covered = true;
                    v = kTexelOpaque;
                } else {
                    bool any = d_visible(ev);
                    for (int f = 0; f < 6 && !any; f++) {
                        const I3h n = face_normal_h(f);
                        const DevDerived *nb = R.evaluated(I3h{x + n[0], y + n[1], z + n[2]});
                        any = nb && d_visible(*nb);
                    }
                    if (any) {
                        R.queue.insert((uint32_t)idx, kPriorityEstimated);
                        v = covered ? kTexelUninit : block_sky[4];  // in_direction(Face::PY)
                    } else {
                        v = kTexelNoRays;
                    }
                }
                S.light[idx] = v;
            }
        }
}

// updater.rs:295-362 apply_light_update; `deps` are the in-bounds dependencies of the computation, in order
int apply_light_update_h(LightRun &R, uint32_t ci, uint32_t new_texel, const uint32_t *deps, size_t n_deps, std::vector<uint32_t> &changed) {
    LightState &S = R.S;
    const uint32_t old = S.light[ci];
    const int diff = texel_difference(new_texel, old);
    if (diff > 0) {
        S.light[ci] = new_texel;
        changed.push_back(ci);
        const I3h cube = S.geom.cube_of(ci);
        for (int f = 0; f < 6; f++) {
            const I3h n = face_normal_h(f);
            const I3h nc = {cube[0] + n[0], cube[1] + n[1], cube[2] + n[2]};
            size_t ni;
            if (!S.geom.index(nc, &ni)) continue;
            uint32_t &nl = S.light[ni];
            if ((nl >> 24) == 0u) {  // Uninitialized: take a guess from the neighbour that just got a value
                if (nl == new_texel) continue;
                if (d_all_opaque(S.derived[S.grid[ni]])) continue;
                const float v[3] = {S.lut[new_texel & 255u], S.lut[(new_texel >> 8) & 255u], S.lut[(new_texel >> 16) & 255u]};
                nl = texel_guess(v);
                changed.push_back((uint32_t)ni);
            }
        }
        if (diff > 1) {
            const int priority = priority_from_difference(diff);
            for (size_t k = 0; k < n_deps; k++) R.queue.insert(deps[k], priority);
        }
    }
    return diff;
}

}  // namespace

namespace aic {

int light_prepare(aic_ctx *c, Layer &l, LightState &S, const uint32_t *vol) {
    if (!vol) vol = l.light.p;
    hipError_t e;
    const size_t n = l.n_cubes();
    if (!S.d_chart.p) {
        const LightChart &ch = light_chart();
        if ((e = S.d_chart.ensure(ch.nodes.size())) != hipSuccess) return hip_fail(c, "alloc light chart", e);
        HIP_TRY(c, hipMemcpy(S.d_chart.p, ch.nodes.data(), ch.nodes.size() * sizeof(DevLightNode), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(S.lut, c->lut.p, sizeof(S.lut), hipMemcpyDeviceToHost));
    }
    if (S.version == l.version) return AIC_OK;
    for (int a = 0; a < 3; a++) { S.geom.lo[a] = l.lo[a]; S.geom.size[a] = l.size[a]; }
    S.grid.resize(n);
    std::vector<uint32_t> before;  // the mirror as it was, if the light report has something pending (LightReport::report_reread)
    if (S.report.report_serial == l.upload_serial && S.light.size() == n && (S.report.cand_all || !S.report.cand.empty())) before = S.light;
    S.light.resize(n);
    if (n) {
        HIP_TRY(c, hipMemcpy(S.grid.data(), l.pool.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(S.light.data(), vol, n * 4, hipMemcpyDeviceToHost));
        if (l.cls_in_code)
            for (size_t i = 0; i < n; i++) S.grid[i] &= (uint16_t)kCubeIndexMask;
    }
    { const int rc = light_prepare_derived(c, l, &S.derived); if (rc != AIC_OK) return rc; }
    if ((e = S.d_derived.ensure(std::max<size_t>(S.derived.size(), 1))) != hipSuccess) return hip_fail(c, "alloc derived", e);
    if (!S.derived.empty()) HIP_TRY(c, hipMemcpy(S.d_derived.p, S.derived.data(), S.derived.size() * sizeof(DevDerived), hipMemcpyHostToDevice));
    S.report.report_reread(S.light, l.upload_serial, before);
    S.version = l.version;
    return AIC_OK;
}

// The layer's update queue: kept across calls, started afresh when a new space was uploaded or another order is asked for.
void light_queue_for(Layer &l, LightState &S, int width) {
    if (!S.queue || S.queue_width != width || S.upload_serial != l.upload_serial || S.queue->by_cube.size() != S.light.size()) {
        delete S.queue;
        S.queue = new LightQueue(S.light.size(), width);
        S.queue_width = width;
        S.upload_serial = l.upload_serial;
    }
    S.queue->geom = &S.geom;
}

void light_update_failed(LightState &S, std::initializer_list<LightOwed> owed) {
    S.version = ~0ull;
    S.report.reread_own = true;
    for (const LightOwed &list : owed)
        for (size_t k = 0; k < list.n; k++) S.queue->insert(list.cubes[k], kPriorityNewlyVisible);
}

}  // namespace aic

namespace {

// ------------------------------------------------------------------------------------
// One update call, step by step: evaluate_light_on (below) is the batch loop, LightCall owns what its steps share.

// -DAIC_LIGHT_TIMING: where the time of a call went, on stderr when it ends. The steps mark their laps with AIC_LAP and
// count with AIC_TIMED; without the flag both are nothing.
#ifdef AIC_LIGHT_TIMING
struct LightLaps {
    uint64_t timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // host side, microseconds: 0 setup (before the first batch), 1 pop + submit, 2 wait for the batch, 3 second copy back, 4 apply, 5 scatter / hand to prep
    double host_us[6] = {0, 0, 0, 0, 0, 0};
    uint64_t n_wants_deps = 0;
    std::chrono::steady_clock::time_point t_mark;
    void start(std::chrono::steady_clock::time_point t_begin) {
        t_mark = std::chrono::steady_clock::now();
        host_us[0] = std::chrono::duration<double, std::micro>(t_mark - t_begin).count();
    }
    void lap(int bucket) {
        const auto t = std::chrono::steady_clock::now();
        host_us[bucket] += std::chrono::duration<double, std::micro>(t - t_mark).count();
        t_mark = t;
    }
    void print(const aic_light_info &out) const {
        std::fprintf(stderr, "light timing: cubes %llu; per cube: walk %.0f ticks, reduction %.0f; levels %.1f, visits %.1f; of the walk, expansion %.0f ticks; deps %.1f\n",
                     (unsigned long long)out.updates, 64.0 * timing[2] / out.updates, 64.0 * timing[3] / out.updates,
                     (double)timing[4] / out.updates, (double)timing[5] / out.updates, 64.0 * timing[6] / (double)out.updates, timing[7] / (double)out.updates);
        std::fprintf(stderr, "light host us: updates %llu batches %llu setup %.1f submit %.1f wait %.1f copy2 %.1f apply %.1f scatter %.1f device_ms %.3f\n",
                     (unsigned long long)out.updates, (unsigned long long)out.batches, host_us[0], host_us[1], host_us[2], host_us[3], host_us[4], host_us[5], out.device_ms);
        std::fprintf(stderr, "light deps wanted: %llu of %llu updates\n", (unsigned long long)n_wants_deps, (unsigned long long)out.updates);
    }
};
#define AIC_LAP(b) laps.lap(b)
#define AIC_TIMED(stmt) stmt
#else
struct LightLaps {};
#define AIC_LAP(b) ((void)0)
#define AIC_TIMED(stmt) ((void)0)
#endif

// what the wave-per-cube kernel keeps in LDS beside its bitmaps (~17 KB of tables), and the LDS of a CU
constexpr size_t kLightWaveStaticLds = 18u << 10, kLightCuLds = (size_t)160 << 10;

// The effective tree of a maximum_distance, and what the wave-per-cube kernel's walk reads of it, made and uploaded.
int upload_light_tree(aic_ctx *c, LightState &S, int maximum_distance) {
    hipError_t e;
    std::vector<float> child_w;
    std::vector<uint32_t> child_pos;
    const std::vector<DevTreePos> tree = build_light_tree(maximum_distance, &S.tree_depth, &child_w, &child_pos);
    if ((e = S.d_tree.ensure(tree.size())) != hipSuccess) return hip_fail(c, "alloc light tree", e);
    if ((e = S.d_child_w.ensure(child_w.size())) != hipSuccess) return hip_fail(c, "alloc light tree", e);
    // What the walk's expansion pass needs of a child without reading the child's record: its position, which of its
    // weights are positive (the chart's weights are never negative, so `(weight * direction_weights).sum() > 0` is
    // "some selected weight is positive"), its face-entered / beyond-the-distance bits and its cube offset.
    std::vector<uint2> child_ent(child_pos.size());
    std::vector<uint4> node(tree.size());
    if (tree.size() >= (1u << 22)) return fail(c, AIC_ERR_INVALID, "aic_evaluate_light: maximum_distance too large");
    auto weight_mask = [&](uint32_t pos) {
        uint32_t m = 0;
        for (int f = 0; f < 6; f++) m |= (tree[pos].weight[f] > 0.f ? 1u : 0u) << f;
        return m;
    };
    for (size_t k = 0; k < tree.size(); k++)
        for (int f = 0; f < 6; f++)
            if (!(tree[k].weight[f] >= 0.f)) return fail(c, AIC_ERR_INVALID, "aic_evaluate_light: negative chart weight");
    for (size_t q = 0; q < child_pos.size(); q++) {
        const uint32_t cp = child_pos[q];
        child_ent[q] = cp ? make_uint2(cp | (weight_mask(cp) << 22) | ((tree[cp].info & 15u) << 28), tree[cp].offset) : make_uint2(0u, 0u);
    }
    // the walk's queue holds the root and the children of branching positions (a single child is followed at once)
    S.n_front = 1;
    for (size_t k = 0; k < tree.size(); k++) {
        uint32_t nch = 0;
        uint2 only = make_uint2(0u, 0u);
        for (int f = 0; f < 6; f++)
            if (child_ent[k * 6 + (size_t)f].x) { nch++; only = child_ent[k * 6 + (size_t)f]; }
        node[k] = make_uint4(only.x, only.y, nch, 0u);
        if (nch > 1) S.n_front += nch;
    }
    S.root_meta = (tree[0].info & 15u) | (weight_mask(0) << 4);
    if ((e = S.d_node.ensure(node.size())) != hipSuccess) return hip_fail(c, "alloc light tree", e);
    HIP_TRY(c, hipMemcpy(S.d_node.p, node.data(), node.size() * sizeof(uint4), hipMemcpyHostToDevice));
    if ((e = S.d_child_ent.ensure(child_ent.size())) != hipSuccess) return hip_fail(c, "alloc light tree", e);
    HIP_TRY(c, hipMemcpy(S.d_tree.p, tree.data(), tree.size() * sizeof(DevTreePos), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(S.d_child_w.p, child_w.data(), child_w.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(S.d_child_ent.p, child_ent.data(), child_ent.size() * sizeof(uint2), hipMemcpyHostToDevice));
    S.tree_size = (uint32_t)tree.size();
    S.tree_distance = maximum_distance;
    return AIC_OK;
}

struct LightCall {
    aic_ctx *const c;
    Layer &l;
    LightState &S;
    const aic_light_params *const p;
    uint32_t *const vol;  // the device volume the update works on
    const hipStream_t ls;
    LightRun R;
    std::vector<uint32_t> cubes, changed, deps, scatter;  // (the destructor's body reads them on its way out; members go after it)
    LightPrep prep;  // the light texels the last batch changed, not yet on the device: they ride with the next batch's preparation launch
    LightJob J;
    aic_light_info out;
    LightLaps laps;
    // how the call runs (size_buffers, prepare_session)
    uint32_t batch = 1, lanes = 64, threads_per_cube = 256, n_waves = 0;
    size_t res_chunks = 0;
    bool by_wave = true, pinned = false, use_session = false;
    bool session_live = false;
    // the batch being computed (compute_batch)
    bool head_cleared = false, prep_in_flight = false;
    const uint32_t *res_host = nullptr;
    bool ok = false;  // set by finish()

    LightCall(aic_ctx *c_, Layer &l_, LightState &S_, const aic_light_params *p_, uint32_t *vol_) : c(c_), l(l_), S(S_), p(p_), vol(vol_), ls(c_->upload_stream), R(S_) {
        std::memset(&prep, 0, sizeof(prep));
        std::memset(&J, 0, sizeof(J));
        std::memset(&out, 0, sizeof(out));
    }
    // Every way out ends the session (a kernel left waiting would end itself, but only after its patience), and that BEFORE the
    // stream is synchronised below. Then every error return leaves through the rest: the host mirrors may be
    // ahead of the device (texels applied but not yet scattered) and a popped batch may be lost, so the failure rule applies
    // (light_update_failed) to the cubes whose results never reached the device: the popped batch (until it is applied),
    // `changed`, and prep's pending scatter.
    ~LightCall() {
        (void)session_end();
        if (ok) return;
        // (the new half of the double buffer may still be the target of copies / scatters / walks queued on `ls`: frames submitted next read it
        //  from their own streams, which do not wait for `ls` -- ADVICE r04)
        (void)hipStreamSynchronize(ls);
        light_update_failed(S, {{cubes.data(), cubes.size()}, {changed.data(), changed.size()}, {prep.scatter_index, prep.n_scatter}});
    }

    // What the call adds to the layer's queue: Mutation::fast_evaluate_light, or the caller's entries (n_queue < 0: every uninitialised cube).
    int fill_queue() {
        const size_t n = l.n_cubes();
        if (p->fast) {
            fast_evaluate_light_h(R, l.block_sky);
            S.report.cand_clear();  // every texel was written: a full relight is measured against the whole baseline
            S.report.cand_all = true;
            if (n) HIP_TRY(c, hipMemcpyAsync(vol, S.light.data(), n * 4, hipMemcpyHostToDevice, ls));
        } else {
            if (p->n_queue < 0)
                for (size_t i = 0; i < n; i++)
                    if ((S.light[i] >> 24) == 0u) R.queue.insert((uint32_t)i, kPriorityUninit);
            for (int32_t k = 0; k < p->n_queue; k++)
                R.light_needs_update(I3h{p->queue_cubes[3 * k], p->queue_cubes[3 * k + 1], p->queue_cubes[3 * k + 2]}, p->queue_priorities[k]);
        }
        return AIC_OK;
    }

    int ensure_pinned(size_t words) {
        if (S.h_pin_words >= words) return AIC_OK;
        if (S.h_pin) (void)hipHostFree(S.h_pin);
        S.h_pin = nullptr;
        S.h_pin_words = 0;
        void *ptr = nullptr;
        hipError_t e2 = hipHostMalloc(&ptr, words * 4, hipHostMallocCoherent);  // (coherent: a session's host reads it while the kernel is still running)
        if (e2 != hipSuccess) return hip_fail(c, "alloc pinned light results", e2);
        S.h_pin = static_cast<uint32_t *>(ptr);
        S.h_pin_words = words;
        return AIC_OK;
    }

    // Which kernel route the call takes, and the device (and pinned) buffers of the size its batches need.
    int size_buffers() {
        batch = (uint32_t)std::max(1, p->batch);
        lanes = (batch + 63u) & ~63u;
        hipError_t e;
        if ((e = S.d_cubes.ensure(lanes)) != hipSuccess) return hip_fail(c, "alloc light batch", e);
        // The counters (8 words) and the per-cube results (4 words each) live in the first `res_chunks` chunks of the
        // dependency pool, so that one copy brings back everything a batch produced.
        res_chunks = (8 + (size_t)lanes * 4 + kLightDepChunk - 1) / kLightDepChunk;
        by_wave = p->lanes_per_cube != 1;
        static const int default_lanes = [] { const char *e = std::getenv("AIC_LIGHT_LANES"); return e ? std::atoi(e) : 0; }();
        threads_per_cube = (p->lanes_per_cube ? p->lanes_per_cube : default_lanes) == 64 ? 64u : 256u;
        if (by_wave) {
            if (S.tree_distance != p->maximum_distance) { int rc = upload_light_tree(c, S, p->maximum_distance); if (rc != AIC_OK) return rc; }
            // resident waves: what the kernel's LDS (bitmaps of 7 bits per tree position + ~17 KB of tables) lets a CU hold,
            // within 4 GiB of per-block arrays (76 bytes per tree position + the queue)
            const size_t lds = (size_t)light_wave_bitmap_words(S.tree_size) * 4u + kLightWaveStaticLds;
            const size_t per_cu = std::max<size_t>(1, kLightCuLds / lds);
            const size_t per_wave = (size_t)S.tree_size * 76u + (size_t)S.n_front * 16u;
            n_waves = (uint32_t)std::min<size_t>(std::min<size_t>(batch, (size_t)c->n_cus * per_cu), std::max<size_t>(1, ((size_t)4 << 30) / per_wave));
            if ((e = S.d_terms.ensure((size_t)n_waves * 4u * S.tree_size)) != hipSuccess) return hip_fail(c, "alloc light terms", e);
            if ((e = S.d_cands.ensure((size_t)n_waves * 2u * S.tree_size)) != hipSuccess) return hip_fail(c, "alloc light candidates", e);
            {
                const uint4 *before = S.d_front.p;
                const size_t cap_before = S.d_front.cap;
                if ((e = S.d_front.ensure((size_t)n_waves * S.n_front)) != hipSuccess) return hip_fail(c, "alloc light queue", e);
                if (S.d_front.p != before || S.d_front.cap != cap_before)  // the kernel leaves the queue zeroed; a new one starts zeroed
                    HIP_TRY(c, hipMemsetAsync(S.d_front.p, 0, S.d_front.cap * sizeof(uint4), ls));
            }
            if ((e = S.d_valpha.ensure((size_t)n_waves * S.tree_size)) != hipSuccess) return hip_fail(c, "alloc light visit alphas", e);
        } else if ((e = S.d_stack.ensure((size_t)lanes * kLightFrameWords * (light_chart().depth + 1))) != hipSuccess) return hip_fail(c, "alloc light stack", e);
        if ((e = S.d_scatter.ensure((size_t)lanes * 14 + 64)) != hipSuccess) return hip_fail(c, "alloc light scatter", e);
        // Eight chunks (504 dependencies) per cube to start with; a batch that needs more grows the pool and is computed again.
        // aic_light_params.hooks bits 8-23 (a test hook) start a fresh layer with that many chunks instead.
        size_t pool_chunks = (size_t)lanes * 8;
        if (const uint32_t hook_chunks = ((uint32_t)p->hooks >> AIC_LIGHT_HOOK_POOL_SHIFT) & 0xffffu) pool_chunks = (size_t)hook_chunks;
        if (S.d_dep_pool.cap < (pool_chunks + res_chunks) * kLightDepChunk)
            if ((e = S.d_dep_pool.ensure((pool_chunks + res_chunks) * kLightDepChunk)) != hipSuccess) return hip_fail(c, "alloc light dependencies", e);
        S.d_dep_pool.n = S.d_dep_pool.cap;
        // A small batch's results (a few tens of KB) are written by the kernel straight into pinned host memory: no copy back.
        // Only the allocator's counters stay on the device (its atomics would be slow across PCIe).
        pinned = by_wave && batch <= kLightPrepMax;
        if (pinned) { int rc = ensure_pinned((pool_chunks + res_chunks) * kLightDepChunk); if (rc != AIC_OK) return rc; }
        return AIC_OK;
    }

    // What a kernel of this call reads of the layer and of the state, whatever the batch.
    void fill_job() {
        J.grid = l.pool.p;
        J.index_mask = l.cls_in_code ? kCubeIndexMask : 0xffffu;
        J.light = vol;
        J.derived = S.d_derived.p;
        J.n_blocks = (uint32_t)S.derived.size();
        J.chart = S.d_chart.p;
        J.lut = c->lut.p;
        for (int a = 0; a < 3; a++) { J.lo[a] = l.lo[a]; J.size[a] = l.size[a]; }
        std::memcpy(J.block_sky, l.block_sky, sizeof(J.block_sky));
        J.max_dist_sq = (double)p->maximum_distance * (double)p->maximum_distance;
        J.cubes = S.d_cubes.p;
        J.stack = S.d_stack.p;
        J.stack_stride = lanes;
        J.max_depth = light_chart().depth + 1;
        if (by_wave) {
            J.tree = S.d_tree.p;
            J.n_tree = S.tree_size;
            J.child_w = S.d_child_w.p;
            J.child_ent = S.d_child_ent.p;
            J.node = S.d_node.p;
            J.root_meta = S.root_meta;
            J.terms = S.d_terms.p;
            J.cands = S.d_cands.p;
            J.front = S.d_front.p;
            J.n_front = S.n_front;
            J.valpha = S.d_valpha.p;
        }
    }

    // Where a batch's results go. The allocator's counters are on the device; a pinned batch's kernel writes results and
    // dependency chunks to host memory itself, any other leaves them behind the counters for the copy back.
    void aim_results() {
        uint32_t *const res = S.d_dep_pool.p;
        J.dep_head = res;
        if (pinned) {
            J.done_count = res + 8;
            J.host_head = S.h_pin;
            J.out = S.h_pin + 8;
            J.dep_pool = S.h_pin + res_chunks * kLightDepChunk;
            J.dep_chunks = (uint32_t)std::min<size_t>(S.h_pin_words / kLightDepChunk - res_chunks, 0x7fffffffu);
        } else {
            J.done_count = nullptr;
            J.host_head = nullptr;
            J.out = res + 8;
            J.dep_pool = res + res_chunks * kLightDepChunk;
            J.dep_chunks = (uint32_t)std::min<size_t>(S.d_dep_pool.cap / kLightDepChunk - res_chunks, 0x7fffffffu);
        }
    }
    // the dependency chunks that come back with a batch's first copy
    size_t first_chunks() const { return std::min<size_t>(std::min<size_t>(J.dep_chunks, (size_t)cubes.size() * 8), 4096); }

    // `scatter` holds m cube indices and then their m texels: onto the device they go, and into the volume.
    int send_scatter(size_t m) {
        hipError_t e;
        if ((e = S.d_scatter.ensure(2 * m)) != hipSuccess) return hip_fail(c, "alloc light scatter", e);
        HIP_TRY(c, hipMemcpyAsync(S.d_scatter.p, scatter.data(), 2 * m * 4, hipMemcpyHostToDevice, ls));
        launch_scatter_light(vol, S.d_scatter.p, S.d_scatter.p + m, (uint32_t)m, ls);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(ls));  // `scatter` is pageable and reused; and the texels are on the device from here on
        return AIC_OK;
    }
    // what `prep` still holds, for a batch (or an end of the call) that has no preparation launch to carry it
    int flush_prep() {
        const uint32_t m = prep.n_scatter;
        if (!m) return AIC_OK;
        scatter.resize(2 * (size_t)m);
        for (uint32_t k = 0; k < m; k++) { scatter[k] = prep.scatter_index[k]; scatter[m + k] = prep.scatter_texel[k]; }
        { int rc = send_scatter(m); if (rc != AIC_OK) return rc; }
        prep.n_scatter = 0;
        return AIC_OK;
    }

    // Sessions (AIC_LIGHT_SESSION=1, read per call; off by default): small batches are served by ONE launch per call
    // (compute_light_session_kernel) -- the batches go to it, and their results come back, through pinned host memory
    // (LightMailbox, aic_light.h): no dispatch, no refill of the XCDs' L2s and no hipStreamSynchronize wake-up per batch. One
    // workgroup per cube of a batch, all resident at once (n_waves is what fits). Built for VERDICT r03's "completion word
    // polled from a pinned host page"; measured, it changes nothing (profiles/r04_experiments.txt J: the host's share of a
    // batch falls by 6 us and the walk, now reading its texels past the L2, takes 7 us longer -- a batch is the walk's own
    // dependent chain, not its launch), so the launch per batch stays the default and this stays as the experiment it was.
    int prepare_session() {
        use_session = pinned && n_waves >= batch && (p->hooks & AIC_LIGHT_HOOK_SESSION) != 0;
        if (!use_session) return AIC_OK;
        if (!S.mailbox) {
            void *ptr = nullptr;
            hipError_t e2 = hipHostMalloc(&ptr, sizeof(LightMailbox), hipHostMallocCoherent);
            if (e2 != hipSuccess) return hip_fail(c, "alloc light mailbox", e2);
            S.mailbox = static_cast<LightMailbox *>(ptr);
            std::memset(S.mailbox, 0, sizeof(LightMailbox));
        }
        if (!S.d_session.p) {
            hipError_t e;
            if ((e = S.d_session.ensure(2)) != hipSuccess) return hip_fail(c, "alloc light session word", e);
            HIP_TRY(c, hipMemsetAsync(S.d_session.p, 0, 8, ls));
        }
        if (S.wall_clock_khz == 0.0) {
            int khz = 0;
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;
            S.wall_clock_khz = (double)khz;
        }
        return AIC_OK;
    }
    uint32_t next_seq() { if (++S.session_seq == 0u) ++S.session_seq; return S.session_seq; }
    int session_start(uint32_t first_seq) {
        aim_results();
        J.mailbox = S.mailbox;
        J.session_word = S.d_session.p;
        J.session_cubes = S.d_cubes.p;
        J.light_rw = vol;
        J.session_seq = first_seq;
        J.coherent_light = 1u;
        J.n = 0u;
        __atomic_store_n(&S.mailbox->exited, 0u, __ATOMIC_RELAXED);
        __atomic_store_n(&S.mailbox->error, 0u, __ATOMIC_RELEASE);
        HIP_TRY(c, hipMemsetAsync(S.d_dep_pool.p, 0, 36, ls));
        launch_compute_light_session(J, batch, threads_per_cube, ls);
        HIP_TRY(c, hipGetLastError());
        (void)hipStreamQuery(ls);  // (a nudge: the launch must reach the device now, the host is about to wait on memory, not on the stream)
        session_live = true;
        return AIC_OK;
    }
    int session_end() {
        if (!session_live) return AIC_OK;
        session_live = false;
        S.mailbox->n_cubes = 0u;
        S.mailbox->n_scatter = 0u;
        __atomic_store_n(&S.mailbox->seq, next_seq(), __ATOMIC_RELEASE);
        HIP_TRY(c, hipStreamSynchronize(ls));
        return AIC_OK;
    }

    // One batch through the session's mailbox (a new session first, if none is live); *flag: what the kernel says of the batch (settle_batch).
    int compute_by_session(uint32_t *flag) {
        if (!session_live) { int rc = session_start(S.session_seq + 1u == 0u ? 1u : S.session_seq + 1u); if (rc != AIC_OK) return rc; }
        LightMailbox *const mb = S.mailbox;
        mb->n_cubes = (uint32_t)cubes.size();
        std::memcpy(mb->cubes, cubes.data(), cubes.size() * 4);
        mb->n_scatter = prep.n_scatter;
        std::memcpy(mb->scatter_index, prep.scatter_index, (size_t)prep.n_scatter * 4);
        std::memcpy(mb->scatter_texel, prep.scatter_texel, (size_t)prep.n_scatter * 4);
        prep_in_flight = prep.n_scatter != 0u;
        const uint32_t seq = next_seq();
        __atomic_store_n(&mb->seq, seq, __ATOMIC_RELEASE);
        AIC_LAP(1);
        const auto t_posted = std::chrono::steady_clock::now();
        for (uint32_t spins = 1;; spins++) {
            if (__atomic_load_n(&mb->done, __ATOMIC_ACQUIRE) == seq) break;
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            if ((spins & 1023u) != 0u) continue;
            if (__atomic_load_n(&mb->error, __ATOMIC_ACQUIRE) != 0u) return fail(c, AIC_ERR_DEVICE, "aic_evaluate_light: the session's workgroups lost each other");
            if (__atomic_load_n(&mb->exited, __ATOMIC_ACQUIRE) == seq) {
                // the kernel gave up waiting before this batch was posted (a host held up for half a second): start another one on the same batch
                session_live = false;
                HIP_TRY(c, hipStreamSynchronize(ls));
                int rc = session_start(seq);
                if (rc != AIC_OK) return rc;
                continue;
            }
            const hipError_t q = hipStreamQuery(ls);
            if (q != hipErrorNotReady && q != hipSuccess) return hip_fail(c, "light session", q);
            if (std::chrono::steady_clock::now() - t_posted > std::chrono::seconds(20)) return fail(c, AIC_ERR_DEVICE, "aic_evaluate_light: no answer from the session kernel");
        }
        AIC_LAP(2);
        if (prep_in_flight) { prep.n_scatter = 0; prep_in_flight = false; }
        res_host = S.h_pin;
        out.device_ms += (double)(mb->t_done - mb->t_seen) / S.wall_clock_khz;
        *flag = res_host[1];
        return AIC_OK;
    }

    // One batch by a launch of its own: cubes and pending texels to the device, the kernel, the results back; *flag as above.
    int compute_by_launch(uint32_t *flag) {
        uint32_t *const res = S.d_dep_pool.p;
        aim_results();
        if (!head_cleared && cubes.size() <= kLightPrepMax) {
            // small batch: the last batch's texels, these cubes and the cleared counters in one launch's arguments
            prep.light = vol;
            prep.cubes_out = S.d_cubes.p;
            prep.head = res;
            prep.n_cubes = (uint32_t)cubes.size();
            std::memcpy(prep.cubes, cubes.data(), cubes.size() * 4);
            launch_prepare_light_batch(prep, ls);
            HIP_TRY(c, hipGetLastError());
            prep_in_flight = true;  // its texels count as delivered only once the batch's sync below has succeeded
        } else {
            if (!head_cleared) {
                { int rc = flush_prep(); if (rc != AIC_OK) return rc; }
                HIP_TRY(c, hipMemcpyAsync(S.d_cubes.p, cubes.data(), cubes.size() * 4, hipMemcpyHostToDevice, ls));
            }
            HIP_TRY(c, hipMemsetAsync(res, 0, 36, ls));
        }
        head_cleared = true;
        HIP_TRY(c, hipEventRecord(S.ev0, ls));  // (the state's own events: slot 0's may belong to a frame in flight)
        if (by_wave) launch_compute_light_waves(J, std::min<uint32_t>(n_waves, J.n), threads_per_cube, ls);
        else launch_compute_light(J, ls);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(S.ev1, ls));
        // one round trip per batch: the counters, the per-cube results and a first stretch of the dependency chunks come
        // back in one copy; the rest of the chunks only if the batch wrote more than that (settle_batch)
        if (!pinned) {
            const size_t first_words = (res_chunks + first_chunks()) * kLightDepChunk;
            if (S.h_res.size() < first_words) S.h_res.resize(first_words);
            HIP_TRY(c, hipMemcpyAsync(S.h_res.data(), res, first_words * 4, hipMemcpyDeviceToHost, ls));
        }
        AIC_LAP(1);
        HIP_TRY(c, hipStreamSynchronize(ls));
        AIC_LAP(2);
        if (prep_in_flight) { prep.n_scatter = 0; prep_in_flight = false; }  // until here a failure requeues them (~LightCall reads prep)
        res_host = pinned ? S.h_pin : S.h_res.data();
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, S.ev0, S.ev1) == hipSuccess) out.device_ms += (double)ms;
        *flag = res_host[1];
        return AIC_OK;
    }

    // What a batch's flag means, whichever route computed it: 2 and 3 are the walk's failures; 0 is done (*done), and what the
    // first copy back left on the device is fetched; anything else says the dependency pool ran out: it grows fourfold (up to
    // 1 GiB of pinned or 8 GiB of device memory) and the caller computes the batch again.
    int settle_batch(uint32_t flag, bool *done) {
        if (flag == 2u) return fail(c, AIC_ERR_DEVICE, "aic_evaluate_light: tree walk stack overflow");
        if (flag == 3u) {
            { int rc = session_end(); if (rc != AIC_OK) return rc; }
            (void)hipMemsetAsync(S.d_front.p, 0, S.d_front.cap * sizeof(uint4), ls);
            return fail(c, AIC_ERR_DEVICE, "aic_evaluate_light: tree walk did not terminate");
        }
        if (flag == 0u) {
            const size_t used = res_host[0], first = first_chunks();
            if (!pinned && used > first) {
                if (S.h_res.size() < (res_chunks + used) * kLightDepChunk) S.h_res.resize((res_chunks + used) * kLightDepChunk);
                HIP_TRY(c, hipMemcpyAsync(S.h_res.data() + (res_chunks + first) * kLightDepChunk, J.dep_pool + first * kLightDepChunk,
                                          (used - first) * kLightDepChunk * 4, hipMemcpyDeviceToHost, ls));
                HIP_TRY(c, hipStreamSynchronize(ls));
                res_host = S.h_res.data();
            }
            *done = true;
            return AIC_OK;
        }
        // the dependency pool ran out: the session (if there is one) ends, the pool grows, the batch is computed again (by another session)
        { int rc = session_end(); if (rc != AIC_OK) return rc; }
        if (pinned) {
            const size_t want_words = S.h_pin_words * 4;
            if (want_words * 4 > (size_t)1 << 30) return fail(c, AIC_ERR_OOM, "aic_evaluate_light: dependency lists exceed 1 GiB of pinned memory");
            return ensure_pinned(want_words);
        }
        const size_t want = S.d_dep_pool.cap * 4;
        if (want * 4 > (size_t)8 << 30) return fail(c, AIC_ERR_OOM, "aic_evaluate_light: dependency lists exceed 8 GiB");
        const hipError_t e = S.d_dep_pool.ensure(want);
        if (e != hipSuccess) return hip_fail(c, "alloc light dependencies", e);
        S.d_dep_pool.n = S.d_dep_pool.cap;
        return AIC_OK;
    }

    // the next batch off the queue, into `cubes`; false: the queue is empty
    bool pop_batch() {
        cubes.clear();
        for (uint32_t k = 0; k < batch; k++) {  // max_updates is checked between batches, like a time budget
            uint32_t idx;
            if (!R.queue.pop(&idx)) break;
            cubes.push_back(idx);
        }
        return !cubes.empty();
    }

    // `cubes` computed on the device, again with a larger pool as often as it takes: res_host is what came back.
    int compute_batch() {
        J.n = (uint32_t)cubes.size();
        head_cleared = prep_in_flight = false;
        res_host = nullptr;
        for (bool done = false; !done;) {
            uint32_t flag = 0;
            { int rc = use_session ? compute_by_session(&flag) : compute_by_launch(&flag); if (rc != AIC_OK) return rc; }
            { int rc = settle_batch(flag, &done); if (rc != AIC_OK) return rc; }
        }
        AIC_LAP(3);
        AIC_TIMED(for (int q = 2; q < 8; q++) laps.timing[q] += res_host[q]);
        return AIC_OK;
    }

    // update_light_from_queue's sequential half: each cube's result applied to the host mirror in queue order, its
    // dependencies re-queued, the texels that moved collected in `changed`.
    void apply_batch() {
        const uint32_t *const h_out = res_host + 8, *const h_deps = res_host + res_chunks * kLightDepChunk;
        changed.clear();
        for (size_t k = 0; k < cubes.size(); k++) {
            const uint32_t *o = &h_out[4 * k];
            deps.clear();
            // the dependencies are only re-queued when the texel moves by more than one unit (apply_light_update_h): most updates of a
            // converging volume do not, and their lists (~190 cubes each) need not be walked out of the chunks at all
            const bool wants_deps = texel_difference(o[0], S.light[cubes[k]]) > 1;
            AIC_TIMED(laps.n_wants_deps += wants_deps ? 1u : 0u);
            uint32_t chunk = o[2], left = wants_deps ? o[1] : 0u;
            while (left) {
                const uint32_t *ck = &h_deps[(size_t)chunk * kLightDepChunk];
                const uint32_t take = std::min(left, kLightDepChunk - 1u);
                deps.insert(deps.end(), ck + 1, ck + 1 + take);
                left -= take;
                chunk = ck[0];
            }
            apply_light_update_h(R, cubes[k], o[0], deps.data(), deps.size(), changed);
            out.cost += o[3];
            out.updates++;
        }
        cubes.clear();  // applied: no longer owed to the queue if a later step fails
        AIC_LAP(4);
        out.bundles_visited += res_host[5];  // counted by the wave-per-cube kernel (0 from the lane-per-cube one)
        out.batches++;
    }

    // The texels the batch changed, on their way to the device: a few ride in `prep` with the next batch's launch, more go now.
    int deliver_changed() {
        if (!changed.empty()) {
            std::sort(changed.begin(), changed.end());
            changed.erase(std::unique(changed.begin(), changed.end()), changed.end());
            const size_t m = changed.size();
            for (uint32_t idx : changed) S.report.cand_add(idx);  // what aic_light_changed_count may report
            if (m <= kLightPrepMax) {
                prep.n_scatter = (uint32_t)m;
                for (size_t k = 0; k < m; k++) { prep.scatter_index[k] = changed[k]; prep.scatter_texel[k] = S.light[changed[k]]; }
            } else {
                { int rc = session_end(); if (rc != AIC_OK) return rc; }  // (the stream is the session's while it lasts)
                scatter.resize(2 * m);
                for (size_t k = 0; k < m; k++) { scatter[k] = changed[k]; scatter[m + k] = S.light[changed[k]]; }
                { int rc = send_scatter(m); if (rc != AIC_OK) return rc; }
            }
            changed.clear();  // handed to `prep` (rides with the next launch) or on the device
        }
        AIC_LAP(5);
        return AIC_OK;
    }

    // the queue is drained or the budget spent: the session ends, the last texels go out, and the device has it all
    int finish() {
        { int rc = session_end(); if (rc != AIC_OK) return rc; }
        { int rc = flush_prep(); if (rc != AIC_OK) return rc; }
        HIP_TRY(c, hipStreamSynchronize(ls));
        ok = true;
        AIC_TIMED(laps.print(out));
        return AIC_OK;
    }
};

}  // namespace

namespace aic {

// The update itself, against the device volume `vol` (the layer's current one, or the spare a submitted update works on).
int evaluate_light_on(aic_ctx *c, int layer, const aic_light_params *p, aic_light_info *info, uint32_t *vol) {
    Layer &l = c->layers[layer];
    const auto t_begin = std::chrono::steady_clock::now();
    if (!l.lstate) l.lstate = new LightState();
    LightState &S = *l.lstate;
    if (!S.ev0) { HIP_TRY(c, hipEventCreate(&S.ev0)); HIP_TRY(c, hipEventCreate(&S.ev1)); }
    { int rc = light_prepare(c, l, S, vol); if (rc != AIC_OK) return rc; }
    light_queue_for(l, S, p->queue_order);
    LightCall K(c, l, S, p, vol);  // (every return below leaves through its destructor)
    { int rc = K.fill_queue(); if (rc != AIC_OK) return rc; }
    { int rc = K.size_buffers(); if (rc != AIC_OK) return rc; }
    K.fill_job();
    const int eps = priority_from_difference(p->epsilon);
    const uint64_t max_updates = p->max_updates ? p->max_updates : ~0ull;
    AIC_TIMED(K.laps.start(t_begin));
    { int rc = K.prepare_session(); if (rc != AIC_OK) return rc; }
    while (K.out.updates < max_updates) {
        if (K.R.queue.peek_priority() <= eps) break;
        if (!K.pop_batch()) break;
        { int rc = K.compute_batch(); if (rc != AIC_OK) return rc; }
        K.apply_batch();
        { int rc = K.deliver_changed(); if (rc != AIC_OK) return rc; }
    }
    { int rc = K.finish(); if (rc != AIC_OK) return rc; }
    K.out.queue_left = (uint32_t)K.R.queue.len;
    K.out.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (info) *info = K.out;
    return AIC_OK;
}

// the worker thread of aic_evaluate_light_submit: one update at a time, as the caller hands them over
void light_worker_main(aic_ctx *c) {
    aic_ctx::LightJob &J = c->ljob;
    (void)hipSetDevice(c->device);
    tl_err_sink = &J.err;
    std::unique_lock<std::mutex> lk(J.mu);
    for (;;) {
        J.cv.wait(lk, [&] { return J.has_work || J.quit; });
        if (J.quit) return;
        J.has_work = false;
        J.running = true;
        lk.unlock();
        aic_light_params p = J.params;
        p.queue_cubes = J.queue_cubes.empty() ? nullptr : J.queue_cubes.data();
        p.queue_priorities = J.queue_priorities.empty() ? nullptr : J.queue_priorities.data();
        J.err.clear();
        const int rc = evaluate_light_on(c, J.layer, &p, &J.info, c->layers[J.layer].light_spare[J.spare].p);
        lk.lock();
        J.rc = rc;
        J.running = false;
        J.cv.notify_all();
    }
}

// Ends a submitted light update, if there is one, and PUBLISHES it: the spare volume it worked on becomes the layer's. Called by aic_evaluate_light_wait and by
// every call that needs the scene or the light still (quiesce, the light entry points, aic_destroy). Its outcome stays with the job for aic_evaluate_light_wait.
int light_job_finish(aic_ctx *c) {
    aic_ctx::LightJob &J = c->ljob;
    if (!J.pending) return AIC_OK;
    {
        std::unique_lock<std::mutex> lk(J.mu);
        J.cv.wait(lk, [&] { return !J.has_work && !J.running; });
    }
    J.pending = false;
    J.result_ready = true;
    Layer &l = c->layers[J.layer];
    if (J.rc == AIC_OK && J.spare >= 0) std::swap(l.light, l.light_spare[J.spare]);  // (a failed update leaves the layer's volume as it was; its mirrors were marked stale)
    J.spare = -1;
    return AIC_OK;
}

}  // namespace aic
