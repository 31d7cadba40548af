// aic_light_host.h -- the light updater's host code, as its own units and the rest of the library see it. Internal, like aic_ctx.h, and written inside
// namespace aic. The units behind it, by subject:
//   aic_light_chart.cpp    the chart generator, the effective tree of a maximum_distance, aic_light_chart            (cold: once per process / distance)
//   aic_light_derived.cpp  compute_derived on the flattened blocks, and the read-back of the voxel and palette pools  (cold: once per scene version)
//   aic_light_host.cpp     the update itself: LightState's mirrors, the batch loop (LightCall), the worker thread
//   aic_light_entry.cpp    the entry points of include/aic_hip.h other than aic_light_chart
// What the batch loop calls once per update or per dependency is inline, here or in the two `std`-only headers: the queue and the geometry
// (aic_light_queue.h), the changed-cube report (aic_light_report.h), the d_* predicates below. The library is built without link-time optimisation.
#pragma once

#include <vector>

#include "aic_ctx.h"
#include "aic_light.h"
#include "aic_light_queue.h"
#include "aic_light_report.h"

namespace aic {

// ------------------------------------------------------------------------------------
// What the rest of the library takes from the light host code.

// aic_light_host.cpp
int light_job_finish(aic_ctx *c);
// keeps the light updater's host mirrors in step with an aic_update_cubes call (no-op if they were not current)
void light_state_cubes_updated(LightState *s, uint64_t version_before, uint64_t version_after, uint32_t n, const int32_t *xyz, const uint16_t *block_index,
                               const uint8_t *light);

// aic_light_derived.cpp
constexpr uint32_t kVisibleBitsWords = 2048;  // 65536 block indices x 1 bit
int light_visible_bits(aic_ctx *c, Layer &l, hipStream_t stream, std::vector<uint32_t> *bits);
// compute_derived of every block of the layer; the voxel and palette pools are read back on `stream` only if a block has voxels.
// (Both calls: `stream` is a stream of the caller's own, whose asynchronous copies are waited for there. A null stream would turn them into blocking
// copies through the null stream, which wait for every blocking stream's work -- light_prepare's way, not meant for these callers.)
int light_rays_derived(aic_ctx *c, Layer &l, hipStream_t stream, std::vector<DevDerived> *out);

// aic_light_chart.cpp
struct LightRaysTree {
    std::vector<DevTreePos> tree;
    std::vector<float> child_w;
    std::vector<uint2> child_ent;
    uint32_t bound = 0;  // aic_light_rays_bound
};
void light_rays_tree(int maximum_distance, LightRaysTree *out);
uint32_t light_rays_bound(int maximum_distance);

// ------------------------------------------------------------------------------------
// What the light units share.

// aic_light_chart.cpp
struct LightChart {
    std::vector<DevLightNode> nodes;
    uint32_t depth = 0;  // the deepest chain of bundles: what the tree walk's stack must hold
};
const LightChart &light_chart();
std::vector<DevTreePos> build_light_tree(int maximum_distance, uint32_t *depth_out, std::vector<float> *child_w, std::vector<uint32_t> *child_pos);

// aic_light_derived.cpp: compute_derived of every block of the layer for light_prepare, the pools read back by blocking copies through the null stream
int light_prepare_derived(aic_ctx *c, Layer &l, std::vector<DevDerived> *out);

inline bool d_all_opaque(const DevDerived &d) { return (d.flags & 63u) == 63u; }
inline bool d_emits(const DevDerived &d) { return !(d.emission[0] == 0.f && d.emission[1] == 0.f && d.emission[2] == 0.f); }
inline bool d_visible(const DevDerived &d) { return (d.flags & kDerivedVisible) != 0u; }
inline bool d_opaque_for_light(const DevDerived &d) { return d_all_opaque(d) && !d_emits(d); }  // updater.rs:1031-1033

// Per-layer state of the light updater: host mirrors of what the sequential half reads, and the device scratch.
struct LightState {
    uint64_t version = ~0ull;  // Layer::version the mirrors were taken at
    LightGeom geom;
    std::vector<uint16_t> grid;     // block index per cube
    std::vector<uint32_t> light;    // texels; kept equal to the device's volume
    std::vector<DevDerived> derived;
    float lut[256];
    DevBuf<DevDerived> d_derived;
    DevBuf<DevLightNode> d_chart;
    DevBuf<uint32_t> d_cubes, d_dep_pool, d_stack, d_scatter;
    // wave-per-cube kernel: the effective tree of one maximum_distance, and per-wave scratch
    int tree_distance = -1;
    uint32_t tree_depth = 0, tree_size = 0;
    DevBuf<DevTreePos> d_tree;
    DevBuf<float> d_child_w;
    DevBuf<float4> d_terms;
    DevBuf<uint32_t> d_cands;
    DevBuf<uint2> d_child_ent;
    DevBuf<uint4> d_front, d_node;
    DevBuf<float> d_valpha;
    uint32_t n_front = 0, root_meta = 0;
    std::vector<uint32_t> h_res;  // what a batch brings back: counters, per-cube results, dependency chunks
    uint32_t *h_pin = nullptr;    // the same for small batches, pinned: the kernel writes its results here itself
    size_t h_pin_words = 0;
    // The update queue lives as long as the uploaded space does (as the reference's Space keeps its LightUpdateQueue):
    // aic_light_cubes_changed adds to it, aic_evaluate_light drains it, possibly over several calls.
    LightQueue *queue = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // device time of a batch
    // Sessions (small batches: one launch per call, batches handed over through `mailbox`; aic_light.h)
    LightMailbox *mailbox = nullptr;  // pinned, coherent
    DevBuf<uint32_t> d_session;       // LightJob::session_word
    uint32_t session_seq = 0;         // the last sequence number posted; never reused within a context
    double wall_clock_khz = 0.0;
    int queue_width = -1;
    uint64_t upload_serial = ~0ull;  // Layer::upload_serial the queue belongs to
    LightReport report;              // what aic_light_changed_count / _take answer from, measured against `light` (aic_light_report.h)
    void release() {
        delete queue;
        queue = nullptr;
        if (h_pin) (void)hipHostFree(h_pin);
        h_pin = nullptr;
        h_pin_words = 0;
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
        if (mailbox) (void)hipHostFree(mailbox);
        mailbox = nullptr;
        d_session.release();
        d_derived.release(); d_chart.release(); d_cubes.release(); d_dep_pool.release();
        d_stack.release(); d_scatter.release(); d_tree.release(); d_child_w.release(); d_terms.release(); d_cands.release(); d_child_ent.release(); d_front.release(); d_node.release(); d_valpha.release();
    }
};

// aic_light_host.cpp
int light_prepare(aic_ctx *c, Layer &l, LightState &S, const uint32_t *vol = nullptr);  // vol: the device volume to mirror (default: the layer's current one)
void light_queue_for(Layer &l, LightState &S, int width);
// A device failure may have left the host mirrors ahead of the device and cubes owed to it: the mirrors are marked stale -- light_prepare re-reads the
// device's volume on the next call, and its report keeps every candidate (LightReport::reread_own) --, and the cubes of `owed`, whose results never
// reached the device, go back into the queue at Priority::NEWLY_VISIBLE (all of them: after a failure the order of these updates is no longer the
// reference's). `owed`: the lists of such cubes, each a pointer and a count, requeued in the order given. S.queue must exist (light_queue_for has run).
struct LightOwed { const uint32_t *cubes; size_t n; };
void light_update_failed(LightState &S, std::initializer_list<LightOwed> owed);
int evaluate_light_on(aic_ctx *c, int layer, const aic_light_params *p, aic_light_info *info, uint32_t *vol);
void light_worker_main(aic_ctx *c);

}  // namespace aic
