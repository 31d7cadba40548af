// aic_ctx.h -- what the translation units of the C ABI's host side share: the context behind the opaque `aic_ctx` of
// include/aic_hip.h, its layers and device buffers, the error helpers and the call recorder. Internal: included by aic_abi.cpp
// (context, scene, options, strips, probes), aic_frame.cpp (the frame path: submit, wait and the entry points that trace),
// aic_split_ops.cpp (reprojection, picking, presentation and export of a resident Split frame), the light updater's units (through aic_light_host.h, which declares what they share and offer) and
// aic_ray_queries.cpp (the luminance sampler's call and the cursor raycast's) and aic_light_rays_host.cpp (the light-ray records' call), aic_cells_host.cpp (the terminal's cells) and aic_grid_replace_host.cpp (scene inputs from device memory) only (all of them are written inside `using namespace aic`, and so is this header). Whatever one of the
// files uses alone stays in that file's anonymous namespace; what is declared here lives in namespace aic, like the kernel
// launchers they call.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aic_hip.h"
#include "aic_device.h"

namespace aic {

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;    // elements in use
    size_t cap = 0;  // elements allocated
    hipError_t ensure(size_t count, bool keep = false, hipStream_t stream = nullptr) {
        if (count <= cap) { n = count; return hipSuccess; }
        size_t new_cap = count + count / 4 + 16;
        T *np_ = nullptr;
        hipError_t e = hipMalloc((void **)&np_, new_cap * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep && p && cap) {
            e = hipMemcpyAsync(np_, p, cap * sizeof(T), hipMemcpyDeviceToDevice, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) {
                (void)hipFree(np_);
                return e;
            }
        }
        if (p) (void)hipFree(p);
        p = np_;
        cap = new_cap;
        n = count;  // only now: a failed grow leaves the buffer as it was
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = cap = 0;
    }
};

struct LightState;                       // aic_light_host.h, with everything else the light host code offers; a Layer only owns one
void light_state_free(LightState *s);

struct Layer {
    bool present = false;
    int32_t lo[3] = {0, 0, 0}, size[3] = {0, 0, 0};
    DevBuf<uint16_t> pool;   // [0, n_cubes): cube grid; then the voxel volumes of the recursive blocks
    DevBuf<uint32_t> cls;    // 2-bit block classes
    std::vector<uint32_t> host_cls;
    DevBuf<uint32_t> light;
    // Spare light volumes: a new volume (aic_update_light_volume, aic_evaluate_light beside frames in flight) is made in one NO frame in flight reads and
    // becomes current for the frames submitted from then on. Two halves (rounds 2-5) made every update wait for the frame submitted two updates before --
    // a sim + render loop with four frames in flight was held to two --, so there are as many spares as it takes (up to kLightSpares), made on demand.
    static constexpr int kLightSpares = 7;
    DevBuf<uint32_t> light_spare[kLightSpares];
    DevBuf<DevBlock> blocks;
    DevBuf<DevPaletteEntry> palette;
    std::vector<DevBlock> host_blocks;  // mirror of the block table (for replace/append)
    // per block: elements of the voxel pool / palette pool its current ranges can hold (so that a re-evaluated block is
    // written in place when it fits, updating.rs:128-145), and what replaced blocks left behind (compacted past a threshold)
    // vox_base / pal_base: where the block's reserved ranges start. Kept apart from host_blocks[i].vox_off / pal_off, which are
    // 0 while the block has no voxels (an atom written over a voxel block keeps its reservation for the next re-evaluation).
    std::vector<uint32_t> vox_cap, pal_cap, vox_base, pal_base;
    uint64_t garbage_vox = 0, garbage_pal = 0;
    int32_t air_index = -1;
    int32_t sky_kind = 0;
    float sky[8][3] = {};
    uint32_t block_sky[7] = {};
    aic_options opt;
    bool opt_set = false;
    bool cls_in_code = false;  // cube-grid entries carry a tag in bits 14-15: the block class, and which invisible cubes are open (aic_device.h)
    uint64_t version = 0;      // bumped by every scene mutation; the light updater's host mirrors follow it
    uint64_t upload_serial = 0;  // bumped by aic_upload_space only: the light update queue lives as long as one upload
    LightState *lstate = nullptr;
    // aic_sample_luminance: one bit per block index, EvaluatedBlock::visible() (light_visible_bits), made by the first sample after `version` moved
    DevBuf<uint32_t> visible_bits;
    uint64_t visible_version = ~0ull;  // the `version` visible_bits describes
    size_t n_cubes() const { return (size_t)size[0] * (size_t)size[1] * (size_t)size[2]; }
    void release() {
        pool.release(); cls.release(); light.release(); blocks.release(); palette.release(); visible_bits.release();
        visible_version = ~0ull;
        for (auto &sp : light_spare) sp.release();
        host_blocks.clear(); host_cls.clear(); vox_cap.clear(); pal_cap.clear(); vox_base.clear(); pal_base.clear();
        garbage_vox = garbage_pal = 0;
        present = false;
        version++;
        light_state_free(lstate);
        lstate = nullptr;
    }
};

}  // namespace aic

using namespace aic;

struct aic_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t upload_stream = nullptr;  // light-volume uploads run beside the frames in flight
    Layer layers[2];
    DevBuf<float> lut;
    DevBuf<float> srgb_thr;         // the 256 sRGB8 thresholds (bloom and presentation kernels)
    DevBuf<uint32_t> srgb_buckets;  // the same as a bucket table (aic_encode.h): what the trace kernels encode from
    DevBuf<uint32_t> out;      // internal RGBA8 target when the caller wants a host copy
    DevBuf<DevAux> aux;
    DevBuf<unsigned char> staging;  // scratch for scatter updates / probes
    DevBuf<DevOrthoView> ortho_views;  // aic_render_orthographic
    DevBuf<unsigned char> reproject_scratch;  // aic_reproject_split: keys, splat image, mips, counters (aic_reproject.h)
    // the size of the last successful aic_reproject_split: the splat image R it left in reproject_scratch is what aic_pick_pixels reads (0 x 0: none)
    uint32_t reproject_valid_w = 0, reproject_valid_h = 0;
    DevBuf<uint32_t> pick_scratch;  // aic_pick_pixels: the record read back, then the scan blocks' counts and offsets (aic_pick.h)
    DevBuf<uint2> present_scratch;  // aic_present_split with bloom: the chain's mips, then the scene texture of a stretched frame (aic_bloom.h)
    // aic_present_split_lines: the key image, the stored scene, the counters, the staged vertices of a host list (aic_present_lines.h)
    DevBuf<unsigned char> lines_scratch;
    // the first lines_keys_clean keys of lines_scratch are all ones (cleared once after an allocation; every finished call leaves them so). 0 after an
    // allocation and while a call that may have failed between its draw and its resolve is the last one: the next call clears first
    size_t lines_keys_clean = 0;
    // aic_set_text_font: the resident font atlas, [16 * text_cell_h][16 * text_cell_w] RGBA8 (n == 0: no font set), and whether its cell 0x20 was all
    // zero, which lets a presentation skip the pixels out of the text's reach; aic_present_split_text: the staged codes of a host list
    DevBuf<uint32_t> text_atlas;
    uint32_t text_cell_w = 0, text_cell_h = 0, text_margin = 0;
    bool text_space_blank = false;
    DevBuf<unsigned char> text_codes;
    DevBuf<unsigned char> exposure_scratch;  // aic_sample_luminance with host pointers: the staged rays, then the samples
    DevBuf<uint32_t> export_counts;  // aic_export_split: the slots of its statistics (kExportSlots ExportCounts, aic_bloom.h), cleared on the stream by every call
    uint64_t aux_records = 0;
    double depth_zw[4] = {1.0, 0.0, 0.0, 1.0};  // aic_set_depth_transform: the Split frames' depth transform
    bool streaming_submit = false;  // set around aic_render_submit: frames meant to overlap are sized for throughput, synchronous ones for latency
    // frames in flight: slot 0 runs on `stream` (and serves the synchronous aic_render), slot 1 on a
    // second stream so that a submitted frame's trace can start while the previous one drains
    // What each frame of a slot owns. A plain frame is sub-frame 0; aic_render_submit_batch traces up to kMaxSub frames in one launch (DevSub) and each has
    // its own counters, tile queues and cost record.
    struct SubSlot {
        DevBuf<DevCounters> counters;
        DevCounters *host_counters = nullptr;      // pinned
        // What a frame needs cleared or ordered is enqueued BEHIND the previous frame of the slot, not ahead of this one (round 4): the counters
        // are cleared again right after they were copied out, the cost record is turned into the next frame's tile order and cleared as soon as the
        // trace that wrote it is done. A frame alone then starts with its trace launch; before, three small launches (~25 us) stood in front of it.
        bool counters_clean = false;       // the device counters are zero (cleared behind the slot's last frame)
        size_t cost_clean_n = 0;           // this many entries of tile_cost are zero
        bool record_ready = false;         // tile_order / queue_start hold the cost order of the frame described by cost_sig / cost_cam / order_key
        uint32_t order_key[6] = {0, 0, 0, 0, 0, 0};  // cost_sig + number of queues + super-block shift
        DevBuf<float4> acc;  // UI pre-pass accumulators
        DevBuf<double> split_depth;  // ... and every sample's DepthBuf (AIC_FRAME_OUT_SPLIT frames over a UI space)
        // cost feedback: the longest ray of every tile of the sub-frame's last frame, and the tile order made from it
        DevBuf<uint32_t> tile_cost, tile_order, queue_start;
        // AIC_FRAME_BLOOM (on the sub-frame's first bloomed frame): the trace's ColorBuf, then the bloom chain's mips (aic_bloom.h)
        DevBuf<float4> bloom_cb;
        DevBuf<uint2> bloom_mips;
        uint32_t cost_sig[4] = {0, 0, 0, 0};  // width, local rows, partition of the frame tile_cost describes
        double cost_cam[16] = {0};            // ... and its world camera
        void release() {
            counters.release(); acc.release(); split_depth.release(); tile_cost.release(); tile_order.release(); queue_start.release(); bloom_cb.release(); bloom_mips.release();
            if (host_counters) (void)hipHostFree(host_counters);
            host_counters = nullptr;
            counters_clean = record_ready = false; cost_clean_n = 0;
        }
    };
    struct FrameSlot {
        hipStream_t stream = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the trace launch(es): the frame's kernel time
        hipEvent_t ev2 = nullptr;                  // behind the copy of the counters to `host_counters`: what aic_render_wait waits for
        SubSlot sub[kMaxSub];
        uint32_t n_sub = 1;                // frames of the batch in flight
        bool static_ready = false;         // tile_static / queue_static hold the index order for static_key (a matter of the frame's shape: shared by a batch's frames)
        uint32_t static_key[6] = {0, 0, 0, 0, 0, 0};
        DevBuf<uint32_t> tile_static, queue_static;
        DevBuf<uint4> ray_cold;  // the exchanging trace kernels' antialiasing sums in global memory (DevFrame::ray_cold; antialiased frames only)
        DevBuf<double> edges;    // DevFrame::edge_x / edge_y of the slot's frame shape: width + 1, then height + 1 doubles
        uint32_t edges_w = 0, edges_h = 0;
        bool busy = false;
        bool diag = false;  // the slot's frame ran the aux-recording kernel variant
        uint32_t variant = 0, tile_queues = 0;  // what aic_frame_info reports of the slot's frame
        const void *light_used[2] = {nullptr, nullptr};  // per layer: the light buffer the slot's frame reads
        uint32_t flaws = 0, local_rows = 0;
        size_t npix = 0;
        std::chrono::steady_clock::time_point t_begin;
    } slots[AIC_MAX_IN_FLIGHT];
    std::string err;
    std::FILE *dump = nullptr;  // AIC_DUMP=path: every scene / options / frame argument is appended here
    char devname[256] = {0};
    uint32_t n_cus = 256;
    // aic_evaluate_light_submit / _wait: ONE light update at a time runs on a worker thread the context owns, against a spare light volume (Layer::light_spare);
    // the frames submitted meanwhile read the volume as it stood. The update is PUBLISHED -- the spare becomes the layer's volume -- by aic_evaluate_light_wait,
    // or by whatever call next needs the scene still (every scene or light call finishes a pending update first: light_job_finish).
    struct LightJob {
        std::thread worker;
        std::mutex mu;
        std::condition_variable cv;
        bool has_work = false, quit = false;   // (under mu)
        bool running = false;                   // (under mu) the worker is inside the update
        bool pending = false;                   // an update was submitted and has not been published yet (caller's thread only)
        bool result_ready = false;              // rc / info / err describe an update aic_evaluate_light_wait has not reported yet
        int layer = 0, spare = -1;
        aic_light_params params;
        std::vector<int32_t> queue_cubes, queue_priorities;
        int rc = AIC_OK;
        aic_light_info info;
        std::string err;
    } ljob;
    // measurement switches, read from the environment ONCE, when the context is made -- nothing on the frame path reads the environment
    struct Switches {
        int tile = 0, macro = 0;         // AIC_TILE, AIC_MACRO: work-tile edge in pixels (8 | 16), tiles per macro tile edge
        bool feedback = true;            // AIC_TILE_FEEDBACK=0: no cost-feedback tile order
        bool wait_whole_stream = false;  // AIC_WAIT_WHOLE_STREAM=1: aic_render_wait drains the slot's stream (rounds 1-3)
        uint32_t tiles_per_wave = 0;     // AIC_TILES_PER_WAVE: grid sizing of streamed frames smaller than the chip
        std::string wave_prof;           // AIC_WAVE_PROF (-DAIC_PROFILE builds): file for the per-wave clocks
        bool lines_clear_keys = false;   // AIC_LINES_CLEAR_KEYS=1: every aic_present_split_lines clears its whole key image first instead of resetting the keys it touched
    } sw;
    // (appended: no member the frame path reads moves)
    DevBuf<unsigned char> stale_scratch;  // aic_pick_stale: the record, the scan blocks' counts and offsets, the bitmap, the rectangles (aic_stale.h)
    DevBuf<unsigned char> cursor_scratch;  // aic_cursor_raycast with host pointers: the staged rays, then the records
    DevBuf<unsigned char> stale_cubes_scratch;  // aic_pick_stale_cubes: the record, the pixel bitmap, the scan blocks' counts, offsets and ballots, the rectangles, the staged boxes and cubes (aic_stale_cubes.h)
    // aic_find_block_cubes, aic_pick_stale_blocks: the record, the set, the workgroups' counts and offsets (aic_stale_blocks.h); the boxes a find hands to
    // the host; the events around a pick's find, made by the first call that needs them
    DevBuf<unsigned char> stale_blocks_scratch;
    DevBuf<int32_t> stale_blocks_boxes;
    hipEvent_t stale_blocks_ev[2] = {nullptr, nullptr};
    // aic_light_rays (aic_light_rays_host.cpp): the effective tree of light_rays_distance (tree, children's weights, children's entries); the derived
    // properties of the blocks of light_rays_layer at its version light_rays_version; the call's scratch (staged cubes, counts, offsets, results, infos,
    // totals, record positions, the records and lines of a host list, the walk's slots and queues)
    DevBuf<unsigned char> light_rays_tree, light_rays_derived, light_rays_scratch;
    DevBuf<unsigned char> light_rays_list;  // aic_light_rays_cursor_lines: the caller's lines and the cube's behind them, as aic_present_split_lines takes them
    int light_rays_distance = -1, light_rays_layer = -1;
    uint32_t light_rays_n_tree = 0, light_rays_bound = 0;
    uint64_t light_rays_version = 0;
    // aic_image_cells, aic_render_cells (aic_cells_host.cpp): the branch counters, then the staged image, records and cells of a call with host pointers;
    // the linear frame aic_render_cells traces into (its first-hit records go to `aux`)
    DevBuf<unsigned char> cells_scratch;
    DevBuf<float4> cells_frame;
    // aic_replace_cube_grid (aic_grid_replace_host.cpp): the record, the workgroups' counts, offsets and changes (aic_grid_replace.h); the boxes it hands
    // to the host
    DevBuf<unsigned char> grid_replace_scratch;
    DevBuf<int32_t> grid_replace_boxes;
    hipEvent_t grid_replace_ev[2] = {nullptr, nullptr};  // around its launches (a frame in flight on a slot keeps that slot's events), made by the first call
};

namespace aic {

// (the light worker's failures go to its job's own string, not to the context's last error, which the caller's thread may be writing: see LightJob)
extern thread_local std::string *tl_err_sink;
int fail(aic_ctx *c, int code, const char *what, hipError_t e = hipSuccess);
int hip_fail(aic_ctx *c, const char *what, hipError_t e);
// an AIC_ERR_INVALID refusal under the entry point's name: "<who>: <why>"
inline int reject(aic_ctx *c, const char *who, const char *why) { return fail(c, AIC_ERR_INVALID, (std::string(who) + ": " + why).c_str()); }
#define HIP_TRY(ctx, expr)                                    \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return hip_fail(ctx, #expr, e_); \
    } while (0)

inline bool valid_layer(int l) { return l == AIC_LAYER_WORLD || l == AIC_LAYER_UI; }

// aic_abi.cpp
aic_options default_options();
// the call recorder (AIC_DUMP): appends one record {tag, layer, bytes, payload} to the context's dump file, if it has one
enum DumpTag : uint32_t { DUMP_UPLOAD = 1, DUMP_CLEAR = 2, DUMP_CUBES = 3, DUMP_LIGHT = 4, DUMP_BLOCK = 5, DUMP_OPTIONS = 6, DUMP_FRAME = 7, DUMP_GRID = 8 };
struct DumpPart { const void *p; size_t n; };
void dump_record(aic_ctx *c, uint32_t tag, uint32_t layer, std::initializer_list<DumpPart> parts);
int take_light_spare(aic_ctx *c, Layer &l, int layer, size_t n, int *index);
int quiesce(aic_ctx *c);

}  // namespace aic
