// aic_abi.cpp -- host side of the C ABI declared in include/aic_hip.h.
//
// Owns the device-resident snapshot of up to two Spaces (world + UI), i.e. what the
// reference keeps in `RtRenderer.rts: Layers<Option<UpdatingSpaceRaytracer>>`
// (all-is-cubes-render/src/raytracer/renderer.rs:35-54), and launches the kernels of
// aic_trace.hip (aic_launch.h) on a private HIP stream. No CPU rendering path exists here: every entry
// point fails with AIC_ERR_NO_DEVICE / AIC_ERR_DEVICE when HIP is unusable.
// Here: the context, scene upload and update, options, strip assembly, synchronisation and the probes. The frame path -- everything that submits or
// waits for a trace -- is aic_frame.cpp, what acts on a resident Split frame aic_split_ops.cpp, the light updater aic_light_host.cpp and the units beside it (aic_light_host.h).

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../../include/aic_hip.h"
#include "aic_bloom.h"
#include "aic_ctx.h"
#include "aic_device.h"
#include "aic_encode.h"
#include "aic_launch.h"
#include "aic_light_host.h"

using namespace aic;

static_assert(sizeof(aic_pixel_aux) == sizeof(DevAux), "aux record layout");

// Frame slots are HIP streams, and the runtime deals streams onto GPU_MAX_HW_QUEUES hardware queues; streams that share a queue run their kernels one
// behind the other. The library leaves that variable to its host: it changes nothing in the process's environment.
static_assert(sizeof(aic_block_desc) == 48, "aic_block_desc is 48 bytes");

namespace {

constexpr uint64_t kMaxPoolElems = 0x7ffffff0ull;  // u16 elements of cube grid + voxel volumes (32-bit byte offsets in the kernel)
constexpr uint64_t kMaxLightTexels = 0x3ffffff0ull; // cubes of a space: the SHADE event addresses light texels by 32-bit byte offsets (aic_lightmath.h)

}  // namespace

// What the frame path (aic_frame.cpp) and the light host code (aic_light_host.cpp, aic_light_entry.cpp) use too: declared in aic_ctx.h.
namespace aic {

aic_options default_options() {
    // GraphicsOptions::default() (graphics_options.rs:256-280)
    aic_options o;
    std::memset(&o, 0, sizeof(o));
    o.fog = 1;
    o.transparency = 1;
    o.threshold = 0.5f;
    o.lighting = 3;
    o.maximum_intensity = INFINITY;
    o.bloom_intensity = 0.125f;
    o.view_distance = 200.0;
    return o;
}

// ---- call recorder: AIC_DUMP=<path> makes a context append every argument it is given --
// scene snapshots, deltas, options, frame descriptors -- to <path>, verbatim, so that a scene produced by
// the reference (which cannot be generated here) can be captured where the Rust shim runs and replayed
// anywhere (all_is_cubes_amd/replay.py). Layout: "AICDUMP1", then records {u32 tag, u32 layer, u64 bytes, payload}.
void dump_record(aic_ctx *c, uint32_t tag, uint32_t layer, std::initializer_list<DumpPart> parts) {
    if (!c || !c->dump) return;
    uint64_t total = 0;
    for (const DumpPart &d : parts) total += d.p ? d.n : 0;
    std::fwrite(&tag, 4, 1, c->dump);
    std::fwrite(&layer, 4, 1, c->dump);
    std::fwrite(&total, 8, 1, c->dump);
    for (const DumpPart &d : parts)
        if (d.p && d.n) std::fwrite(d.p, 1, d.n, c->dump);
    std::fflush(c->dump);
}

thread_local std::string *tl_err_sink = nullptr;
int fail(aic_ctx *c, int code, const char *what, hipError_t e) {
    if (c) {
        std::string &dst = tl_err_sink ? *tl_err_sink : c->err;
        dst = what;
        if (e != hipSuccess) {
            dst += ": ";
            dst += hipGetErrorString(e);
        }
    }
    return code;
}

int hip_fail(aic_ctx *c, const char *what, hipError_t e) {
    return fail(c, e == hipErrorOutOfMemory ? AIC_ERR_OOM : AIC_ERR_DEVICE, what, e);
}

// A light volume of `n` cubes that no frame in flight reads: an existing spare, else a new one, else -- every spare in use by a frame -- the first one, once
// the frame reading it is done. *index says which (the caller swaps it with Layer::light when its contents are complete).
int take_light_spare(aic_ctx *c, Layer &l, int layer, size_t n, int *index) {
    auto in_use = [&](const DevBuf<uint32_t> &b) {
        for (uint32_t i = 0; i < AIC_MAX_IN_FLIGHT; i++)
            if (c->slots[i].busy && b.p && c->slots[i].light_used[layer] == (const void *)b.p) return true;
        return false;
    };
    int pick = -1;
    for (int k = 0; k < Layer::kLightSpares && pick < 0; k++)
        if (l.light_spare[k].p && l.light_spare[k].cap >= n && !in_use(l.light_spare[k])) pick = k;
    for (int k = 0; k < Layer::kLightSpares && pick < 0; k++)
        if (!l.light_spare[k].p || (l.light_spare[k].cap < n && !in_use(l.light_spare[k]))) pick = k;  // (a buffer of an earlier, smaller space is re-made)
    if (pick < 0) {
        pick = 0;
        for (uint32_t i = 0; i < AIC_MAX_IN_FLIGHT; i++)
            if (c->slots[i].busy && c->slots[i].light_used[layer] == (const void *)l.light_spare[0].p) {
                const hipError_t e = hipStreamSynchronize(c->slots[i].stream);
                if (e != hipSuccess) return fail(c, AIC_ERR_DEVICE, "waiting for a frame that reads a spare light volume", e);
            }
    }
    const hipError_t e = l.light_spare[pick].ensure(n);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? AIC_ERR_OOM : AIC_ERR_DEVICE, "alloc light (spare volume)", e);
    *index = pick;
    return AIC_OK;
}

// Every scene mutation waits for the frames in flight: they read the buffers it is about to change.
int quiesce(aic_ctx *c) {
    { const int rc = light_job_finish(c); if (rc != AIC_OK) return rc; }  // (a light update in flight reads the scene too, and its result is published first)
    for (uint32_t i = 0; i < AIC_MAX_IN_FLIGHT; i++)
        if (c->slots[i].busy) HIP_TRY(c, hipStreamSynchronize(c->slots[i].stream));
    return AIC_OK;
}

}  // namespace aic

namespace {

bool valid_resolution(int r) { return r >= 1 && r <= 128 && (r & (r - 1)) == 0; }

inline uint32_t block_class(const DevBlock &b) { return (b.kind & 255u) ? 2u : ((b.kind & 0x80000000u) ? 0u : 1u); }
inline void set_class(std::vector<uint32_t> &cls, uint32_t index, uint32_t c2) {
    if (cls.size() <= index / 16u) cls.resize(index / 16u + 1u, 0u);
    cls[index / 16u] = (cls[index / 16u] & ~(3u << ((index & 15u) * 2u))) | (c2 << ((index & 15u) * 2u));
}

inline bool invisible(const float *e) { return e[3] == 0.f && e[4] == 0.f && e[5] == 0.f && e[6] == 0.f; }
inline bool selectable_float_ok(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, sizeof(bits));
    return bits == 0u || bits == 0x3f800000u;
}

// Builds the device form of one block: palette reordered "invisible entries first", voxel
// codes remapped accordingly (aic_device.h). Appends to vox/pal pools at the given offsets.
int convert_block(aic_ctx *c, const aic_block_desc &d, const uint16_t *voxels, const float *palette, uint32_t vox_off,
                  uint32_t pal_off, DevBlock *out, std::vector<uint16_t> *vox_out, std::vector<DevPaletteEntry> *pal_out) {
    std::memset(out, 0, sizeof(*out));
    if (!valid_resolution(d.resolution)) return fail(c, AIC_ERR_INVALID, "block resolution must be a power of two in 1..128");
    const bool one = (d.flags & AIC_BLOCK_ONE) != 0;
    const bool voxel_flag = (d.flags & AIC_BLOCK_VOXEL_SELECTABLE) != 0;
    size_t nvox = one ? 1 : (size_t)d.vsize[0] * (size_t)d.vsize[1] * (size_t)d.vsize[2];
    for (int a = 0; a < 3 && !one; a++) {
        if (d.vsize[a] < 0 || d.vlo[a] < 0 || d.vlo[a] + d.vsize[a] > d.resolution)
            return fail(c, AIC_ERR_INVALID, "block voxel bounds exceed GridAab::for_block(resolution)");
    }
    if (d.pal_len == 0 && nvox > 0) return fail(c, AIC_ERR_INVALID, "block has voxels but an empty palette");
    if (!palette && (one || d.pal_len > 0)) return fail(c, AIC_ERR_INVALID, "block has a palette length but no palette");
    if (!voxels && !one && nvox > 0) return fail(c, AIC_ERR_INVALID, "block has a voxel volume but no voxels");
    // Evoxel colours are the reference's Rgba = PositiveSign<f32> x 3 + ZeroOne<f32> (math/color.rs:288-314): components that type
    // cannot hold (NaN, negative, alpha above 1) are rejected here, and the kernel's powf / compositing rely on it
    for (uint32_t i = 0; i < (one ? 1u : d.pal_len) && palette; i++) {
        const float *e = palette + 8 * (size_t)i;
        for (int k = 0; k < 7; k++)
            if (!(e[k] >= 0.f)) return fail(c, AIC_ERR_INVALID, "palette entry has a negative or NaN component");
        if (!(e[3] <= 1.f)) return fail(c, AIC_ERR_INVALID, "palette entry has alpha above 1");
        // Evoxel::selectable of a block that carries it: the pattern of 1.0f or of +0.0f
        if (voxel_flag && !selectable_float_ok(e[7])) return fail(c, AIC_ERR_INVALID, "palette entry of an AIC_BLOCK_VOXEL_SELECTABLE block: the eighth float is neither 1.0f nor 0.0f");
    }
    // what aic_cursor_raycast reads (no other kernel does): the block's own attribute -- AIR's says unselectable -- and each voxel's
    const bool block_selectable = !(d.flags & (AIC_BLOCK_UNSELECTABLE | AIC_BLOCK_AIR));
    auto voxel_selectable = [&](const float *e) { return voxel_flag ? e[7] == 1.f : !invisible(e); };
    if (one || d.resolution == 1) {
        // Evoxels::single_voxel() (voxel_storage.rs:364-385)
        const float *e = nullptr;
        static const float air[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (one) e = palette;
        else {
            // indices.get([0,0,0]) or Evoxel::AIR
            bool inb = nvox > 0 && d.vlo[0] <= 0 && d.vlo[1] <= 0 && d.vlo[2] <= 0 && d.vlo[0] + d.vsize[0] > 0 &&
                       d.vlo[1] + d.vsize[1] > 0 && d.vlo[2] + d.vsize[2] > 0;
            if (inb) {
                size_t i = ((size_t)(0 - d.vlo[0]) * d.vsize[1] + (size_t)(0 - d.vlo[1])) * d.vsize[2] + (size_t)(0 - d.vlo[2]);
                uint16_t idx = voxels[i];
                if (idx >= d.pal_len) return fail(c, AIC_ERR_INVALID, "voxel index exceeds palette");
                e = palette + 8 * (size_t)idx;
            } else e = air;
        }
        out->kind = invisible(e) ? 0x80000000u : 0u;
        // (+ 0.0f: a PositiveSign never holds -0.0 -- restricted_number.rs:283 -- and the kernel's ps_mul relies on the sign bit)
        for (int k = 0; k < 4; k++) out->color[k] = e[k] + 0.0f;
        for (int k = 0; k < 3; k++) out->emission[k] = e[4 + k] + 0.0f;
        // (a single voxel: the block's attribute ANDed with the voxel's; the AIR read outside the stored volume is Evoxel::AIR, unselectable either way)
        out->pad[0] = block_selectable && voxel_selectable(e) ? kBlockSelectable : 0u;
        return AIC_OK;
    }
    // recursive block
    std::vector<uint32_t> remap(d.pal_len);
    uint32_t n_inv = 0;
    for (uint32_t i = 0; i < d.pal_len; i++)
        if (invisible(palette + 8 * (size_t)i)) n_inv++;
    uint32_t next_inv = 0, next_vis = n_inv;
    size_t pal_base = pal_out->size();
    pal_out->resize(pal_base + d.pal_len);
    for (uint32_t i = 0; i < d.pal_len; i++) {
        const float *e = palette + 8 * (size_t)i;
        uint32_t dst = invisible(e) ? next_inv++ : next_vis++;
        remap[i] = dst;
        DevPaletteEntry &pe = (*pal_out)[pal_base + dst];
        for (int k = 0; k < 4; k++) pe.color[k] = e[k] + 0.0f;
        for (int k = 0; k < 3; k++) pe.emission[k] = e[4 + k] + 0.0f;
        pe.pad = voxel_selectable(e) ? 1.f : 0.f;
    }
    size_t vox_base = vox_out->size();
    vox_out->resize(vox_base + nvox);
    for (size_t i = 0; i < nvox; i++) {
        uint16_t idx = voxels[i];
        if (idx >= d.pal_len) return fail(c, AIC_ERR_INVALID, "voxel index exceeds palette");
        (*vox_out)[vox_base + i] = (uint16_t)remap[idx];
    }
    out->kind = (uint32_t)d.resolution;
    out->vlo_packed = (uint32_t)d.vlo[0] | ((uint32_t)d.vlo[1] << 8) | ((uint32_t)d.vlo[2] << 16);
    out->vsize_packed = (uint32_t)d.vsize[0] | ((uint32_t)d.vsize[1] << 8) | ((uint32_t)d.vsize[2] << 16);
    out->vox_off = vox_off;
    out->pal_off = pal_off;
    out->n_invisible = n_inv;
    out->pad[0] = block_selectable ? kBlockSelectable : 0u;
    return AIC_OK;
}

}  // namespace

extern "C" {

int aic_abi_version(void) { return AIC_ABI_VERSION; }

aic_ctx *aic_create(int device_id, int *status) {
    int st_dummy;
    if (!status) status = &st_dummy;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        *status = AIC_ERR_NO_DEVICE;
        return nullptr;
    }
    if (device_id < 0) {
        if (hipGetDevice(&device_id) != hipSuccess) device_id = 0;
    }
    if (device_id >= n) {
        *status = AIC_ERR_INVALID;
        return nullptr;
    }
    if (hipSetDevice(device_id) != hipSuccess) {
        *status = AIC_ERR_DEVICE;
        return nullptr;
    }
    aic_ctx *c = new aic_ctx();
    c->device = device_id;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->n_cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) std::snprintf(c->devname, sizeof(c->devname), "%s (%s)", prop.name, prop.gcnArchName);
    {
        auto env_int = [](const char *name, int dflt) { const char *e = std::getenv(name); return e ? std::atoi(e) : dflt; };
        c->sw.tile = env_int("AIC_TILE", 0);
        c->sw.macro = env_int("AIC_MACRO", 0);
        c->sw.feedback = env_int("AIC_TILE_FEEDBACK", 1) != 0;
        c->sw.wait_whole_stream = env_int("AIC_WAIT_WHOLE_STREAM", 0) != 0;
        c->sw.lines_clear_keys = env_int("AIC_LINES_CLEAR_KEYS", 0) != 0;
        c->sw.tiles_per_wave = (uint32_t)std::max(0, env_int("AIC_TILES_PER_WAVE", 0));
        if (const char *p = std::getenv("AIC_WAVE_PROF")) c->sw.wave_prof = p;
    }
    if (const char *path = std::getenv("AIC_DUMP")) {
        static int n_dumps = 0;  // one file per context: <path>, <path>.1, <path>.2 ...
        std::string pth = path;
        if (n_dumps > 0) pth += "." + std::to_string(n_dumps);
        n_dumps++;
        c->dump = std::fopen(pth.c_str(), "wb");
        if (c->dump) std::fwrite("AICDUMP1", 1, 8, c->dump);
    }
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    // the first eight slots are made with the context (as AIC_MAX_IN_FLIGHT = 8 always was: HIP deals streams onto its hardware queues in creation order); slots
    // 8..31 -- a rank's many small shares of a multi-GPU frame -- get their stream and events on first use (ensure_slot)
    for (uint32_t i = 0; ok && i < 8u && i < AIC_MAX_IN_FLIGHT; i++) {
        aic_ctx::FrameSlot &fs = c->slots[i];
        if (i == 0) fs.stream = c->stream;
        else ok = hipStreamCreateWithFlags(&fs.stream, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreate(&fs.ev0) == hipSuccess && hipEventCreate(&fs.ev1) == hipSuccess && hipEventCreate(&fs.ev2) == hipSuccess && fs.sub[0].counters.ensure(1) == hipSuccess;
    }
    // created after the frame streams: HIP deals streams onto a few hardware queues in creation order
    // (4 by default), and two frame slots sharing a queue would serialise their kernels
    ok = ok && hipStreamCreateWithFlags(&c->upload_stream, hipStreamNonBlocking) == hipSuccess;
    // PackedLight decode table: PACKED_LIGHT_SCALAR_LOOKUP_TABLE is *defined* as
    // exp2f((v - 144) / 10) with 0 -> 0 (light/data.rs:239-249, 301-354); correctly rounded.
    float lut[256];
    lut[0] = 0.f;
    for (int v = 1; v < 256; v++) {
        float arg = ((float)v - 144.0f) / 10.0f;
        lut[v] = (float)std::exp2((double)arg);
    }
    ok = ok && c->lut.ensure(256) == hipSuccess && hipMemcpy(c->lut.p, lut, sizeof(lut), hipMemcpyHostToDevice) == hipSuccess;
    // sRGB8 encode thresholds: thr[k] = the smallest f32 c with to_srgb8(c) >= k, found by bisection
    // on the reference formula (color.rs:1038-1054) evaluated here on the host with powf.
    {
        auto enc = [](float cc) -> int {
            float v = cc <= 0.0031308f ? cc * (323.f / 25.f) : (211.f * std::pow(cc, 5.f / 12.f) - 11.f) / 200.f;
            float r = std::round(v * 255.f);
            if (!(r > 0.f)) return 0;
            return r >= 255.f ? 255 : (int)r;
        };
        float thr[256];
        thr[0] = 0.f;
        for (int k = 1; k < 256; k++) {
            uint32_t lo_b = 0u, hi_b = 0x40000000u;  // (0.0, 2.0]: enc(lo) < k <= enc(hi)
            while (hi_b - lo_b > 1u) {
                const uint32_t mid = lo_b + (hi_b - lo_b) / 2u;
                float f;
                std::memcpy(&f, &mid, 4);
                if (enc(f) >= k) hi_b = mid; else lo_b = mid;
            }
            // the bisection assumes enc() is monotone; libm's powf need not be at the last bit, so settle the threshold on
            // the LOWEST float of the neighbourhood that encodes to >= k while its predecessor does not
            for (int back = 0; back < 8 && hi_b > 1u; back++) {
                uint32_t probe = hi_b - 1u;
                float f;
                std::memcpy(&f, &probe, 4);
                bool lower_found = false;
                for (uint32_t d = 0; d < 8u && probe > d; d++) {
                    const uint32_t q = probe - d;
                    std::memcpy(&f, &q, 4);
                    if (enc(f) >= k) { hi_b = q; lower_found = true; }
                }
                if (!lower_found) break;
            }
            std::memcpy(&thr[k], &hi_b, 4);
        }
        ok = ok && c->srgb_thr.ensure(256) == hipSuccess && hipMemcpy(c->srgb_thr.p, thr, sizeof(thr), hipMemcpyHostToDevice) == hipSuccess;
        // ... and as the bucket table the trace kernels read (aic_encode.h). Thresholds that did not fit it would be a libm whose powf is far off.
        uint32_t buckets[kSrgbBucketWords];
        ok = ok && srgb8_bucket_build(thr, buckets) && c->srgb_buckets.ensure(kSrgbBucketWords) == hipSuccess &&
             hipMemcpy(c->srgb_buckets.p, buckets, sizeof(buckets), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        *status = AIC_ERR_DEVICE;
        aic_destroy(c);
        return nullptr;
    }
    for (auto &l : c->layers) l.opt = default_options();
    *status = AIC_OK;
    return c;
}

void aic_destroy(aic_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)light_job_finish(c);  // a light update in flight ends (and is published) before anything it uses is freed ...
    if (c->ljob.worker.joinable()) {  // ... and the worker leaves
        { std::lock_guard<std::mutex> lk(c->ljob.mu); c->ljob.quit = true; }
        c->ljob.cv.notify_all();
        c->ljob.worker.join();
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (uint32_t i = 0; i < AIC_MAX_IN_FLIGHT; i++) {
        aic_ctx::FrameSlot &fs = c->slots[i];
        if (fs.stream) (void)hipStreamSynchronize(fs.stream);
        for (auto &sb : fs.sub) sb.release();
        fs.ray_cold.release(); fs.edges.release();
        if (fs.ev0) (void)hipEventDestroy(fs.ev0);
        if (fs.ev1) (void)hipEventDestroy(fs.ev1);
        if (fs.ev2) (void)hipEventDestroy(fs.ev2);
        fs.tile_static.release(); fs.queue_static.release();
        if (i > 0 && fs.stream) (void)hipStreamDestroy(fs.stream);
    }
    for (auto &l : c->layers) l.release();
    c->lut.release(); c->srgb_thr.release(); c->srgb_buckets.release(); c->out.release(); c->aux.release(); c->staging.release(); c->ortho_views.release(); c->reproject_scratch.release(); c->pick_scratch.release(); c->stale_scratch.release(); c->stale_cubes_scratch.release(); c->stale_blocks_scratch.release(); c->stale_blocks_boxes.release(); c->present_scratch.release(); c->lines_scratch.release();
    c->text_atlas.release(); c->text_codes.release(); c->export_counts.release(); c->exposure_scratch.release(); c->cursor_scratch.release();
    c->light_rays_tree.release(); c->light_rays_derived.release(); c->light_rays_scratch.release(); c->light_rays_list.release();
    c->cells_scratch.release(); c->cells_frame.release();
    c->grid_replace_scratch.release(); c->grid_replace_boxes.release();
    for (hipEvent_t ev : c->stale_blocks_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : c->grid_replace_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->dump) std::fclose(c->dump);
    if (c->upload_stream) (void)hipStreamDestroy(c->upload_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *aic_last_error(const aic_ctx *c) { return c ? c->err.c_str() : "no context"; }

int aic_device_name(const aic_ctx *c, char *buf, uint32_t buf_len) {
    if (!c || !buf || !buf_len) return AIC_ERR_INVALID;
    std::snprintf(buf, buf_len, "%s", c->devname);
    return AIC_OK;
}

int aic_upload_space(aic_ctx *c, int layer, const aic_space_desc *s) {
    if (!c || !s || !valid_layer(layer)) return fail(c, AIC_ERR_INVALID, "aic_upload_space: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    { int qrc = quiesce(c); if (qrc != AIC_OK) return qrc; }
    for (int a = 0; a < 3; a++)
        if (s->size[a] < 0 || (int64_t)s->lo[a] + s->size[a] > 2147483647LL) return fail(c, AIC_ERR_INVALID, "space bounds out of range");
    Layer &l = c->layers[layer];
    const size_t n = (size_t)s->size[0] * (size_t)s->size[1] * (size_t)s->size[2];
    if (n && (!s->block_index || !s->light)) return fail(c, AIC_ERR_INVALID, "space has cubes but no block_index/light");
    if (s->n_blocks > 65536) return fail(c, AIC_ERR_INVALID, "more than 65536 blocks");
    // the trace kernel addresses the pool with 32-bit BYTE offsets: at most 2^31 u16 elements (4 GiB)
    if (n + s->n_voxels > kMaxPoolElems) return fail(c, AIC_ERR_INVALID, "space too large (cube grid + voxel pool must stay within 4 GiB)");
    if (n > kMaxLightTexels) return fail(c, AIC_ERR_INVALID, "space too large (the light volume, 4 bytes per cube, must stay within 4 GiB)");
    if (s->n_blocks && !s->blocks) return fail(c, AIC_ERR_INVALID, "blocks is null");
    // Sky colours are Rgb = PositiveSign<f32> x 3 (sky.rs:20-41): what that type cannot hold is rejected (as for palette entries, make_dev_block)
    for (int o = 0; o < 8; o++)
        for (int k = 0; k < 3; k++)
            if (!(s->sky[o][k] >= 0.f)) return fail(c, AIC_ERR_INVALID, "sky colour has a negative or NaN component");

    // block table + pools
    std::vector<DevBlock> blocks(s->n_blocks);
    std::vector<uint32_t> vox_cap(s->n_blocks, 0u), pal_cap(s->n_blocks, 0u), vox_base(s->n_blocks, 0u), pal_base(s->n_blocks, 0u);
    std::vector<uint16_t> vox;
    std::vector<DevPaletteEntry> pal;
    vox.reserve((size_t)s->n_voxels);
    pal.reserve((size_t)s->n_palette);
    int32_t air_index = -1;
    for (uint32_t i = 0; i < s->n_blocks; i++) {
        const aic_block_desc &d = s->blocks[i];
        const bool one = (d.flags & AIC_BLOCK_ONE) != 0;
        size_t nvox = one ? 1 : (size_t)(d.vsize[0] > 0 ? d.vsize[0] : 0) * (size_t)(d.vsize[1] > 0 ? d.vsize[1] : 0) * (size_t)(d.vsize[2] > 0 ? d.vsize[2] : 0);
        if ((uint64_t)d.vox_off + nvox > s->n_voxels || (uint64_t)d.pal_off + d.pal_len > s->n_palette)
            return fail(c, AIC_ERR_INVALID, "block voxel/palette range exceeds the pools");
        // blocks may alias or overlap ranges of the input pools, so the converted pools can outgrow n_voxels / n_palette:
        // check the running sizes before every conversion (offsets are stored in 32 bits)
        if (n + vox.size() + nvox > kMaxPoolElems || pal.size() + d.pal_len > 0xfffffff0ull) return fail(c, AIC_ERR_INVALID, "pool too large");
        const size_t vb = vox.size(), pb = pal.size();
        int rc = convert_block(c, d, s->voxels ? s->voxels + d.vox_off : nullptr, s->palette ? s->palette + 8 * (size_t)d.pal_off : nullptr,
                               (uint32_t)(n + vox.size()), (uint32_t)pal.size(), &blocks[i], &vox, &pal);
        if (rc != AIC_OK) return rc;
        vox_cap[i] = (uint32_t)(vox.size() - vb);
        pal_cap[i] = (uint32_t)(pal.size() - pb);
        vox_base[i] = (uint32_t)(n + vb);
        pal_base[i] = (uint32_t)pb;
        if ((d.flags & AIC_BLOCK_AIR) && air_index < 0) air_index = (int32_t)i;
    }
    // validate cube indices on the host copy (the reference indexes `blocks[...]` with a bounds check)
    for (size_t i = 0; i < n; i++)
        if (s->block_index[i] >= s->n_blocks) return fail(c, AIC_ERR_INVALID, "cube block index out of range");

    hipError_t e;
    std::vector<uint32_t> cls;
    for (uint32_t i = 0; i < s->n_blocks; i++) set_class(cls, i, block_class(blocks[i]));
    if (cls.empty()) cls.push_back(0u);
    if ((e = l.pool.ensure(n + vox.size())) != hipSuccess) return hip_fail(c, "alloc pool", e);
    if ((e = l.cls.ensure(cls.size())) != hipSuccess) return hip_fail(c, "alloc classes", e);
    if ((e = l.light.ensure(n)) != hipSuccess) return hip_fail(c, "alloc light", e);
    if ((e = l.blocks.ensure(blocks.size())) != hipSuccess) return hip_fail(c, "alloc blocks", e);
    if ((e = l.palette.ensure(pal.size())) != hipSuccess) return hip_fail(c, "alloc palette", e);
    if (n) {
        HIP_TRY(c, hipMemcpyAsync(l.pool.p, s->block_index, n * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(l.light.p, s->light, n * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (!blocks.empty()) HIP_TRY(c, hipMemcpyAsync(l.blocks.p, blocks.data(), blocks.size() * sizeof(DevBlock), hipMemcpyHostToDevice, c->stream));
    if (!vox.empty()) HIP_TRY(c, hipMemcpyAsync(l.pool.p + n, vox.data(), vox.size() * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(l.cls.p, cls.data(), cls.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const bool cls_in_code = s->n_blocks <= kCubeIndexMask + 1u;
    if (cls_in_code) {
        launch_tag_cubes(l.pool.p, n, l.cls.p, 0, 1, c->stream);
        launch_open_cubes(l.pool.p, s->size, c->stream);
    }
    if (!pal.empty()) HIP_TRY(c, hipMemcpyAsync(l.palette.p, pal.data(), pal.size() * sizeof(DevPaletteEntry), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // host buffers may be released on return

    for (int a = 0; a < 3; a++) { l.lo[a] = s->lo[a]; l.size[a] = s->size[a]; }
    l.host_blocks.swap(blocks);
    l.host_cls.swap(cls);
    l.vox_cap.swap(vox_cap);
    l.pal_cap.swap(pal_cap);
    l.vox_base.swap(vox_base);
    l.pal_base.swap(pal_base);
    l.garbage_vox = l.garbage_pal = 0;
    l.air_index = air_index;
    l.sky_kind = s->sky_kind;
    for (int o = 0; o < 8; o++)
        for (int k = 0; k < 3; k++) l.sky[o][k] = s->sky[o][k] + 0.0f;  // (-0.0 becomes +0.0, as in a PositiveSign)
    for (int f = 0; f < 7; f++)
        l.block_sky[f] = (uint32_t)s->block_sky[f][0] | ((uint32_t)s->block_sky[f][1] << 8) | ((uint32_t)s->block_sky[f][2] << 16) |
                         ((uint32_t)s->block_sky[f][3] << 24);
    l.cls_in_code = cls_in_code;
    l.present = true;
    l.version++;
    l.upload_serial++;
    if (c->dump) {
        struct { int32_t lo[3], size[3]; uint32_t n_blocks; int32_t sky_kind; uint64_t n_voxels, n_palette; float sky[8][3]; uint8_t block_sky[7][4]; } h;
        std::memset(&h, 0, sizeof(h));
        for (int a = 0; a < 3; a++) { h.lo[a] = s->lo[a]; h.size[a] = s->size[a]; }
        h.n_blocks = s->n_blocks; h.sky_kind = s->sky_kind; h.n_voxels = s->n_voxels; h.n_palette = s->n_palette;
        std::memcpy(h.sky, s->sky, sizeof(h.sky));
        std::memcpy(h.block_sky, s->block_sky, sizeof(h.block_sky));
        dump_record(c, DUMP_UPLOAD, (uint32_t)layer,
                    {{&h, sizeof(h)}, {s->block_index, n * 2}, {s->light, n * 4}, {s->blocks, (size_t)s->n_blocks * sizeof(aic_block_desc)},
                     {s->voxels, (size_t)s->n_voxels * 2}, {s->palette, (size_t)s->n_palette * 32}});
    }
    return AIC_OK;
}

int aic_clear_space(aic_ctx *c, int layer) {
    if (!c || !valid_layer(layer)) return fail(c, AIC_ERR_INVALID, "aic_clear_space: bad argument");
    { int qrc = quiesce(c); if (qrc != AIC_OK) return qrc; }
    c->layers[layer].present = false;
    dump_record(c, DUMP_CLEAR, (uint32_t)layer, {});
    return AIC_OK;
}

int aic_update_cubes(aic_ctx *c, int layer, uint32_t n, const int32_t *xyz, const uint16_t *block_index, const uint8_t *light) {
    if (!c || !valid_layer(layer) || (n && !xyz)) return fail(c, AIC_ERR_INVALID, "aic_update_cubes: bad argument");
    Layer &l = c->layers[layer];
    if (!l.present) return fail(c, AIC_ERR_INVALID, "aic_update_cubes: no space uploaded for this layer");
    if (!n) return AIC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    { int qrc = quiesce(c); if (qrc != AIC_OK) return qrc; }
    if (block_index)
        for (uint32_t i = 0; i < n; i++)
            if (block_index[i] >= l.host_blocks.size()) return fail(c, AIC_ERR_INVALID, "cube block index out of range");
    const size_t b_xyz = (size_t)n * 12, b_bi = block_index ? (((size_t)n * 2 + 15) & ~(size_t)15) : 0, b_lt = light ? (size_t)n * 4 : 0;
    hipError_t e = c->staging.ensure(b_xyz + b_bi + b_lt + 64);
    if (e != hipSuccess) return hip_fail(c, "alloc staging", e);
    unsigned char *base = c->staging.p;
    HIP_TRY(c, hipMemcpyAsync(base, xyz, b_xyz, hipMemcpyHostToDevice, c->stream));
    if (block_index) HIP_TRY(c, hipMemcpyAsync(base + b_xyz, block_index, (size_t)n * 2, hipMemcpyHostToDevice, c->stream));
    if (light) HIP_TRY(c, hipMemcpyAsync(base + b_xyz + b_bi, light, b_lt, hipMemcpyHostToDevice, c->stream));
    l.version++;
    light_state_cubes_updated(l.lstate, l.version - 1, l.version, n, xyz, block_index, light);
    launch_scatter_cubes(l.pool.p, l.light.p, (const int32_t *)base, block_index ? (const uint16_t *)(base + b_xyz) : nullptr,
                         light ? (const uint32_t *)(base + b_xyz + b_bi) : nullptr, n, l.lo, l.size, l.cls_in_code ? l.cls.p : nullptr, c->stream);
    // the scatter leaves no changed cube OPEN; whether it and its six neighbours are is decided now, from the grid with every change in (no frame is in flight)
    if (block_index && l.cls_in_code) launch_open_changed_cubes(l.pool.p, (const int32_t *)base, n, l.lo, l.size, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    {
        const uint32_t h[4] = {n, block_index ? 1u : 0u, light ? 1u : 0u, 0u};
        dump_record(c, DUMP_CUBES, (uint32_t)layer, {{h, sizeof(h)}, {xyz, (size_t)n * 12}, {block_index, (size_t)n * 2}, {light, (size_t)n * 4}});
    }
    return AIC_OK;
}

// Test probe: the cube grid as it stands on the device -- indices, tags and OPEN marks (aic_device.h) -- and the class table behind the tags. Copies only.
int aic_probe_cube_grid(aic_ctx *c, int layer, uint16_t *out_grid, uint32_t *out_cls, uint32_t *out_tagged) {
    if (!c || !valid_layer(layer) || !out_grid) return fail(c, AIC_ERR_INVALID, "aic_probe_cube_grid: bad argument");
    Layer &l = c->layers[layer];
    if (!l.present) return fail(c, AIC_ERR_INVALID, "aic_probe_cube_grid: no space uploaded for this layer");
    HIP_TRY(c, hipSetDevice(c->device));
    { int qrc = quiesce(c); if (qrc != AIC_OK) return qrc; }
    const size_t n = l.n_cubes(), n_words = (l.host_blocks.size() + 15u) / 16u;
    if (n) HIP_TRY(c, hipMemcpy(out_grid, l.pool.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (out_cls && n_words) HIP_TRY(c, hipMemcpy(out_cls, l.cls.p, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_tagged) *out_tagged = l.cls_in_code ? 1u : 0u;
    return AIC_OK;
}

int aic_update_light_volume(aic_ctx *c, int layer, const uint8_t *light) {
    if (!c || !valid_layer(layer) || !light) return fail(c, AIC_ERR_INVALID, "aic_update_light_volume: bad argument");
    Layer &l = c->layers[layer];
    if (!l.present) return fail(c, AIC_ERR_INVALID, "aic_update_light_volume: no space uploaded for this layer");
    HIP_TRY(c, hipSetDevice(c->device));
    { const int rc = light_job_finish(c); if (rc != AIC_OK) return rc; }
    // Double-buffered: the new volume goes into the buffer no frame in flight is reading, on its own
    // stream, and becomes current for the frames submitted from now on -- a streaming loop that
    // re-lights every frame (BASELINE config 5) keeps its frames overlapped.
    const size_t n = l.n_cubes();
    int spare = 0;
    { const int rc = take_light_spare(c, l, layer, n, &spare); if (rc != AIC_OK) return rc; }
    if (n) HIP_TRY(c, hipMemcpyAsync(l.light_spare[spare].p, light, n * 4, hipMemcpyHostToDevice, c->upload_stream));
    HIP_TRY(c, hipStreamSynchronize(c->upload_stream));
    std::swap(l.light, l.light_spare[spare]);
    l.version++;
    {
        const uint64_t h = n;
        dump_record(c, DUMP_LIGHT, (uint32_t)layer, {{&h, sizeof(h)}, {light, n * 4}});
    }
    return AIC_OK;
}

namespace {

// Re-packs the voxel and palette pools of a layer on the device, dropping the ranges that replaced blocks left
// behind: the cube grid stays at offset 0, every recursive block's ranges are copied (device to device) to the
// next free offset of fresh pools, and the block table follows. Called with no frame in flight.
int compact_pools(aic_ctx *c, Layer &l) {
    l.version++;
    const size_t n = l.n_cubes();
    uint64_t need_vox = n, need_pal = 0;
    for (size_t i = 0; i < l.host_blocks.size(); i++) { need_vox += l.vox_cap[i]; need_pal += l.pal_cap[i]; }
    DevBuf<uint16_t> np;
    DevBuf<DevPaletteEntry> npal;
    hipError_t e;
    if ((e = np.ensure((size_t)need_vox)) != hipSuccess) return hip_fail(c, "compact pool", e);
    if ((e = npal.ensure((size_t)(need_pal ? need_pal : 1))) != hipSuccess) { np.release(); return hip_fail(c, "compact palette", e); }
    // the new offsets go into copies of the tables: the layer keeps pointing at its old pools until every copy has landed
    std::vector<DevBlock> blocks = l.host_blocks;
    std::vector<uint32_t> vbase = l.vox_base, pbase = l.pal_base;
    uint64_t vo = n, po = 0;
    e = n ? hipMemcpyAsync(np.p, l.pool.p, n * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
    for (size_t i = 0; e == hipSuccess && i < blocks.size(); i++) {
        DevBlock &b = blocks[i];
        if (l.vox_cap[i]) {
            e = hipMemcpyAsync(np.p + vo, l.pool.p + l.vox_base[i], (size_t)l.vox_cap[i] * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->stream);
            if ((b.kind & 255u) != 0u) b.vox_off = (uint32_t)vo;  // a block that is a single voxel at the moment keeps offset 0 (its reservation moves all the same)
            vbase[i] = (uint32_t)vo;
            vo += l.vox_cap[i];
        }
        if (e == hipSuccess && l.pal_cap[i]) {
            e = hipMemcpyAsync(npal.p + po, l.palette.p + l.pal_base[i], (size_t)l.pal_cap[i] * sizeof(DevPaletteEntry), hipMemcpyDeviceToDevice, c->stream);
            if ((b.kind & 255u) != 0u) b.pal_off = (uint32_t)po;
            pbase[i] = (uint32_t)po;
            po += l.pal_cap[i];
        }
    }
    if (e == hipSuccess && !blocks.empty())
        e = hipMemcpyAsync(l.blocks.p, blocks.data(), blocks.size() * sizeof(DevBlock), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        // nothing was committed: put the old block table back on the device (best effort) and drop the new pools
        if (!l.host_blocks.empty()) (void)hipMemcpy(l.blocks.p, l.host_blocks.data(), l.host_blocks.size() * sizeof(DevBlock), hipMemcpyHostToDevice);
        np.release();
        npal.release();
        return hip_fail(c, "compact pools", e);
    }
    l.pool.release();
    l.palette.release();
    l.pool = np;
    l.palette = npal;
    l.pool.n = (size_t)vo;
    l.palette.n = (size_t)po;
    l.host_blocks.swap(blocks);
    l.vox_base.swap(vbase);
    l.pal_base.swap(pbase);
    l.garbage_vox = l.garbage_pal = 0;
    return AIC_OK;
}

// One BlockEvaluation / BlockIndex change (updating.rs:128-145), issued on c->stream without synchronising.
int replace_one(aic_ctx *c, int layer, Layer &l, uint32_t index, const aic_block_desc *desc, const uint16_t *voxels, const float *palette) {
    l.version++;
    if (!desc) return fail(c, AIC_ERR_INVALID, "aic_replace_block: null descriptor");
    if (index > l.host_blocks.size() || index >= 65536) return fail(c, AIC_ERR_INVALID, "aic_replace_block: index out of range");
    const bool exists = index < l.host_blocks.size();
    std::vector<uint16_t> vox;
    std::vector<DevPaletteEntry> pal;
    DevBlock db;
    // convert first (offsets patched below), then decide where the data goes
    int rc = convert_block(c, *desc, voxels, palette, 0u, 0u, &db, &vox, &pal);
    if (rc != AIC_OK) return rc;
    // in place when the block's current ranges can hold the new data (the reference replaces the block in place);
    // otherwise append and leave the old ranges as garbage for compact_pools
    const bool fits = exists && vox.size() <= l.vox_cap[index] && pal.size() <= l.pal_cap[index];
    uint32_t vox_off, pal_off;
    hipError_t e;
    if (fits) {
        // the reserved ranges, not host_blocks[index].vox_off / pal_off: those are 0 after a replacement that had no voxels
        vox_off = l.vox_base[index];
        pal_off = l.pal_base[index];
    } else {
        vox_off = (uint32_t)l.pool.n;
        pal_off = (uint32_t)l.palette.n;
        if ((uint64_t)vox_off + vox.size() > kMaxPoolElems || (uint64_t)pal_off + pal.size() > 0xfffffff0ull)
            return fail(c, AIC_ERR_INVALID, "voxel pool too large");
        if (!vox.empty() && (e = l.pool.ensure(vox_off + vox.size(), true, c->stream)) != hipSuccess) return hip_fail(c, "grow pool", e);
        if (!pal.empty() && (e = l.palette.ensure(pal_off + pal.size(), true, c->stream)) != hipSuccess) return hip_fail(c, "grow palette", e);
        if (exists) { l.garbage_vox += l.vox_cap[index]; l.garbage_pal += l.pal_cap[index]; }
    }
    if (!vox.empty()) {
        db.vox_off = vox_off;
        HIP_TRY(c, hipMemcpy(l.pool.p + vox_off, vox.data(), vox.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    if (!pal.empty()) {
        db.pal_off = pal_off;
        HIP_TRY(c, hipMemcpy(l.palette.p + pal_off, pal.data(), pal.size() * sizeof(DevPaletteEntry), hipMemcpyHostToDevice));
    }
    bool class_changed = false;
    if (!exists) {
        l.host_blocks.push_back(db);
        l.vox_cap.push_back((uint32_t)vox.size());
        l.pal_cap.push_back((uint32_t)pal.size());
        l.vox_base.push_back(vox_off);
        l.pal_base.push_back(pal_off);
        if ((e = l.blocks.ensure(l.host_blocks.size(), true, c->stream)) != hipSuccess) return hip_fail(c, "grow blocks", e);
    } else {
        class_changed = block_class(l.host_blocks[index]) != block_class(db);
        l.host_blocks[index] = db;
        if (!fits) {
            l.vox_cap[index] = (uint32_t)vox.size(); l.pal_cap[index] = (uint32_t)pal.size();
            l.vox_base[index] = vox_off; l.pal_base[index] = pal_off;
        }
    }
    HIP_TRY(c, hipMemcpy(l.blocks.p + index, &db, sizeof(db), hipMemcpyHostToDevice));
    set_class(l.host_cls, index, block_class(db));
    if ((e = l.cls.ensure(l.host_cls.size(), true, c->stream)) != hipSuccess) return hip_fail(c, "grow classes", e);
    HIP_TRY(c, hipMemcpy(l.cls.p + index / 16u, &l.host_cls[index / 16u], sizeof(uint32_t), hipMemcpyHostToDevice));
    if (l.cls_in_code) {
        // the cube grid carries class bits: drop them if the table outgrew 14-bit indices, refresh
        // them if an existing block changed class (cubes already holding this index must follow, and
        // the OPEN tags around them: the retag leaves none, the pass behind it decides them all again)
        if (l.host_blocks.size() > kCubeIndexMask + 1u) {
            launch_tag_cubes(l.pool.p, l.n_cubes(), l.cls.p, 1, 0, c->stream);
            l.cls_in_code = false;
        } else if (class_changed) {
            launch_tag_cubes(l.pool.p, l.n_cubes(), l.cls.p, 1, 1, c->stream);
            launch_open_cubes(l.pool.p, l.size, c->stream);
        }
        HIP_TRY(c, hipGetLastError());
    }
    if (desc->flags & AIC_BLOCK_AIR) {
        if (l.air_index < 0) l.air_index = (int32_t)index;
    } else if (l.air_index == (int32_t)index) {
        l.air_index = -1;
    }
    {
        const bool one = (desc->flags & AIC_BLOCK_ONE) != 0;
        const uint64_t nvox = one ? 0 : (uint64_t)(desc->vsize[0] > 0 ? desc->vsize[0] : 0) * (uint64_t)(desc->vsize[1] > 0 ? desc->vsize[1] : 0) * (uint64_t)(desc->vsize[2] > 0 ? desc->vsize[2] : 0);
        const uint64_t h[2] = {index, nvox};
        dump_record(c, DUMP_BLOCK, (uint32_t)layer, {{h, sizeof(h)}, {desc, sizeof(*desc)}, {voxels, (size_t)nvox * 2}, {palette, (size_t)desc->pal_len * 32}});
    }
    return AIC_OK;
}

}  // namespace

int aic_replace_blocks(aic_ctx *c, int layer, uint32_t n, const uint32_t *indices, const aic_block_desc *descs, const uint16_t *const *voxels,
                       const float *const *palettes) {
    if (!c || !valid_layer(layer) || (n && (!indices || !descs || !voxels || !palettes))) return fail(c, AIC_ERR_INVALID, "aic_replace_blocks: bad argument");
    Layer &l = c->layers[layer];
    if (!l.present) return fail(c, AIC_ERR_INVALID, "aic_replace_block: no space uploaded for this layer");
    HIP_TRY(c, hipSetDevice(c->device));
    { int qrc = quiesce(c); if (qrc != AIC_OK) return qrc; }  // once for the whole batch
    int rc = AIC_OK;
    for (uint32_t k = 0; k < n && rc == AIC_OK; k++) rc = replace_one(c, layer, l, indices[k], &descs[k], voxels[k], palettes[k]);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (rc != AIC_OK) return rc;
    // garbage left by blocks that outgrew their ranges: re-pack once it is worth it (more than a quarter of the pool,
    // and more than 256 KB), instead of growing without bound until the next full upload
    const bool big_vox = l.garbage_vox * 4 > l.pool.n && l.garbage_vox > (1u << 17);
    const bool big_pal = l.garbage_pal * 4 > l.palette.n && l.garbage_pal > (1u << 13);
    if (big_vox || big_pal) return compact_pools(c, l);
    return AIC_OK;
}

int aic_compact(aic_ctx *c, int layer) {
    if (!c || !valid_layer(layer)) return fail(c, AIC_ERR_INVALID, "aic_compact: bad argument");
    Layer &l = c->layers[layer];
    if (!l.present) return AIC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    { int qrc = quiesce(c); if (qrc != AIC_OK) return qrc; }
    return compact_pools(c, l);
}

int aic_replace_block(aic_ctx *c, int layer, uint32_t index, const aic_block_desc *desc, const uint16_t *voxels, const float *palette) {
    if (!desc) return fail(c, AIC_ERR_INVALID, "aic_replace_block: bad argument");
    return aic_replace_blocks(c, layer, 1u, &index, desc, &voxels, &palette);
}

int aic_set_options(aic_ctx *c, int layer, const aic_options *o) {
    if (!c || !valid_layer(layer) || !o) return fail(c, AIC_ERR_INVALID, "aic_set_options: bad argument");
    if (o->fog < 0 || o->fog > 3 || o->transparency < 0 || o->transparency > 2 || o->lighting < 0 || o->lighting > 5 ||
        o->antialiasing < 0 || o->antialiasing > 2 || o->tone_mapping < 0 || o->tone_mapping > 1 || !(o->view_distance > 0.0))
        return fail(c, AIC_ERR_INVALID, "aic_set_options: enum or view_distance out of range");
    c->layers[layer].opt = *o;
    c->layers[layer].opt_set = true;
    dump_record(c, DUMP_OPTIONS, (uint32_t)layer, {{o, sizeof(*o)}});
    return AIC_OK;
}

int aic_set_depth_transform(aic_ctx *c, const double zw[4]) {
    if (!c || !zw) return fail(c, AIC_ERR_INVALID, "aic_set_depth_transform: bad argument");
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(zw[i])) return fail(c, AIC_ERR_INVALID, "aic_set_depth_transform: a component is not finite");
    HIP_TRY(c, hipSetDevice(c->device));
    { const int rc = quiesce(c); if (rc != AIC_OK) return rc; }
    std::memcpy(c->depth_zw, zw, sizeof(c->depth_zw));
    return AIC_OK;
}

uint32_t aic_partition_rows(uint32_t height, const aic_partition *p) {
    if (!p || p->n_parts <= 1 || p->strip_rows == 0) return height;
    if (p->part >= p->n_parts) return 0;
    uint32_t rows = 0;
    const uint32_t n_strips = (height + p->strip_rows - 1) / p->strip_rows;
    for (uint32_t s = p->part; s < n_strips; s += p->n_parts) {
        uint32_t r0 = s * p->strip_rows;
        uint32_t r1 = r0 + p->strip_rows;
        if (r1 > height) r1 = height;
        rows += r1 - r0;
    }
    return rows;
}

int aic_assemble_strips_on(aic_ctx *c, const void *gathered_device, void *out_device, uint32_t width, uint32_t height,
                           uint32_t strip_rows, uint32_t n_parts, void *hip_stream) {
    if (!c || !gathered_device || !out_device || !strip_rows || !n_parts) return fail(c, AIC_ERR_INVALID, "aic_assemble_strips: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t max_rows = 0;
    for (uint32_t p = 0; p < n_parts; p++) {
        aic_partition pp = {strip_rows, n_parts, p, 0};
        uint32_t r = aic_partition_rows(height, &pp);
        if (r > max_rows) max_rows = r;
    }
    launch_assemble_strips((const uint32_t *)gathered_device, (uint32_t *)out_device, width, height, strip_rows, n_parts, max_rows, hip_stream ? (hipStream_t)hip_stream : c->stream);
    HIP_TRY(c, hipGetLastError());
    return AIC_OK;
}

int aic_assemble_strips_async(aic_ctx *c, const void *gathered_device, void *out_device, uint32_t width, uint32_t height,
                              uint32_t strip_rows, uint32_t n_parts) {
    return aic_assemble_strips_on(c, gathered_device, out_device, width, height, strip_rows, n_parts, nullptr);
}

int aic_assemble_strips(aic_ctx *c, const void *gathered_device, void *out_device, uint32_t width, uint32_t height,
                        uint32_t strip_rows, uint32_t n_parts) {
    const int rc = aic_assemble_strips_async(c, gathered_device, out_device, width, height, strip_rows, n_parts);
    if (rc != AIC_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return AIC_OK;
}

int aic_read_aux(aic_ctx *c, aic_pixel_aux *out, uint64_t n_records) {
    if (!c || !out) return fail(c, AIC_ERR_INVALID, "aic_read_aux: bad argument");
    if (n_records > c->aux_records) return fail(c, AIC_ERR_INVALID, "aic_read_aux: more records requested than the last frame produced");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(out, c->aux.p, n_records * sizeof(aic_pixel_aux), hipMemcpyDeviceToHost));
    return AIC_OK;
}

int aic_synchronize(aic_ctx *c) {
    if (!c) return AIC_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 1; i < AIC_MAX_IN_FLIGHT; i++)
        if (c->slots[i].stream) HIP_TRY(c, hipStreamSynchronize(c->slots[i].stream));
    return AIC_OK;
}

void *aic_stream(aic_ctx *c) { return c ? (void *)c->stream : nullptr; }

int aic_wait_event(aic_ctx *c, void *hip_event) {
    if (!c || !hip_event) return fail(c, AIC_ERR_INVALID, "aic_wait_event: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, (hipEvent_t)hip_event, 0));
    for (uint32_t i = 1; i < AIC_MAX_IN_FLIGHT; i++)
        if (c->slots[i].stream) HIP_TRY(c, hipStreamWaitEvent(c->slots[i].stream, (hipEvent_t)hip_event, 0));
    return AIC_OK;
}

int aic_stream_wait_frame(aic_ctx *c, uint32_t slot, void *hip_stream) {
    if (!c || slot >= AIC_MAX_IN_FLIGHT) return fail(c, AIC_ERR_INVALID, "aic_stream_wait_frame: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    aic_ctx::FrameSlot &fs = c->slots[slot];
    if (!fs.busy || !fs.npix) return AIC_OK;  // nothing in flight (or an empty partition: no event was recorded)
    HIP_TRY(c, hipStreamWaitEvent((hipStream_t)hip_stream, fs.ev1, 0));
    return AIC_OK;
}

int aic_probe_raycast(aic_ctx *c, const double origin[3], const double direction[3], int use_bounds, const int32_t lo[3],
                      const int32_t hi[3], int include_exit, uint32_t max_steps, aic_rc_step *out, uint32_t *n_out, int *ended) {
    if (!c || !origin || !direction || !out || !n_out || !ended) return fail(c, AIC_ERR_INVALID, "aic_probe_raycast: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = 6 * sizeof(double) + 8 * sizeof(int) + (size_t)max_steps * 8 * sizeof(double) + 64;
    hipError_t e = c->staging.ensure(bytes);
    if (e != hipSuccess) return hip_fail(c, "alloc staging", e);
    unsigned char *base = c->staging.p;
    double od[6] = {origin[0], origin[1], origin[2], direction[0], direction[1], direction[2]};
    int lohi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (use_bounds && lo && hi) {
        for (int a = 0; a < 3; a++) { lohi[a] = lo[a]; lohi[3 + a] = hi[a]; }
    }
    double *d_od = (double *)base;
    int *d_lohi = (int *)(base + 48);
    uint32_t *d_n = (uint32_t *)(base + 48 + 24);
    int *d_end = (int *)(base + 48 + 28);
    double *d_rec = (double *)(base + 48 + 32);
    HIP_TRY(c, hipMemcpyAsync(d_od, od, sizeof(od), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_lohi, lohi, 24, hipMemcpyHostToDevice, c->stream));
    launch_probe_raycast(d_od, use_bounds, d_lohi, include_exit, max_steps, d_rec, d_n, d_end, c->stream);
    HIP_TRY(c, hipGetLastError());
    std::vector<double> rec((size_t)max_steps * 8);
    uint32_t n = 0;
    int en = 0;
    HIP_TRY(c, hipMemcpyAsync(&n, d_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&en, d_end, 4, hipMemcpyDeviceToHost, c->stream));
    if (max_steps) HIP_TRY(c, hipMemcpyAsync(rec.data(), d_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n && i < max_steps; i++) {
        const double *r = rec.data() + 8 * (size_t)i;
        out[i].cube[0] = (int32_t)r[0]; out[i].cube[1] = (int32_t)r[1]; out[i].cube[2] = (int32_t)r[2];
        out[i].face = (int32_t)r[3];
        out[i].t_distance = r[4];
        out[i].intersection_point[0] = r[5]; out[i].intersection_point[1] = r[6]; out[i].intersection_point[2] = r[7];
    }
    *n_out = n;
    *ended = en;
    return AIC_OK;
}

int aic_probe_powf(aic_ctx *c, const float *x, const float *y, uint32_t n, float *out) {
    if (!c || (n && (!x || !y || !out))) return fail(c, AIC_ERR_INVALID, "aic_probe_powf: bad argument");
    if (!n) return AIC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipError_t e = c->staging.ensure((size_t)n * 12);
    if (e != hipSuccess) return hip_fail(c, "alloc staging", e);
    float *dx = (float *)c->staging.p, *dy = dx + n, *dout = dy + n;
    HIP_TRY(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dy, y, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    launch_probe_powf(dx, dy, dout, n, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return AIC_OK;
}

int aic_probe_expf(aic_ctx *c, const float *x, uint32_t n, float *out) {
    if (!c || (n && (!x || !out))) return fail(c, AIC_ERR_INVALID, "aic_probe_expf: bad argument");
    if (!n) return AIC_OK;
    for (uint32_t i = 0; i < n; i++)  // expf_table has no overflow / underflow handling: keep to its domain
        if (!(std::fabs(x[i]) < 88.0f)) return fail(c, AIC_ERR_INVALID, "aic_probe_expf: x outside (-88, 88)");
    HIP_TRY(c, hipSetDevice(c->device));
    hipError_t e = c->staging.ensure((size_t)n * 8);
    if (e != hipSuccess) return hip_fail(c, "alloc staging", e);
    float *dx = (float *)c->staging.p, *dout = dx + n;
    HIP_TRY(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    launch_probe_expf(dx, dout, n, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return AIC_OK;
}

int aic_probe_bloom(aic_ctx *c, uint32_t width, uint32_t height, const float *colorbuf, float exposure, const aic_options *options, uint8_t *out_rgba8,
                    uint16_t *out_mip0, uint32_t mip0_size[2]) {
    if (!c || !colorbuf || !options || !out_rgba8 || !width || !height) return fail(c, AIC_ERR_INVALID, "aic_probe_bloom: bad argument");
    if (width > 65535u || height > 65535u) return fail(c, AIC_ERR_INVALID, "aic_probe_bloom: frame dimensions above 65535 are not supported");
    if (!(exposure >= 0.f) || !(options->bloom_intensity >= 0.f)) return fail(c, AIC_ERR_INVALID, "aic_probe_bloom: exposure or bloom_intensity is negative or NaN");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->slots[0].busy) return fail(c, AIC_ERR_INVALID, "aic_probe_bloom: a submitted frame still occupies slot 0 (aic_render_wait it first)");
    const BloomGeom geom = bloom_geometry(width, height);
    const size_t npix = (size_t)width * height;
    aic_ctx::SubSlot &sb = c->slots[0].sub[0];
    hipError_t e;
    if ((e = sb.bloom_cb.ensure(npix)) != hipSuccess || (e = sb.bloom_mips.ensure(geom.texels)) != hipSuccess || (e = c->out.ensure(npix)) != hipSuccess)
        return hip_fail(c, "alloc bloom scratch", e);
    HIP_TRY(c, hipMemcpyAsync(sb.bloom_cb.p, colorbuf, npix * 16, hipMemcpyHostToDevice, c->stream));
    BloomParams bp;
    bp.colorbuf = sb.bloom_cb.p;
    bp.mips = sb.bloom_mips.p;
    bp.out = c->out.p;
    bp.exposure = exposure + 0.0f;
    bp.intensity = options->bloom_intensity;
    bp.tone_mapping = options->tone_mapping;
    bp.maximum_intensity = options->maximum_intensity;
    bp.srgb_thr = c->srgb_thr.p;
    launch_bloom(geom, bp, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out_rgba8, c->out.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_mip0) HIP_TRY(c, hipMemcpyAsync(out_mip0, sb.bloom_mips.p, (size_t)geom.mw[0] * geom.mh[0] * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (mip0_size) { mip0_size[0] = geom.mw[0]; mip0_size[1] = geom.mh[0]; }
    return AIC_OK;
}

int aic_probe_light_lut(aic_ctx *c, float out[256]) {
    if (!c || !out) return AIC_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(out, c->lut.p, 256 * sizeof(float), hipMemcpyDeviceToHost));
    return AIC_OK;
}

}  // extern "C"
