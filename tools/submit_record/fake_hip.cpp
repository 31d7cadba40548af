// fake_hip.cpp -- a recording stand-in for the HIP runtime calls and kernel launchers the host side of the C ABI (aic_abi.cpp, aic_frame.cpp,
// aic_split_ops.cpp, aic_ray_queries.cpp) uses.
// Nothing of the real runtime is loaded: device memory is host memory, streams and events are ordinals, a launch is a line of text. Every call is logged
// with its sizes; streams and events by creation ordinal, every device pointer as allocation ordinal + offset, so that two builds of the host code driven
// through the same scenarios (driver.cpp, split_ops_record.cpp, listed_ops_record.cpp) give byte-identical records exactly when they make the same calls in the same order.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "aic_bloom.h"
#include "aic_cursor_raycast.h"
#include "aic_device.h"
#include "aic_exposure.h"
#include "aic_launch.h"
#include "aic_light_host.h"
#include "aic_light_rays.h"
#include "aic_pick.h"
#include "aic_present_lines.h"
#include "aic_reproject.h"
#include "aic_stale.h"
#include "aic_stale_blocks.h"
#include "aic_stale_cubes.h"
#include "record.h"

namespace {

struct Alloc { size_t size; int ordinal; };
std::map<const char *, Alloc> g_allocs;  // by base address
std::map<const void *, int> g_handles;   // streams and events
std::map<std::string, int> g_calls, g_fail_at;
int g_next_alloc = 0, g_next_stream = 0, g_next_event = 0;
bool g_bail = false;

std::string handle(const void *h, char kind) {
    if (!h) return std::string(1, kind) + "-";
    auto it = g_handles.find(h);
    return std::string(1, kind) + (it == g_handles.end() ? "?" : std::to_string(it->second));
}
#define P(x) rec_ptr(x).c_str()
#define S(x) handle(x, 'S').c_str()
#define E(x) handle(x, 'E').c_str()

// counts the call; true when it is the one fake_fail asked to fail
bool failing(const char *fn) {
    const int n = g_calls[fn]++;
    auto it = g_fail_at.find(fn);
    if (it == g_fail_at.end() || it->second != n) return false;
    g_fail_at.erase(it);
    rec("%s FAILS", fn);
    return true;
}
#define FAKE(fn, ...)                                      \
    do {                                                   \
        rec(__VA_ARGS__);                                  \
        if (failing(fn)) return std::strcmp(fn, "hipMalloc") ? hipErrorInvalidValue : hipErrorOutOfMemory; \
    } while (0)

void rec_words(const char *name, const void *p, size_t n_words) {  // floats and ints alike, as 32-bit words
    std::string s = name;
    for (size_t i = 0; i < n_words; i++) { char b[16]; std::snprintf(b, sizeof(b), " %08x", ((const uint32_t *)p)[i]); s += b; }
    rec("%s", s.c_str());
}

void rec_layer(const aic::DevLayer &l) {
    rec("  layer pool %s cls %s light %s blocks %s palette %s n_blocks %u present %d air %d sky_kind %d cls_in_code %u", P(l.pool), P(l.cls), P(l.light), P(l.blocks),
        P(l.palette), l.n_blocks, l.present, l.air_index, l.sky_kind, l.cls_in_code);
    rec_words("  layer lo size", l.lo, 6);
    rec_words("  layer sky", l.sky, 24);
    rec_words("  layer block_sky", l.block_sky, 7);
    rec("  layer opt fog %d transparency %d threshold %a lighting %d antialiasing %d debug_pixel_cost %d tone_mapping %d maximum_intensity %a bounce_samples %d pad %d view_distance %a exposure %a",
        l.opt.fog, l.opt.transparency, l.opt.threshold, l.opt.lighting, l.opt.antialiasing, l.opt.debug_pixel_cost, l.opt.tone_mapping, l.opt.maximum_intensity,
        l.opt.bounce_samples, l.opt.pad_, l.opt.view_distance, l.exposure);
    rec_words("  layer inv", l.inv, 32);
}

void rec_frame(const aic::DevFrame &F) {
    rec_layer(F.layer);
    rec("  transparency %d lighting %d size %ux%u antialias %d maximum_intensity %a tone_mapping %d strip_rows %u n_parts %u part %u local_rows %u", F.layer_transparency,
        F.layer_lighting, F.width, F.height, F.antialias, F.maximum_intensity, F.tone_mapping, F.strip_rows, F.n_parts, F.part, F.local_rows);
    rec("  tiles %ux%u tile %u macro %u macros %ux%u n_cus %u tiles_per_wave %u pass %d hit_layer %u use_init %d pixel_centers %d out_mode %d", F.tiles_x, F.tiles_y, F.tile,
        F.macro, F.macros_x, F.macros_y, F.n_cus, F.tiles_per_wave, F.pass, F.hit_layer, F.use_init, F.pixel_centers, F.out_mode);
    rec("  ortho %s ortho_n %d patches %s n_patches %u bare_trace %d rays %s aux %s n_queues %u n_sub %u", P(F.ortho), F.ortho_n, P(F.patches), F.n_patches, F.bare_trace, P(F.rays),
        P(F.aux), F.n_queues, F.n_sub);
    rec("  light_lut %s srgb_buckets %s edge_x %s edge_y %s ray_cold %s ray_cold_groups %u ray_mode %u exchange %u", P(F.light_lut), P(F.srgb_buckets), P(F.edge_x), P(F.edge_y),
        P(F.ray_cold), F.ray_cold_groups, F.ray_mode, F.exchange);
    rec_words("  depth_zw", F.depth_zw, 8);
    static const aic::DevSub none = {};
    for (uint32_t j = 0; j < aic::kMaxSub; j++) {
        const aic::DevSub &s = F.sub[j];
        if (j >= F.n_sub && !std::memcmp(&s, &none, sizeof(s)) && !F.split_depth[j] && F.split_ui_exposure[j] == 0.f) continue;  // (an unused sub-frame left at zero)
        rec("  sub %u exposure %a has_backdrop %d out %s acc %s counters %s host_counters %s tile_order %s tile_cost %s queue_start %s split_depth %s ui_exposure %a", j, s.exposure,
            s.has_backdrop, P(s.out), P(s.acc_buf), P(s.counters), P(s.host_counters), P(s.tile_order), P(s.tile_cost), P(s.queue_start), P(F.split_depth[j]), F.split_ui_exposure[j]);
        rec_words("  sub inv", s.inv, 32);
        rec_words("  sub backdrop", s.backdrop, 4);
    }
}

void rec_bloom_geom(const aic::BloomGeom &g) {
    rec("  geom %ux%u levels %u texels %u", g.width, g.height, g.levels, g.texels);
    rec_words("  geom mw", g.mw, aic::kBloomMaxLevels);
    rec_words("  geom mh", g.mh, aic::kBloomMaxLevels);
    rec_words("  geom off", g.off, aic::kBloomMaxLevels);
}
void rec_present(const aic::BloomGeom &g, const aic::PresentParams &p, hipStream_t stream) {
    rec_bloom_geom(g);
    rec("  src %s %ux%u scene %s mips %s out %s intensity %a tone_mapping %d maximum_intensity %a srgb_thr %s out_f16 %d %s", P(p.src), p.src_width, p.src_height, P(p.scene), P(p.mips),
        P(p.out), p.intensity, p.tone_mapping, p.maximum_intensity, P(p.srgb_thr), (int)p.out_f16, S(stream));
    const aic::PresentText &t = p.text;
    if (t.codes)  // (a presentation without text records what it did before there was any)
        rec("  text codes %s atlas %s scale %a %a origin %a %a grid %ux%u cell %ux%u margin %u reach %u %u %u %u", P(t.codes), P(t.atlas), t.scale[0], t.scale[1], t.origin[0],
            t.origin[1], t.cols, t.rows, t.cell_w, t.cell_h, t.margin, t.x0, t.y0, t.x1, t.y1);
}

}  // namespace

void rec(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::putchar('\n');
}
std::string rec_ptr(const void *p) {
    if (!p) return "null";
    auto it = g_allocs.upper_bound((const char *)p);
    if (it != g_allocs.begin()) {
        --it;
        const size_t off = (size_t)((const char *)p - it->first);
        if (off < it->second.size) return "A" + std::to_string(it->second.ordinal) + "+" + std::to_string(off);
    }
    return "host";
}
void fake_reset() {
    if (!g_allocs.empty() || !g_handles.empty()) rec("LEAK %zu allocations, %zu streams and events", g_allocs.size(), g_handles.size());
    g_next_alloc = g_next_stream = g_next_event = 0;
    g_calls.clear();
    g_fail_at.clear();
    g_bail = false;
}
void fake_fail(const char *fn, int nth) { g_fail_at[fn] = g_calls[fn] + nth; }
int fake_calls(const char *fn) { return g_calls[fn]; }
void fake_bail(bool on) { g_bail = on; }

// ---- the runtime
extern "C" {

hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return failing("hipSetDevice") ? hipErrorInvalidValue : hipSuccess; }  // (every entry point begins with it: logged only where it is made to fail)
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) {
    std::memset(p, 0, sizeof(*p));
    p->multiProcessorCount = 256;
    std::snprintf(p->name, sizeof(p->name), "fake");
    std::snprintf(p->gcnArchName, sizeof(p->gcnArchName), "gfx950");
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return failing("hipGetLastError") ? hipErrorInvalidValue : hipSuccess; }  // (the same)
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "invalid value"; }

hipError_t hipMalloc(void **p, size_t bytes) {
    FAKE("hipMalloc", "hipMalloc %zu -> A%d", bytes, g_next_alloc);
    *p = std::calloc(1, bytes);
    g_allocs[(const char *)*p] = Alloc{bytes, g_next_alloc++};
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    rec("hipFree %s", P(p));
    g_allocs.erase((const char *)p);
    std::free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int flags) {
    FAKE("hipHostMalloc", "hipHostMalloc %zu flags %u", bytes, flags);
    *p = std::calloc(1, bytes);
    return hipSuccess;
}
hipError_t hipHostFree(void *p) { rec("hipHostFree"); std::free(p); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    FAKE("hipMemcpyAsync", "hipMemcpyAsync %s <- %s bytes %zu kind %d %s", P(dst), P(src), bytes, (int)kind, S(s));
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    FAKE("hipMemcpy", "hipMemcpy %s <- %s bytes %zu kind %d", P(dst), P(src), bytes, (int)kind);
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t s) {
    FAKE("hipMemsetAsync", "hipMemsetAsync %s value %d bytes %zu %s", P(dst), value, bytes, S(s));
    std::memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags) {
    FAKE("hipStreamCreateWithFlags", "hipStreamCreateWithFlags %u -> S%d", flags, g_next_stream);
    *s = (hipStream_t) new char;
    g_handles[*s] = g_next_stream++;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { rec("hipStreamDestroy %s", S(s)); g_handles.erase(s); delete (char *)s; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { FAKE("hipStreamSynchronize", "hipStreamSynchronize %s", S(s)); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int flags) { FAKE("hipStreamWaitEvent", "hipStreamWaitEvent %s %s %u", S(s), E(e), flags); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int flags) {
    FAKE("hipEventCreate", "hipEventCreate flags %u -> E%d", flags, g_next_event);
    *e = (hipEvent_t) new char;
    g_handles[*e] = g_next_event++;
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { rec("hipEventDestroy %s", E(e)); g_handles.erase(e); delete (char *)e; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { FAKE("hipEventRecord", "hipEventRecord %s %s", E(e), S(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { FAKE("hipEventSynchronize", "hipEventSynchronize %s", E(e)); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) { FAKE("hipEventElapsedTime", "hipEventElapsedTime %s %s", E(a), E(b)); *ms = 1.0f; return hipSuccess; }

}  // extern "C"

// ---- the kernel launchers and the light updater's hooks
struct aic_ctx;
int (*fake_light_job_finish)(aic_ctx *) = nullptr;  // (record.h: a program that wants to see the call sets it; nobody else's record changes)
namespace aic {

void light_state_free(LightState *) {}
void light_state_cubes_updated(LightState *, uint64_t, uint64_t, uint32_t, const int32_t *, const uint16_t *, const uint8_t *) {}
int light_job_finish(aic_ctx *c) { return fake_light_job_finish ? fake_light_job_finish(c) : 0; }
// (the luminance sampler's bitmap, kVisibleBitsWords words: a fixed pattern; can be made to fail like a runtime call)
int light_visible_bits(aic_ctx *, Layer &, hipStream_t stream, std::vector<uint32_t> *bits) {
    rec("light_visible_bits %s", S(stream));
    if (failing("light_visible_bits")) return AIC_ERR_DEVICE;
    bits->assign(2048, 0xa5a5a5a5u);
    return AIC_OK;
}

size_t trace_ray_cold_bytes(uint32_t n_cus, uint32_t *groups) {  // (a pure question, not a launch: not logged. The numbers are arbitrary, not the library's: any non-zero size serves)
    *groups = n_cus * 4u;
    return (size_t)*groups * 320u * 16u;
}
void launch_trace_image(const DevFrame &F, bool diag, hipStream_t stream) {
    rec("launch_trace_image diag %d %s", (int)diag, S(stream));
    rec_frame(F);
    if (g_bail && F.sub[0].host_counters) F.sub[0].host_counters[5] = 1;  // DevCounters::bailed
}
void launch_order_tiles(const uint32_t *cost, uint32_t *order, uint32_t n_tiles, uint32_t macros_x, uint32_t sb_shift, uint32_t n_queues, uint32_t *queue_start, hipStream_t stream,
                        bool clear_cost, uint32_t *clear_words, uint32_t n_clear_words) {
    rec("launch_order_tiles cost %s order %s n_tiles %u macros_x %u sb_shift %u n_queues %u queue_start %s %s clear_cost %d clear_words %s %u", P(cost), P(order), n_tiles, macros_x,
        sb_shift, n_queues, P(queue_start), S(stream), (int)clear_cost, P(clear_words), n_clear_words);
}
void launch_order_tiles_jobs(const OrderJobs &jobs, uint32_t n_jobs, uint32_t n_tiles, uint32_t macros_x, uint32_t sb_shift, uint32_t n_queues, hipStream_t stream, bool clear_cost,
                             uint32_t n_clear_words) {
    rec("launch_order_tiles_jobs n_jobs %u n_tiles %u macros_x %u sb_shift %u n_queues %u %s clear_cost %d n_clear_words %u", n_jobs, n_tiles, macros_x, sb_shift, n_queues, S(stream),
        (int)clear_cost, n_clear_words);
    for (uint32_t j = 0; j < kMaxSub; j++)
        if (j < n_jobs || jobs.cost[j] || jobs.order[j] || jobs.queue_start[j] || jobs.clear_words[j])
            rec("  job %u cost %s order %s queue_start %s clear_words %s", j, P(jobs.cost[j]), P(jobs.order[j]), P(jobs.queue_start[j]), P(jobs.clear_words[j]));
}
void launch_bloom(const BloomGeom &g, const BloomParams &p, hipStream_t stream) {
    rec("launch_bloom %ux%u levels %u texels %u colorbuf %s mips %s out %s exposure %a intensity %a tone_mapping %d maximum_intensity %a srgb_thr %s %s", g.width, g.height, g.levels,
        g.texels, P(p.colorbuf), P(p.mips), P(p.out), p.exposure, p.intensity, p.tone_mapping, p.maximum_intensity, P(p.srgb_thr), S(stream));
}
void launch_tag_cubes(uint16_t *grid, size_t n, const uint32_t *cls, int from_tagged, int to_tagged, hipStream_t stream) {
    rec("launch_tag_cubes %s n %zu cls %s %d %d %s", P(grid), n, P(cls), from_tagged, to_tagged, S(stream));
}
void launch_open_cubes(uint16_t *grid, const int size[3], hipStream_t stream) { rec("launch_open_cubes %s size %d %d %d %s", P(grid), size[0], size[1], size[2], S(stream)); }
// (what the scenarios never reach: scene updates, strip assembly, the probes)
void launch_scatter_cubes(uint16_t *, uint32_t *, const int32_t *, const uint16_t *, const uint32_t *, uint32_t, const int[3], const int[3], const uint32_t *, hipStream_t) { rec("launch_scatter_cubes"); }
void launch_open_changed_cubes(uint16_t *, const int32_t *, uint32_t, const int[3], const int[3], hipStream_t) { rec("launch_open_changed_cubes"); }
// (the operations on a resident Split frame. The first line is the launcher's name alone, its arguments follow indented; each can be made to fail like a runtime call)
hipError_t launch_reproject(const ReprojectGeom &g, const ReprojectParams &p, hipStream_t stream) {
    rec("launch_reproject");
    rec("  geom %ux%u levels %u texels %zu", g.width, g.height, g.levels, g.texels);
    rec_words("  geom mw", g.mw, kReprojectMaxLevels);
    rec_words("  geom mh", g.mh, kReprojectMaxLevels);
    std::string off = "  geom off";
    for (size_t o : g.off) off += " " + std::to_string(o);
    rec("%s", off.c_str());
    rec("  src_color %s src_depth %s dst_color %s dst_depth %s scratch %s keep_splats %u %s", P(p.src_color), P(p.src_depth), P(p.dst_color), P(p.dst_depth), P(p.scratch), p.keep_splats,
        S(stream));
    rec_words("  m", p.m, 16);
    rec_words("  ipzw", p.ipzw, 4);
    return failing("launch_reproject") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_pick(const PickParams &p, hipStream_t stream) {
    rec("launch_pick");
    rec("  R %s order %s out %s scratch %s count %u n %u max_unknown %u skip_unknown %llu cursor %llu %s", P(p.R), P(p.order), P(p.out), P(p.scratch), p.count, p.n, p.max_unknown,
        p.skip_unknown, p.cursor, S(stream));
    return failing("launch_pick") ? hipErrorInvalidValue : hipSuccess;
}
void launch_present(const BloomGeom &g, const PresentParams &p, hipStream_t stream) { rec("launch_present"); rec_present(g, p, stream); }
void launch_present_scene(const BloomGeom &g, const PresentParams &p, hipStream_t stream) { rec("launch_present_scene"); rec_present(g, p, stream); }
hipError_t launch_present_lines(const LinesParams &p, hipStream_t stream) {
    rec("launch_present_lines vertices %s n_lines %u keys %s scene %s counts %s clear_keys %d reset_keys %d", P(p.vertices), p.n_lines, P(p.keys), P(p.scene), P(p.counts),
        (int)p.clear_keys, (int)p.reset_keys);
    rec("  depth %s src %ux%u out %ux%u %s", P(p.depth), p.src_width, p.src_height, p.width, p.height, S(stream));
    rec_words("  m", p.m, 16);
    return failing("launch_present_lines") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_export(const ExportParams &p, hipStream_t stream) {
    rec("launch_export src %s %ux%u out %ux%u color %s depth %s srgb_thr %s counts %s %s", P(p.src), p.src_width, p.src_height, p.out_width, p.out_height, P(p.color), P(p.depth),
        P(p.srgb_thr), P(p.counts), S(stream));
    rec_words("  ipzw", p.ipzw, 4);
    return failing("launch_export") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_cursor_raycast(const CursorRaycastParams &p, hipStream_t stream) {
    rec("launch_cursor_raycast groups %u n %u rays %s out %s maximum_distance %a index_mask %u %s", cursor_raycast_groups(p.n), p.n, P(p.rays), P(p.out), p.maximum_distance, p.index_mask,
        S(stream));
    rec("  pool %s light %s blocks %s palette %s", P(p.pool), P(p.light), P(p.blocks), P(p.palette));
    rec_words("  lo size", p.lo, 6);
    rec_words("  block_sky", p.block_sky, 7);
    return failing("launch_cursor_raycast") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_sample_luminance(const ExposureParams &p, hipStream_t stream) {
    rec("launch_sample_luminance");
    rec("  grid %s light %s visible %s lut %s rays %s out %s index_mask %u n %u max_steps %u sky_kind %d %s", P(p.grid), P(p.light), P(p.visible), P(p.lut), P(p.rays), P(p.out), p.index_mask,
        p.n, p.max_steps, p.sky_kind, S(stream));
    rec_words("  lo size", p.lo, 6);
    std::string sky = "  sky";
    for (int o = 0; o < 8; o++)
        for (int k = 0; k < 3; k++) { char b[32]; std::snprintf(b, sizeof(b), " %a", p.sky[o][k]); sky += b; }
    rec("%s", sky.c_str());
    rec_words("  block_sky", p.block_sky, 7);
    return failing("launch_sample_luminance") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_pick_stale(const StaleParams &p, hipStream_t stream) {
    rec("launch_pick_stale");
    rec("  color %s depth %s order %s out %s scratch %s rects %s width %u count %u n %u max_stale %u n_rects %u depth_test %u skip_stale %llu cursor %llu %s", P(p.color), P(p.depth),
        P(p.order), P(p.out), P(p.scratch), P(p.rects), p.width, p.count, p.n, p.max_stale, p.n_rects, p.depth_test, p.skip_stale, p.cursor, S(stream));
    for (uint32_t i = 0; i < p.n_rects; i++) rec("  rect %u x0y0 %08x x1y1 %08x dmin %a reserved %u", i, p.rects[i].x0y0, p.rects[i].x1y1, p.rects[i].dmin, p.rects[i].reserved);
    return failing("launch_pick_stale") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_pick_stale_cubes(const StaleCubesParams &p, hipStream_t stream) {
    rec("launch_pick_stale_cubes");
    rec("  color %s depth %s order %s out %s scratch %s boxes %s light_cubes %s rects %s %ux%u n %u max_stale %u n_boxes %u n_light_cubes %u expand %d front %u behind %u skip_stale %llu cursor %llu %s",
        P(p.color), P(p.depth), P(p.order), P(p.out), P(p.scratch), P(p.boxes), P(p.light_cubes), P(p.rects), p.width, p.height, p.n, p.max_stale, p.n_boxes, p.n_light_cubes, p.expand,
        p.depth_front, p.depth_behind, p.skip_stale, p.cursor, S(stream));
    return failing("launch_pick_stale_cubes") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_project_stale_cubes(const StaleCubesParams &p, hipStream_t stream) {
    rec("launch_project_stale_cubes scratch %s boxes %s light_cubes %s rects %s %ux%u n_boxes %u n_light_cubes %u expand %d %s", P(p.scratch), P(p.boxes), P(p.light_cubes), P(p.rects), p.width,
        p.height, p.n_boxes, p.n_light_cubes, p.expand, S(stream));
    return failing("launch_project_stale_cubes") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_count_block_cubes(const BlockCubesParams &p, hipStream_t stream) {
    rec("launch_count_block_cubes grid %s n %llu size %u %u %u lo %d %d %d index_mask %04x set_words %u scratch %s %s", P(p.grid), p.n, p.sx, p.sy, p.sz, p.lo[0], p.lo[1], p.lo[2], p.index_mask,
        p.set_words, P(p.scratch), S(stream));
    return failing("launch_count_block_cubes") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t launch_write_block_cubes(const BlockCubesParams &p, hipStream_t stream) {
    rec("launch_write_block_cubes grid %s n %llu scratch %s boxes %s n_runs %u %s", P(p.grid), p.n, P(p.scratch), P(p.boxes), p.n_runs, S(stream));
    return failing("launch_write_block_cubes") ? hipErrorInvalidValue : hipSuccess;
}
// (the light-ray records, aic_light_rays_host.cpp. The tree is a stand-in of ten positions with a bound of three; the scan answers two records a cube
// and stores the cubes the capacity holds; the emitters write every byte they may, so that the sanitizer sees a buffer that is too small)
void light_rays_tree(int maximum_distance, LightRaysTree *out) {
    rec("light_rays_tree %d", maximum_distance);
    out->tree.assign(10, DevTreePos{});
    out->child_w.assign(10 * 36, 0.f);
    out->child_ent.assign(10 * 6, make_uint2(0u, 0u));
    out->bound = 3;
}
uint32_t light_rays_bound(int) { return 3; }
int light_rays_derived(aic_ctx *, Layer &, hipStream_t stream, std::vector<DevDerived> *out) {
    rec("light_rays_derived %s", S(stream));
    if (failing("light_rays_derived")) return AIC_ERR_DEVICE;
    out->assign(4, DevDerived{});
    return AIC_OK;
}
hipError_t launch_light_rays_walk(const LightRaysParams &p, uint32_t workgroups, hipStream_t stream) {
    rec("launch_light_rays_walk groups %u n %u n_tree %u bound %u capacity %u cubes %s results %s counts %s positions %s slots %s queue %s %s", workgroups, p.n, p.n_tree, p.bound,
        p.capacity, P(p.cubes), P(p.results), P(p.counts), P(p.positions), P(p.slots), P(p.queue), S(stream));
    rec("  grid %s light %s derived %s lut %s tree %s child_w %s child_ent %s index_mask %u", P(p.grid), P(p.light), P(p.derived), P(p.lut), P(p.tree), P(p.child_w), P(p.child_ent),
        p.index_mask);
    rec_words("  lo size", p.lo, 6);
    rec_words("  block_sky", p.block_sky, 7);
    if (failing("launch_light_rays_walk")) return hipErrorInvalidValue;
    std::memset(p.positions, 0x33, (size_t)p.n * p.bound * 4);
    std::memset(p.slots, 0x44, (size_t)workgroups * p.n_tree * 64);
    std::memset(p.queue, 0x55, (size_t)workgroups * p.n_tree * 8);
    return hipSuccess;
}
hipError_t launch_light_rays_scan(const LightRaysParams &p, hipStream_t stream) {
    rec("launch_light_rays_scan n %u capacity %u counts %s offsets %s infos %s totals %s %s", p.n, p.capacity, P(p.counts), P(p.offsets), P(p.infos), P(p.totals), S(stream));
    if (failing("launch_light_rays_scan")) return hipErrorInvalidValue;
    uint32_t stored = 0;
    for (uint32_t i = 0; i < p.n; i++) {
        p.counts[i] = 2; p.offsets[i] = 2 * i;
        aic_light_cube_info info = {};
        for (int a = 0; a < 3; a++) info.cube[a] = p.cubes[3 * i + a];
        info.n_rays = 2; info.first_ray = 2 * i;
        if ((uint64_t)2 * i + 2 <= p.capacity) { info.flags = AIC_LIGHT_CUBE_STORED; stored++; }
        p.infos[i] = info;
    }
    p.totals[0] = 2ull * p.n; p.totals[1] = stored; p.totals[2] = 2ull * stored; p.totals[3] = 0;
    return hipSuccess;
}
hipError_t launch_light_rays_emit(const LightRaysParams &p, hipStream_t stream) {
    rec("launch_light_rays_emit n_stored %u n_stored_rays %u rays %s lines %s %s", p.n_stored, p.n_stored_rays, P(p.rays), P(p.lines), S(stream));
    if (failing("launch_light_rays_emit")) return hipErrorInvalidValue;
    std::memset((void *)p.rays, 0x11, (size_t)p.n_stored_rays * sizeof(aic_light_ray));
    if (p.lines) std::memset((void *)p.lines, 0x22, ((size_t)12 * p.n_stored + (size_t)29 * p.n_stored_rays) * 2 * sizeof(aic_line_vertex));
    return hipSuccess;
}
void launch_probe_powf(const float *, const float *, float *, uint32_t, hipStream_t) { rec("launch_probe_powf"); }
void launch_probe_expf(const float *, float *, uint32_t, hipStream_t) { rec("launch_probe_expf"); }
void launch_assemble_strips(const uint32_t *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t) { rec("launch_assemble_strips"); }
void launch_probe_raycast(const double *, int, const int *, int, uint32_t, double *, uint32_t *, int *, hipStream_t) { rec("launch_probe_raycast"); }

}  // namespace aic
