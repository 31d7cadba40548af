// aic_light_rays_host.cpp -- the context's side of aic_light_rays (include/aic_hip.h) and its two host-only companions,
// aic_light_rays_bound and aic_light_rays_wireframe. The call finishes a pending light update, then runs on the context's upload stream, beside the
// frame slots: frames in flight are neither waited for nor touched, and nothing a frame reads or writes is written. Its tables are the context's own --
// the effective tree of the call's maximum_distance and the derived properties of the layer's blocks, each made again only when the distance or the
// layer's version moved -- not the light updater's, whose mirrors and queue the call leaves alone. tools/submit_record/light_rays_record.cpp drives
// every path of this file.
#include <cmath>
#include <cstring>
#include <vector>

#include "aic_ctx.h"
#include "aic_light_host.h"
#include "aic_light_rays.h"

static_assert(sizeof(aic_light_cube_info) == 32 && sizeof(aic_light_ray) == 40 && sizeof(aic_line_vertex) == 28, "the records of aic_light_rays");

namespace {

const char *const kWho = "aic_light_rays";

// Ray::wireframe_points' `ang`: f64::from(step) * (TAU / 8.0), through the host's C library
LightRayAngles light_ray_angles() {
    LightRayAngles a;
    const double tau = 6.283185307179586476925286766559;
    for (int k = 0; k <= 8; k++) {
        const double x = (double)k * (tau / 8.0);
        a.sc[k][0] = std::sin(x);
        a.sc[k][1] = std::cos(x);
    }
    return a;
}

size_t align_up(size_t x) { return (x + 255u) & ~(size_t)255u; }

// memory the walk's workgroups may take for their slots and queues together
constexpr size_t kWalkScratchBudget = (size_t)256 << 20;
constexpr uint32_t kWalkMaxGroups = 1024;

int ensure_tree(aic_ctx *c, int maximum_distance, hipStream_t stream) {
    if (c->light_rays_distance == maximum_distance) return AIC_OK;
    LightRaysTree t;
    light_rays_tree(maximum_distance, &t);
    const size_t nt = t.tree.size();
    const size_t tree_bytes = align_up(nt * sizeof(DevTreePos)), w_bytes = align_up(nt * 36 * sizeof(float)), ent_bytes = align_up(nt * 6 * sizeof(uint2));
    c->light_rays_distance = -1;
    if (const hipError_t e = c->light_rays_tree.ensure(tree_bytes + w_bytes + ent_bytes)) return hip_fail(c, "alloc light rays tree", e);
    HIP_TRY(c, hipMemcpyAsync(c->light_rays_tree.p, t.tree.data(), nt * sizeof(DevTreePos), hipMemcpyHostToDevice, stream));
    HIP_TRY(c, hipMemcpyAsync(c->light_rays_tree.p + tree_bytes, t.child_w.data(), nt * 36 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(c, hipMemcpyAsync(c->light_rays_tree.p + tree_bytes + w_bytes, t.child_ent.data(), nt * 6 * sizeof(uint2), hipMemcpyHostToDevice, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));  // (`t` goes out of scope)
    c->light_rays_n_tree = (uint32_t)nt;
    c->light_rays_bound = t.bound;
    c->light_rays_distance = maximum_distance;
    return AIC_OK;
}

int ensure_derived(aic_ctx *c, int layer, Layer &l, hipStream_t stream) {
    if (c->light_rays_layer == layer && c->light_rays_version == l.version && c->light_rays_derived.p) return AIC_OK;
    std::vector<DevDerived> derived;
    if (const int rc = light_rays_derived(c, l, stream, &derived)) return rc;
    c->light_rays_layer = -1;
    if (const hipError_t e = c->light_rays_derived.ensure(std::max<size_t>(derived.size(), 1) * sizeof(DevDerived))) return hip_fail(c, "alloc light rays derived", e);
    if (!derived.empty()) {
        HIP_TRY(c, hipMemcpyAsync(c->light_rays_derived.p, derived.data(), derived.size() * sizeof(DevDerived), hipMemcpyHostToDevice, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));  // (`derived` goes out of scope)
    }
    c->light_rays_layer = layer;
    c->light_rays_version = l.version;
    return AIC_OK;
}

}  // namespace

extern "C" uint32_t aic_light_rays_bound(int32_t maximum_distance) {
    if (maximum_distance < 0 || maximum_distance > 255) return 0u;
    return light_rays_bound(maximum_distance);
}

extern "C" int aic_light_rays_wireframe(const aic_light_cube_info *info, const aic_light_ray *rays, aic_line_vertex *out, uint32_t *n_lines) {
    if (!info || !out || !n_lines || (info->n_rays && !rays)) return AIC_ERR_INVALID;
    static const LightRayAngles angles = light_ray_angles();
    const uint32_t n = kLightRayBoxLines + kLightRayLines * info->n_rays;
    for (uint32_t j = 0; j < n; j++) light_rays_line(info->cube, rays, angles, j, out + 2 * (size_t)j);
    *n_lines = n;
    return AIC_OK;
}

extern "C" int aic_light_rays(aic_ctx *c, int layer, uint32_t n, const int32_t *cubes, int32_t maximum_distance, uint32_t flags, uint32_t capacity,
                              aic_light_cube_info *infos, aic_light_ray *rays, aic_line_vertex *lines, uint64_t totals[2]) {
    if (!c || !valid_layer(layer) || (n && !cubes)) return reject(c, kWho, "bad argument");
    if (flags & ~AIC_LIGHT_RAYS_DEVICE) return reject(c, kWho, "unknown flag bits (AIC_LIGHT_RAYS_DEVICE is the only one)");
    if (n > AIC_LIGHT_RAYS_MAX_CUBES) return reject(c, kWho, "more than 1 << 16 cubes in one call");
    if (maximum_distance < 0 || maximum_distance > 255) return reject(c, kWho, "maximum_distance is a u8");
    if (!c->layers[layer].present) return reject(c, kWho, "no space uploaded for this layer");
    const bool on_device = (flags & AIC_LIGHT_RAYS_DEVICE) != 0;
    if (on_device && ((((uintptr_t)rays) | ((uintptr_t)lines)) & 3u)) return reject(c, kWho, "AIC_LIGHT_RAYS_DEVICE wants rays and lines at 4-byte boundaries");
    if (totals) totals[0] = totals[1] = 0;
    if (!n) return AIC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // a submitted light update is published first, like every call that needs the scene
    if (const int rc = light_job_finish(c)) return rc;
    Layer &l = c->layers[layer];
    hipStream_t stream = c->upload_stream;
    if (const int rc = ensure_tree(c, maximum_distance, stream)) return rc;
    if (const int rc = ensure_derived(c, layer, l, stream)) return rc;

    const uint32_t n_tree = c->light_rays_n_tree, bound = c->light_rays_bound;
    // the records and lines that can be stored at all: what the batch can produce, and what the caller has room for
    const uint64_t ray_room = std::min<uint64_t>(capacity, (uint64_t)n * bound);
    const uint64_t line_room = (uint64_t)kLightRayBoxLines * n + (uint64_t)kLightRayLines * ray_room;
    const size_t per_group = (size_t)n_tree * (4 * sizeof(float4) + sizeof(uint2));
    const uint32_t groups = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n, kWalkMaxGroups), kWalkScratchBudget / per_group));

    // the scratch, in this order; a device list stages neither its records (unless only lines are wanted) nor its lines
    const bool own_rays = !(on_device && rays), own_lines = lines && !on_device;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align_up(bytes); return o; };
    const size_t o_cubes = take((size_t)n * 12), o_counts = take((size_t)n * 4), o_offsets = take((size_t)n * 4), o_results = take((size_t)n * sizeof(LightRayResult)),
                 o_infos = take((size_t)n * sizeof(aic_light_cube_info)), o_totals = take(32), o_positions = take(std::max<size_t>((size_t)n * bound * 4, 4)),
                 o_rays = take(own_rays ? (size_t)ray_room * sizeof(aic_light_ray) : 0), o_lines = take(own_lines ? (size_t)line_room * 2 * sizeof(aic_line_vertex) : 0),
                 o_slots = take((size_t)groups * n_tree * 4 * sizeof(float4)), o_queue = take((size_t)groups * n_tree * sizeof(uint2));
    if (const hipError_t e = c->light_rays_scratch.ensure(at)) return hip_fail(c, "alloc light rays scratch", e);
    unsigned char *const base = c->light_rays_scratch.p;

    LightRaysParams p;
    std::memset(&p, 0, sizeof(p));
    p.grid = l.pool.p;
    p.index_mask = l.cls_in_code ? kCubeIndexMask : 0xffffu;
    p.light = l.light.p;
    p.derived = (const DevDerived *)c->light_rays_derived.p;
    p.lut = c->lut.p;
    for (int a = 0; a < 3; a++) { p.lo[a] = l.lo[a]; p.size[a] = l.size[a]; }
    for (int f = 0; f < 7; f++) p.block_sky[f] = l.block_sky[f];
    {
        const size_t tree_bytes = align_up((size_t)n_tree * sizeof(DevTreePos)), w_bytes = align_up((size_t)n_tree * 36 * sizeof(float));
        p.tree = (const DevTreePos *)c->light_rays_tree.p;
        p.child_w = (const float *)(c->light_rays_tree.p + tree_bytes);
        p.child_ent = (const uint2 *)(c->light_rays_tree.p + tree_bytes + w_bytes);
    }
    p.n_tree = n_tree;
    p.cubes = (const int32_t *)(base + o_cubes);
    p.n = n;
    p.bound = bound;
    p.capacity = capacity;
    p.results = (LightRayResult *)(base + o_results);
    p.counts = (uint32_t *)(base + o_counts);
    p.offsets = (uint32_t *)(base + o_offsets);
    p.positions = (uint32_t *)(base + o_positions);
    p.infos = (aic_light_cube_info *)(base + o_infos);
    p.totals = (unsigned long long *)(base + o_totals);
    p.slots = (float4 *)(base + o_slots);
    p.queue = (uint2 *)(base + o_queue);
    p.rays = own_rays ? (aic_light_ray *)(base + o_rays) : rays;
    p.lines = own_lines ? (aic_line_vertex *)(base + o_lines) : lines;
    p.angles = light_ray_angles();

    HIP_TRY(c, hipMemcpyAsync(base + o_cubes, cubes, (size_t)n * 12, hipMemcpyHostToDevice, stream));
    HIP_TRY(c, launch_light_rays_walk(p, groups, stream));
    HIP_TRY(c, launch_light_rays_scan(p, stream));
    unsigned long long t[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(t, p.totals, sizeof(t), hipMemcpyDeviceToHost, stream));
    if (infos) HIP_TRY(c, hipMemcpyAsync(infos, p.infos, (size_t)n * sizeof(aic_light_cube_info), hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    if (t[1] > n || t[2] > ray_room || t[0] > (uint64_t)n * bound) return fail(c, AIC_ERR_DEVICE, "aic_light_rays: the scan's totals are out of range");
    p.n_stored = (uint32_t)t[1];
    p.n_stored_rays = (uint32_t)t[2];
    const uint64_t n_lines = (uint64_t)kLightRayBoxLines * p.n_stored + (uint64_t)kLightRayLines * p.n_stored_rays;
    if (rays || lines) {
        HIP_TRY(c, launch_light_rays_emit(p, stream));
        if (rays && !on_device && p.n_stored_rays) HIP_TRY(c, hipMemcpyAsync(rays, p.rays, (size_t)p.n_stored_rays * sizeof(aic_light_ray), hipMemcpyDeviceToHost, stream));
        if (own_lines && n_lines) HIP_TRY(c, hipMemcpyAsync(lines, p.lines, (size_t)n_lines * 2 * sizeof(aic_line_vertex), hipMemcpyDeviceToHost, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));
    }
    if (totals) {
        totals[0] = t[0];
        totals[1] = (uint64_t)kLightRayBoxLines * n + (uint64_t)kLightRayLines * t[0];
    }
    return AIC_OK;
}

extern "C" int aic_light_rays_cursor_lines(aic_ctx *c, int layer, const int32_t *cube, int32_t maximum_distance, const aic_line_vertex *first, uint32_t n_first,
                                           aic_light_cube_info *info, const aic_line_vertex **device_lines, uint32_t *n_lines) {
    const char *const who = "aic_light_rays_cursor_lines";
    if (!c || !valid_layer(layer) || !cube || !device_lines || !n_lines || (n_first && !first)) return reject(c, who, "bad argument");
    if (maximum_distance < 0 || maximum_distance > 255) return reject(c, who, "maximum_distance is a u8");
    if (!c->layers[layer].present) return reject(c, who, "no space uploaded for this layer");
    const uint32_t bound = light_rays_bound(maximum_distance);
    const uint64_t most = (uint64_t)n_first + kLightRayBoxLines + (uint64_t)kLightRayLines * bound;
    if (most > AIC_LINES_MAX) return reject(c, who, "more than AIC_LINES_MAX lines in all");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const hipError_t e = c->light_rays_list.ensure((size_t)most * 2 * sizeof(aic_line_vertex))) return hip_fail(c, "alloc light rays list", e);
    aic_line_vertex *const list = (aic_line_vertex *)c->light_rays_list.p;
    if (n_first) {
        HIP_TRY(c, hipMemcpyAsync(list, first, (size_t)n_first * 2 * sizeof(aic_line_vertex), hipMemcpyHostToDevice, c->upload_stream));
        HIP_TRY(c, hipStreamSynchronize(c->upload_stream));  // (`first` is the caller's again when the call returns, whatever follows)
    }
    aic_light_cube_info own;
    uint64_t totals[2] = {0, 0};
    if (const int rc = aic_light_rays(c, layer, 1, cube, maximum_distance, AIC_LIGHT_RAYS_DEVICE, bound, &own, nullptr, list + 2 * (size_t)n_first, totals)) return rc;
    if (info) *info = own;
    *device_lines = list;
    *n_lines = n_first + (uint32_t)totals[1];
    return AIC_OK;
}
