// aic_grid_replace_host.cpp -- the context's side of the scene inputs that come from device memory (aic_grid_replace.hip):
// aic_replace_cube_grid, aic_copy_cube_grid and aic_update_light_volume_device.
//
// aic_replace_cube_grid is a scene mutation and opens like aic_update_cubes (quiesce: no frame in flight, no pending light update); from there it runs on
// the context's stream in this order -- count, the record back, the refusal of an index out of range with nothing written yet, the boxes, the store,
// OPEN over the whole grid (launch_open_cubes, as behind an upload), the light -- and synchronises once more. The light updater's host mirrors are not
// told: the layer's version moves and light_prepare reads the new grid and volume, and the texels the caller wrote are the caller's (report_reread).
#include <cstring>
#include <vector>

#include "aic_ctx.h"
#include "aic_grid_replace.h"
#include "aic_launch.h"
#include "aic_light_host.h"

namespace {

// What the three calls reject of an array the caller says is in device memory; 0: nothing. `what` names it.
int device_array_invalid(aic_ctx *c, const char *who, const void *p, uintptr_t mask, const char *what) {
    if ((uintptr_t)p & mask) return reject(c, who, (std::string(what) + " does not start at a " + std::to_string(mask + 1u) + "-byte boundary").c_str());
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // (the runtime keeps the failed query as its last error)
        return reject(c, who, (std::string(what) + " is not in device memory").c_str());
    }
    if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) return reject(c, who, (std::string(what) + " is not in device memory").c_str());
    if (at.type == hipMemoryTypeDevice && at.device != c->device) return reject(c, who, (std::string(what) + " is on another device than the context").c_str());
    return 0;
}

}  // namespace

extern "C" int aic_replace_cube_grid(aic_ctx *c, int layer, const uint16_t *block_index, const uint8_t *light, uint32_t capacity, int32_t *out_boxes,
                                     aic_block_cubes_info *info) {
    const char *who = "aic_replace_cube_grid";
    if (!c || !info) return reject(c, who, "bad argument");
    std::memset(info, 0, sizeof(*info));
    if (!valid_layer(layer)) return reject(c, who, "a layer that is neither 0 nor 1");
    Layer &l = c->layers[layer];
    if (!l.present) return reject(c, who, "no space uploaded for the layer");
    if (capacity && !out_boxes) return reject(c, who, "no boxes to write to");
    const size_t n = l.n_cubes();
    if (!n) return AIC_OK;
    if (!block_index) return reject(c, who, "no block indices");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = device_array_invalid(c, who, block_index, 15u, "block_index_device")) return rc;
    if (light)
        if (const int rc = device_array_invalid(c, who, light, 3u, "light_device")) return rc;
    if (const int rc = quiesce(c)) return rc;

    hipError_t e = c->grid_replace_scratch.ensure(grid_replace_scratch_bytes(n));
    if (e != hipSuccess) return hip_fail(c, "alloc grid replace scratch", e);
    GridReplaceParams gp = {};
    gp.grid = l.pool.p;
    gp.fresh = block_index;
    gp.n = n;
    gp.sx = (uint32_t)l.size[0];
    gp.sy = (uint32_t)l.size[1];
    gp.sz = (uint32_t)l.size[2];
    gp.index_mask = l.cls_in_code ? kCubeIndexMask : 0xffffu;
    gp.cls = l.cls_in_code ? l.cls.p : nullptr;
    gp.cls_words = (uint32_t)((l.host_blocks.size() + 15u) / 16u);
    for (int a = 0; a < 3; a++) gp.lo[a] = l.lo[a];
    gp.scratch = c->grid_replace_scratch.p;
    for (hipEvent_t &ev : c->grid_replace_ev)
        if (!ev) HIP_TRY(c, hipEventCreate(&ev));
    hipEvent_t ev0 = c->grid_replace_ev[0], ev1 = c->grid_replace_ev[1];
    hipStream_t stream = c->stream;
    GridReplaceRecord rec = {};
    rec.lo[0] = rec.lo[1] = rec.lo[2] = 0xFFFFFFFFu;
    HIP_TRY(c, hipMemcpyAsync(gp.scratch, &rec, sizeof(rec), hipMemcpyHostToDevice, stream));
    HIP_TRY(c, hipEventRecord(ev0, stream));
    if ((e = launch_count_grid_replace(gp, stream)) != hipSuccess) return hip_fail(c, "launch count grid replace", e);
    HIP_TRY(c, hipEventRecord(ev1, stream));
    HIP_TRY(c, hipMemcpyAsync(&rec, gp.scratch, sizeof(rec), hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    // (the reference indexes `blocks[...]` with a bounds check; nothing has been written so far)
    if (rec.max_index >= l.host_blocks.size()) return reject(c, who, "a block index at or above the layer's block count");
    float count_ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&count_ms, ev0, ev1));
    info->kernel_ms = count_ms;
    info->n_cubes = rec.n_cubes;
    info->n_runs = rec.n_runs;
    if (rec.n_cubes)
        for (int a = 0; a < 3; a++) {
            info->bounds[a] = l.lo[a] + (int32_t)rec.lo[a];
            info->bounds[3 + a] = l.lo[a] + (int32_t)rec.hi[a];
        }
    info->merged = rec.n_runs > capacity ? 1u : 0u;
    info->n_written = info->merged ? (capacity ? 1u : 0u) : (uint32_t)rec.n_runs;
    const bool writes_runs = info->n_written && !info->merged;
    if (info->merged && capacity) std::memcpy(out_boxes, info->bounds, sizeof(info->bounds));
    if (writes_runs) {
        if ((e = c->grid_replace_boxes.ensure(6u * (size_t)info->n_written)) != hipSuccess) return hip_fail(c, "alloc grid replace boxes", e);
        gp.boxes = c->grid_replace_boxes.p;
        gp.n_runs = info->n_written;
    }

    l.version++;  // from here on the grid changes: the light updater's mirrors are stale whatever follows
    HIP_TRY(c, hipEventRecord(ev0, stream));  // (the count's time has been read)
    if (writes_runs) {
        if ((e = launch_write_grid_replace(gp, stream)) != hipSuccess) return hip_fail(c, "launch write grid replace", e);
        HIP_TRY(c, hipMemcpyAsync(out_boxes, gp.boxes, 24u * (size_t)info->n_written, hipMemcpyDeviceToHost, stream));
    }
    if (rec.n_cubes) {
        if ((e = launch_store_grid_replace(gp, stream)) != hipSuccess) return hip_fail(c, "launch store grid replace", e);
        if (l.cls_in_code) launch_open_cubes(l.pool.p, l.size, stream);
        HIP_TRY(c, hipGetLastError());
    }
    if (light) HIP_TRY(c, hipMemcpyAsync(l.light.p, light, n * 4u, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(c, hipEventRecord(ev1, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    float rest_ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&rest_ms, ev0, ev1));
    info->kernel_ms += rest_ms;
    if (c->dump) {  // the arrays as the call saw them: header {n cubes, whether light came, capacity}, the indices, the light
        std::vector<uint16_t> bi(n);
        std::vector<uint8_t> lt(light ? n * 4u : 0u);
        HIP_TRY(c, hipMemcpy(bi.data(), block_index, n * 2u, hipMemcpyDeviceToHost));
        if (light) HIP_TRY(c, hipMemcpy(lt.data(), light, n * 4u, hipMemcpyDeviceToHost));
        const struct { uint64_t n; uint32_t has_light, capacity; } h = {(uint64_t)n, light ? 1u : 0u, capacity};
        dump_record(c, DUMP_GRID, (uint32_t)layer, {{&h, sizeof(h)}, {bi.data(), n * 2u}, {light ? lt.data() : nullptr, n * 4u}});
    }
    return AIC_OK;
}

extern "C" int aic_copy_cube_grid(aic_ctx *c, int layer, uint16_t *out, uint8_t *light_out) {
    const char *who = "aic_copy_cube_grid";
    if (!c) return reject(c, who, "bad argument");
    if (!valid_layer(layer)) return reject(c, who, "a layer that is neither 0 nor 1");
    Layer &l = c->layers[layer];
    if (!l.present) return reject(c, who, "no space uploaded for the layer");
    const size_t n = l.n_cubes();
    if (!n || (!out && !light_out)) return AIC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (out)
        if (const int rc = device_array_invalid(c, who, out, 15u, "out_device")) return rc;
    if (light_out)
        if (const int rc = device_array_invalid(c, who, light_out, 3u, "light_out_device")) return rc;
    if (c->slots[0].busy) return reject(c, who, "a submitted frame still occupies slot 0 (aic_render_wait it first)");
    // every scene write has finished when its call returned; the light a submitted update is making is published first
    if (light_out)
        if (const int rc = light_job_finish(c)) return rc;
    hipStream_t stream = c->slots[0].stream;
    if (out) HIP_TRY(c, launch_copy_cube_grid(l.pool.p, n, l.cls_in_code ? kCubeIndexMask : 0xffffu, out, stream));
    if (light_out) HIP_TRY(c, hipMemcpyAsync(light_out, l.light.p, n * 4u, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    return AIC_OK;
}

extern "C" int aic_update_light_volume_device(aic_ctx *c, int layer, const uint8_t *light) {
    const char *who = "aic_update_light_volume_device";
    if (!c || !valid_layer(layer) || !light) return reject(c, who, "bad argument");
    Layer &l = c->layers[layer];
    if (!l.present) return reject(c, who, "no space uploaded for the layer");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = device_array_invalid(c, who, light, 3u, "light_device")) return rc;
    if (const int rc = light_job_finish(c)) return rc;
    // as aic_update_light_volume: into a volume no frame in flight reads, on the upload stream, current for the frames submitted from now on
    const size_t n = l.n_cubes();
    int spare = 0;
    if (const int rc = take_light_spare(c, l, layer, n, &spare)) return rc;
    if (n) HIP_TRY(c, hipMemcpyAsync(l.light_spare[spare].p, light, n * 4u, hipMemcpyDeviceToDevice, c->upload_stream));
    HIP_TRY(c, hipStreamSynchronize(c->upload_stream));
    std::swap(l.light, l.light_spare[spare]);
    l.version++;
    if (c->dump) {  // the same record as aic_update_light_volume's: a replay needs no device array for it
        std::vector<uint8_t> lt(n * 4u);
        if (n) HIP_TRY(c, hipMemcpy(lt.data(), light, n * 4u, hipMemcpyDeviceToHost));
        const uint64_t h = n;
        dump_record(c, DUMP_LIGHT, (uint32_t)layer, {{&h, sizeof(h)}, {lt.data(), n * 4u}});
    }
    return AIC_OK;
}
