// aic_cursor_raycast_host.cpp -- aic_cursor_raycast: the context's side of the cursor raycast (aic_cursor_raycast.hip). It finishes a pending light
// update, stages host rays, launches the kernel and waits for it -- all on the context's upload stream, which runs beside the frame slots: frames in
// flight are neither waited for nor touched. What the kernel reads of "selectable" was put into the block table and the palette pool
// by convert_block (aic_abi.cpp) when the scene was written.
#include "aic_ctx.h"
#include "aic_cursor_raycast.h"

static_assert(sizeof(aic_cursor_desc) == 88 && sizeof(aic_cursor_hit) == 144 && sizeof(aic_cursor_hit) % 8 == 0, "aic_cursor_hit: 144 bytes, lists of it 8-byte aligned");

extern "C" int aic_cursor_raycast(aic_ctx *c, int layer, uint32_t n, const double *rays, double maximum_distance, uint32_t flags, aic_cursor_hit *out) {
    if (!c || !valid_layer(layer) || (n && (!rays || !out))) return fail(c, AIC_ERR_INVALID, "aic_cursor_raycast: bad argument");
    if (flags & ~AIC_RAYS_DEVICE) return fail(c, AIC_ERR_INVALID, "aic_cursor_raycast: unknown flag bits (AIC_RAYS_DEVICE is the only one)");
    if (n > (1u << 20)) return fail(c, AIC_ERR_INVALID, "aic_cursor_raycast: more than 1 << 20 rays in one call");
    if (!(maximum_distance >= 0.0)) return fail(c, AIC_ERR_INVALID, "aic_cursor_raycast: maximum_distance is NaN or negative");
    Layer &l = c->layers[layer];
    if (!l.present) return fail(c, AIC_ERR_INVALID, "aic_cursor_raycast: no space uploaded for this layer");
    if (!n) return AIC_OK;
    const bool on_device = (flags & AIC_RAYS_DEVICE) != 0;
    if (on_device && (((uintptr_t)rays & 7u) || ((uintptr_t)out & 7u)))
        return fail(c, AIC_ERR_INVALID, "aic_cursor_raycast: AIC_RAYS_DEVICE wants rays and out at 8-byte boundaries");
    HIP_TRY(c, hipSetDevice(c->device));
    // a submitted light update is published first, like every call that needs the scene; every other scene or light write has finished when its call
    // returned, so the raycast is behind all of them on whatever stream it runs
    { const int rc = light_job_finish(c); if (rc != AIC_OK) return rc; }
    hipStream_t stream = c->upload_stream;
    hipError_t e;
    CursorRaycastParams p;
    p.pool = l.pool.p;
    p.light = l.light.p;
    p.blocks = l.blocks.p;
    p.palette = l.palette.p;
    p.rays = rays;
    p.out = out;
    p.maximum_distance = maximum_distance;
    for (int a = 0; a < 3; a++) { p.lo[a] = l.lo[a]; p.size[a] = l.size[a]; }
    p.index_mask = l.cls_in_code ? kCubeIndexMask : 0xffffu;
    p.n = n;
    for (int f = 0; f < 7; f++) p.block_sky[f] = l.block_sky[f];
    const size_t ray_bytes = (size_t)n * 48, out_bytes = (size_t)n * sizeof(aic_cursor_hit);
    if (!on_device) {
        if ((e = c->cursor_scratch.ensure(ray_bytes + out_bytes)) != hipSuccess) return hip_fail(c, "alloc cursor raycast scratch", e);
        HIP_TRY(c, hipMemcpyAsync(c->cursor_scratch.p, rays, ray_bytes, hipMemcpyHostToDevice, stream));
        p.rays = (const double *)c->cursor_scratch.p;
        p.out = (aic_cursor_hit *)(c->cursor_scratch.p + ray_bytes);  // (48 n: an 8-byte boundary)
    }
    HIP_TRY(c, launch_cursor_raycast(p, stream));
    if (!on_device) HIP_TRY(c, hipMemcpyAsync(out, p.out, out_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    return AIC_OK;
}
