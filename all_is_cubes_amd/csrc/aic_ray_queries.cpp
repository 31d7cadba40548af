// aic_ray_queries.cpp -- the two calls that ask the scene something along listed rays, one lane per ray: aic_sample_luminance, the context's side of the
// luminance sampler (aic_exposure.hip), and aic_cursor_raycast, that of the cursor raycast (aic_cursor_raycast.hip).
// Both finish a pending light update, stage host rays, launch their kernel and wait for it -- all on the context's upload stream, which runs beside the
// frame slots: frames in flight are neither waited for nor touched. The checks they open with (`begin`, under the entry point's name: `also` is a refusal
// of the entry point's own, or nullptr, which has its place among them; rays_mask, out_mask and `alignment` are what AIC_RAYS_DEVICE asks of the two lists)
// and the part of the kernarg they share are written once, below. From there on the two run alike -- stage the rays at the scratch's start and the results behind them, launch, copy back, synchronise -- and each
// writes it out: a failed runtime call is reported by its expression, which names the call's own buffer and launcher. What the cursor raycast reads of
// "selectable" was put into the block table and the palette pool by convert_block (aic_abi.cpp) when the scene was written.
// tools/submit_record/listed_ops_record.cpp and cursor_raycast_record.cpp drive every path of this file.
#include <cstring>
#include <vector>

#include "aic_ctx.h"
#include "aic_cursor_raycast.h"
#include "aic_exposure.h"
#include "aic_light_host.h"

static_assert(sizeof(aic_cursor_desc) == 88 && sizeof(aic_cursor_hit) == 144 && sizeof(aic_cursor_hit) % 8 == 0, "aic_cursor_hit: 144 bytes, lists of it 8-byte aligned");

namespace {

// What a ray query opens with. *l stays nullptr when the call is over: refused, failed, or n == 0.
int begin(aic_ctx *c, const char *who, int layer, uint32_t n, const void *rays, const void *out, uint32_t flags, const char *also, uintptr_t rays_mask,
          uintptr_t out_mask, const char *alignment, Layer **l) {
    *l = nullptr;
    if (!c || !valid_layer(layer) || (n && (!rays || !out))) return reject(c, who, "bad argument");
    if (flags & ~AIC_RAYS_DEVICE) return reject(c, who, "unknown flag bits (AIC_RAYS_DEVICE is the only one)");
    if (n > (1u << 20)) return reject(c, who, "more than 1 << 20 rays in one call");
    if (also) return reject(c, who, also);
    if (!c->layers[layer].present) return reject(c, who, "no space uploaded for this layer");
    if (!n) return AIC_OK;
    if ((flags & AIC_RAYS_DEVICE) && (((uintptr_t)rays & rays_mask) || ((uintptr_t)out & out_mask))) return reject(c, who, alignment);
    HIP_TRY(c, hipSetDevice(c->device));
    // a submitted light update is published first, like every call that needs the scene; every other scene or light write has finished when its call
    // returned, so the query is behind all of them on whatever stream it runs
    if (const int rc = light_job_finish(c)) return rc;
    *l = &c->layers[layer];
    return AIC_OK;
}

// what the two flat kernargs (ExposureParams, CursorRaycastParams) share
template <typename Params, typename Out>
void fill_shared(Params &p, const Layer &l, uint32_t n, const double *rays, Out *out) {
    p.rays = rays;
    p.out = out;
    p.light = l.light.p;
    for (int a = 0; a < 3; a++) { p.lo[a] = l.lo[a]; p.size[a] = l.size[a]; }
    p.index_mask = l.cls_in_code ? kCubeIndexMask : 0xffffu;
    p.n = n;
    for (int f = 0; f < 7; f++) p.block_sky[f] = l.block_sky[f];
}

}  // namespace

extern "C" int aic_sample_luminance(aic_ctx *c, int layer, uint32_t n, const double *rays, uint32_t max_steps, uint32_t flags, float *out) {
    Layer *lp;
    const int rc = begin(c, "aic_sample_luminance", layer, n, rays, out, flags, nullptr, 15u, 3u, "AIC_RAYS_DEVICE wants rays at a 16-byte boundary and out at a float's", &lp);
    if (!lp) return rc;
    Layer &l = *lp;  // (by this name: a failed copy of its bitmap is reported by its expression)
    const bool on_device = (flags & AIC_RAYS_DEVICE) != 0;
    hipStream_t stream = c->upload_stream;
    if (l.visible_version != l.version) {
        std::vector<uint32_t> bits;
        if (const int made = light_visible_bits(c, l, stream, &bits)) return made;
        if (const hipError_t e = l.visible_bits.ensure(kVisibleBitsWords)) return hip_fail(c, "alloc visible bits", e);
        HIP_TRY(c, hipMemcpyAsync(l.visible_bits.p, bits.data(), kVisibleBitsWords * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));  // (`bits` goes out of scope)
        l.visible_version = l.version;
    }
    ExposureParams p;
    fill_shared(p, l, n, rays, out);
    p.grid = l.pool.p;
    p.visible = l.visible_bits.p;
    p.lut = c->lut.p;
    p.max_steps = max_steps;
    p.sky_kind = l.sky_kind;
    std::memcpy(p.sky, l.sky, sizeof(p.sky));
    const size_t ray_bytes = (size_t)n * 48;
    if (!on_device) {
        if (const hipError_t e = c->exposure_scratch.ensure(ray_bytes + (size_t)n * 4)) return hip_fail(c, "alloc exposure scratch", e);
        HIP_TRY(c, hipMemcpyAsync(c->exposure_scratch.p, rays, ray_bytes, hipMemcpyHostToDevice, stream));
        p.rays = (const double *)c->exposure_scratch.p;
        p.out = (float *)(c->exposure_scratch.p + ray_bytes);
    }
    HIP_TRY(c, launch_sample_luminance(p, stream));
    if (!on_device) HIP_TRY(c, hipMemcpyAsync(out, p.out, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    return AIC_OK;
}

extern "C" int aic_cursor_raycast(aic_ctx *c, int layer, uint32_t n, const double *rays, double maximum_distance, uint32_t flags, aic_cursor_hit *out) {
    Layer *l;
    const int rc = begin(c, "aic_cursor_raycast", layer, n, rays, out, flags, maximum_distance >= 0.0 ? nullptr : "maximum_distance is NaN or negative", 7u, 7u,
                         "AIC_RAYS_DEVICE wants rays and out at 8-byte boundaries", &l);
    if (!l) return rc;
    const bool on_device = (flags & AIC_RAYS_DEVICE) != 0;
    hipStream_t stream = c->upload_stream;
    CursorRaycastParams p;
    fill_shared(p, *l, n, rays, out);
    p.pool = l->pool.p;
    p.blocks = l->blocks.p;
    p.palette = l->palette.p;
    p.maximum_distance = maximum_distance;
    const size_t ray_bytes = (size_t)n * 48, out_bytes = (size_t)n * sizeof(aic_cursor_hit);
    if (!on_device) {
        if (const hipError_t e = c->cursor_scratch.ensure(ray_bytes + out_bytes)) return hip_fail(c, "alloc cursor raycast scratch", e);
        HIP_TRY(c, hipMemcpyAsync(c->cursor_scratch.p, rays, ray_bytes, hipMemcpyHostToDevice, stream));
        p.rays = (const double *)c->cursor_scratch.p;
        p.out = (aic_cursor_hit *)(c->cursor_scratch.p + ray_bytes);  // (48 n: an 8-byte boundary)
    }
    HIP_TRY(c, launch_cursor_raycast(p, stream));
    if (!on_device) HIP_TRY(c, hipMemcpyAsync(out, p.out, out_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    return AIC_OK;
}
