// aic_exposure_host.cpp -- aic_sample_luminance: the context's side of the luminance sampler (aic_exposure.hip). It finishes a pending light update, makes
// the layer's `visible` bitmap if the scene has changed since the last one, stages host rays, launches the sampler and waits for it -- all on the context's
// upload stream, which runs beside the frame slots: frames in flight are neither waited for nor touched.
#include <vector>

#include "aic_ctx.h"
#include "aic_exposure.h"

extern "C" int aic_sample_luminance(aic_ctx *c, int layer, uint32_t n, const double *rays, uint32_t max_steps, uint32_t flags, float *out) {
    if (!c || !valid_layer(layer) || (n && (!rays || !out))) return fail(c, AIC_ERR_INVALID, "aic_sample_luminance: bad argument");
    if (flags & ~AIC_RAYS_DEVICE) return fail(c, AIC_ERR_INVALID, "aic_sample_luminance: unknown flag bits (AIC_RAYS_DEVICE is the only one)");
    if (n > (1u << 20)) return fail(c, AIC_ERR_INVALID, "aic_sample_luminance: more than 1 << 20 rays in one call");
    Layer &l = c->layers[layer];
    if (!l.present) return fail(c, AIC_ERR_INVALID, "aic_sample_luminance: no space uploaded for this layer");
    if (!n) return AIC_OK;
    const bool on_device = (flags & AIC_RAYS_DEVICE) != 0;
    if (on_device && (((uintptr_t)rays & 15u) || ((uintptr_t)out & 3u)))
        return fail(c, AIC_ERR_INVALID, "aic_sample_luminance: AIC_RAYS_DEVICE wants rays at a 16-byte boundary and out at a float's");
    HIP_TRY(c, hipSetDevice(c->device));
    // a submitted light update is published first, like every call that needs the scene; every other scene or light write has finished when its call
    // returned, so the sampler is behind all of them on whatever stream it runs
    { const int rc = light_job_finish(c); if (rc != AIC_OK) return rc; }
    hipStream_t stream = c->upload_stream;
    hipError_t e;
    if (l.visible_version != l.version) {
        std::vector<uint32_t> bits;
        { const int rc = light_visible_bits(c, l, stream, &bits); if (rc != AIC_OK) return rc; }
        if ((e = l.visible_bits.ensure(kVisibleBitsWords)) != hipSuccess) return hip_fail(c, "alloc visible bits", e);
        HIP_TRY(c, hipMemcpyAsync(l.visible_bits.p, bits.data(), kVisibleBitsWords * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));  // (`bits` goes out of scope)
        l.visible_version = l.version;
    }
    ExposureParams p;
    p.grid = l.pool.p;
    p.light = l.light.p;
    p.visible = l.visible_bits.p;
    p.lut = c->lut.p;
    p.rays = rays;
    p.out = out;
    for (int a = 0; a < 3; a++) { p.lo[a] = l.lo[a]; p.size[a] = l.size[a]; }
    p.index_mask = l.cls_in_code ? kCubeIndexMask : 0xffffu;
    p.n = n;
    p.max_steps = max_steps;
    p.sky_kind = l.sky_kind;
    for (int o = 0; o < 8; o++)
        for (int k = 0; k < 3; k++) p.sky[o][k] = l.sky[o][k];
    for (int f = 0; f < 7; f++) p.block_sky[f] = l.block_sky[f];
    const size_t ray_bytes = (size_t)n * 48;
    if (!on_device) {
        if ((e = c->exposure_scratch.ensure(ray_bytes + (size_t)n * 4)) != hipSuccess) return hip_fail(c, "alloc exposure scratch", e);
        HIP_TRY(c, hipMemcpyAsync(c->exposure_scratch.p, rays, ray_bytes, hipMemcpyHostToDevice, stream));
        p.rays = (const double *)c->exposure_scratch.p;
        p.out = (float *)(c->exposure_scratch.p + ray_bytes);
    }
    HIP_TRY(c, launch_sample_luminance(p, stream));
    if (!on_device) HIP_TRY(c, hipMemcpyAsync(out, p.out, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    return AIC_OK;
}
