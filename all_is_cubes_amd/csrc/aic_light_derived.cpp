// aic_light_derived.cpp -- compute_derived on the flattened blocks as the device holds them, for the light updater (aic_light_host.cpp), the luminance
// sampler's bitmap (aic_ray_queries.cpp) and the light-ray records (aic_light_rays_host.cpp); declared in aic_light_host.h. Cold: once per scene
// version. Follows
//   all-is-cubes/src/block/eval/derived.rs:78-240     compute_derived (face colours, opacity, visibility)

#include <cmath>
#include <cstring>
#include <vector>

#include "aic_light_host.h"

using namespace aic;

namespace {

// ------------------------------------------------------------------------------------
// restricted_number.rs / color.rs / raytracer_components.rs arithmetic used by compute_derived

inline float h_ps_new_clamped(float v) { return v > 0.f ? v : 0.f; }
inline float h_zo_new_clamped(float v) {
    if (v > 0.f && v <= 1.f) return v;
    if (v <= 0.f) return 0.f;
    return 1.f;
}
inline float h_ps_mul(float a, float b) {
    const float v = a * b;
    return (v != v) ? 0.f : v;
}

struct HostVoxel { float color[4]; float emission[3]; };

// The flattened block data as the device holds it (aic_device.h), read back once per scene version.
struct HostBlocks {
    const std::vector<DevBlock> *blocks = nullptr;
    std::vector<uint16_t> vox;       // pool past the cube grid
    std::vector<DevPaletteEntry> pal;
    size_t n_cubes = 0;
    bool get(const DevBlock &b, const I3h &c, HostVoxel *out) const {  // voxel_storage.rs:731-733 get_opt_evoxel
        const uint32_t res = b.kind & 255u;
        if (res == 0u) {
            if (c[0] == 0 && c[1] == 0 && c[2] == 0) {
                for (int k = 0; k < 4; k++) out->color[k] = b.color[k];
                for (int k = 0; k < 3; k++) out->emission[k] = b.emission[k];
                return true;
            }
            return false;
        }
        const uint32_t vlo[3] = {b.vlo_packed & 255u, (b.vlo_packed >> 8) & 255u, (b.vlo_packed >> 16) & 255u};
        const uint32_t vs[3] = {b.vsize_packed & 255u, (b.vsize_packed >> 8) & 255u, (b.vsize_packed >> 16) & 255u};
        const uint32_t dx = (uint32_t)c[0] - vlo[0], dy = (uint32_t)c[1] - vlo[1], dz = (uint32_t)c[2] - vlo[2];
        if ((dx >= vs[0]) | (dy >= vs[1]) | (dz >= vs[2])) return false;
        const size_t i = ((size_t)dx * vs[1] + dy) * vs[2] + dz;
        const DevPaletteEntry &pe = pal[(size_t)b.pal_off + vox[(size_t)b.vox_off - n_cubes + i]];
        for (int k = 0; k < 4; k++) out->color[k] = pe.color[k];
        for (int k = 0; k < 3; k++) out->emission[k] = pe.emission[k];
        return true;
    }
};

// raytracer_components.rs:215-258 apply_transmittance
inline void h_apply_transmittance(const float color[4], float thickness, float out_color[4], float *out_coeff) {
    thickness = std::fmax(thickness, 0.0f);
    if (thickness == 0.0f) {
        if (color[3] == 1.0f) { for (int k = 0; k < 4; k++) out_color[k] = color[k]; *out_coeff = 1.0f; }
        else { for (int k = 0; k < 4; k++) out_color[k] = 0.f; *out_coeff = 0.0f; }
        return;
    }
    const float unit_transmittance = 1.0f - color[3];
    const float depth_transmittance = std::pow(unit_transmittance, thickness);
    const float alpha = h_zo_new_clamped(1.0f - depth_transmittance);
    out_color[0] = color[0]; out_color[1] = color[1]; out_color[2] = color[2]; out_color[3] = alpha;
    float emission_coeff;
    if (unit_transmittance == 1.0f) emission_coeff = thickness;
    else emission_coeff = (depth_transmittance - 1.f) / (unit_transmittance - 1.f);
    *out_coeff = std::fmax(emission_coeff, 0.0f);
}

// raytracer_components.rs:174-201 trace_for_eval: one axis-aligned ray through the block's voxels
inline void h_trace_for_eval(const HostBlocks &hb, const DevBlock &b, I3h cube, int direction_face, int resolution, float out_color[4], float out_emission[3]) {
    const float thickness = 1.0f / (float)resolution;
    const I3h step = face_normal_h(direction_face);
    float light[3] = {0.f, 0.f, 0.f}, transmittance = 1.0f;  // ColorBuf (raytracer_components.rs:20-39)
    float emission[3] = {0.f, 0.f, 0.f};
    HostVoxel v;
    while (hb.get(b, cube, &v)) {
        float adjusted[4], coeff;
        h_apply_transmittance(v.color, thickness, adjusted, &coeff);
        const float c = h_ps_new_clamped(coeff);
        for (int i = 0; i < 3; i++) emission[i] += h_ps_mul(v.emission[i], c) * transmittance;
        // ColorBuf::from(Rgba) then add_color_internal (raytracer_components.rs:87-92, 149-163)
        for (int i = 0; i < 3; i++) light[i] += (adjusted[i] * adjusted[3]) * transmittance;
        transmittance *= 1.0f - adjusted[3];
        if (transmittance < 1.0f / 256.0f) break;
        for (size_t a = 0; a < 3; a++) cube[a] += step[a];
    }
    // Rgba::from(ColorBuf) (raytracer_components.rs:122-147)
    if (transmittance >= 1.0f) { for (int k = 0; k < 4; k++) out_color[k] = 0.f; }
    else {
        const float color_alpha = 1.0f - transmittance;
        float c3[3];
        bool ok = true;
        for (int i = 0; i < 3; i++) {
            const float q = light[i] / color_alpha;
            if (q > 0.f) c3[i] = q;
            else if (q == 0.f) c3[i] = 0.f;
            else ok = false;
        }
        if (ok) { out_color[0] = c3[0]; out_color[1] = c3[1]; out_color[2] = c3[2]; }
        else { out_color[0] = 1.0f; out_color[1] = 0.0f; out_color[2] = 0.0f; }
        if (color_alpha > 0.f && color_alpha <= 1.f) out_color[3] = color_alpha;
        else if (color_alpha == 0.f) out_color[3] = 0.f;
        else out_color[3] = 1.0f;
    }
    for (int i = 0; i < 3; i++) out_emission[i] = emission[i];
}

// derived.rs:241-292 VoxSum
struct HVoxSum {
    float color_sum[3] = {0.f, 0.f, 0.f}, alpha_sum = 0.f, emission_sum[3] = {0.f, 0.f, 0.f};
    size_t count = 0;
    void add(const float color[4], const float emission[3]) {
        const float alpha = color[3];
        for (int i = 0; i < 3; i++) color_sum[i] += color[i] * alpha;
        alpha_sum += alpha;
        for (int i = 0; i < 3; i++) emission_sum[i] += emission[i];
        count += 1;
    }
    void add(const HVoxSum &o) {
        for (int i = 0; i < 3; i++) { color_sum[i] += o.color_sum[i]; emission_sum[i] += o.emission_sum[i]; }
        alpha_sum += o.alpha_sum;
        count += o.count;
    }
    void color(float surface_area, float out[4]) const {
        if (!(alpha_sum > 0.0f)) { out[0] = out[1] = out[2] = out[3] = 0.f; return; }
        for (int i = 0; i < 3; i++) out[i] = h_ps_new_clamped(color_sum[i] / alpha_sum);
        out[3] = h_zo_new_clamped(alpha_sum / surface_area);
    }
    void emission(float surface_area, float out[3]) const {
        if (count == 0) { out[0] = out[1] = out[2] = 0.f; return; }
        for (int i = 0; i < 3; i++) out[i] = h_ps_new_clamped(emission_sum[i] / surface_area);
    }
};

// EvaluatedBlock::visible() as compute_derived decides it (derived.rs:78-240): a single voxel that is not fully transparent or emits, a voxel volume with
// one such voxel. The one copy of the property: compute_derived_h's kDerivedVisible and the luminance sampler's bitmap (light_visible_bits) both ask here.
bool derived_visible_h(const HostBlocks &hb, const DevBlock &b) {
    if ((b.kind & 255u) == 0u) {
        const bool emits = !(b.emission[0] == 0.f && b.emission[1] == 0.f && b.emission[2] == 0.f);
        return !(b.color[3] <= 0.0f) || emits;
    }
    const int lo[3] = {(int)(b.vlo_packed & 255u), (int)((b.vlo_packed >> 8) & 255u), (int)((b.vlo_packed >> 16) & 255u)};
    const int sz[3] = {(int)(b.vsize_packed & 255u), (int)((b.vsize_packed >> 8) & 255u), (int)((b.vsize_packed >> 16) & 255u)};
    for (int x = lo[0]; x < lo[0] + sz[0]; x++)
        for (int y = lo[1]; y < lo[1] + sz[1]; y++)
            for (int z = lo[2]; z < lo[2] + sz[2]; z++) {
                HostVoxel v;
                std::memset(&v, 0, sizeof(v));
                hb.get(b, I3h{x, y, z}, &v);
                if (!(v.color[3] == 0.f && v.emission[0] == 0.f && v.emission[1] == 0.f && v.emission[2] == 0.f)) return true;
            }
    return false;
}

// derived.rs:78-240 compute_derived, on the flattened block
DevDerived compute_derived_h(const HostBlocks &hb, const DevBlock &b) {
    DevDerived d;
    std::memset(&d, 0, sizeof(d));
    const int res = (int)(b.kind & 255u);
    if (res == 0) {  // Evoxels::single_voxel(): every face is the voxel
        for (int k = 0; k < 4; k++) d.color[k] = b.color[k];
        for (int f = 0; f < 6; f++) for (int k = 0; k < 4; k++) d.face[f][k] = b.color[k];
        for (int k = 0; k < 3; k++) d.emission[k] = b.emission[k];
        if (b.color[3] >= 1.0f) d.flags |= 63u;
        if (derived_visible_h(hb, b)) d.flags |= kDerivedVisible;
        return d;
    }
    const int lo[3] = {(int)(b.vlo_packed & 255u), (int)((b.vlo_packed >> 8) & 255u), (int)((b.vlo_packed >> 16) & 255u)};
    const int sz[3] = {(int)(b.vsize_packed & 255u), (int)((b.vsize_packed >> 8) & 255u), (int)((b.vsize_packed >> 16) & 255u)};
    const int hi[3] = {lo[0] + sz[0], lo[1] + sz[1], lo[2] + sz[2]};
    HVoxSum all;
    for (int f = 0; f < 6; f++) {
        const int axis = f % 3;
        const bool positive = f >= 3;
        const int opposite = positive ? f - 3 : f + 3;
        const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
        HVoxSum fs;
        if (sz[0] > 0 && sz[1] > 0 && sz[2] > 0) {
            for (int v = lo[a2]; v < hi[a2]; v++)
                for (int u = lo[a1]; u < hi[a1]; u++) {
                    I3h c;
                    c[(size_t)axis] = positive ? hi[axis] - 1 : lo[axis];
                    c[(size_t)a1] = u; c[(size_t)a2] = v;
                    float col[4], em[3];
                    h_trace_for_eval(hb, b, c, opposite, res, col, em);
                    fs.add(col, em);
                }
        }
        all.add(fs);
        fs.color((float)res * (float)res, d.face[f]);
    }
    const float surface_area = (float)(6.0 * (double)res * (double)res);
    all.color(surface_area, d.color);
    all.emission(surface_area, d.emission);
    if (derived_visible_h(hb, b)) d.flags |= kDerivedVisible;
    for (int f = 0; f < 6; f++) {
        const int axis = f % 3;
        const bool positive = f >= 3;
        int llo[3] = {0, 0, 0}, lhi[3] = {res, res, res};
        if (positive) llo[axis] = res - 1; else lhi[axis] = 1;
        bool covered = true;  // the layer of voxels just inside the face lies wholly within the stored volume ...
        for (int a = 0; a < 3; a++) covered = covered && lo[a] <= llo[a] && hi[a] >= lhi[a];
        bool all_opaque = covered;
        if (covered)
            for (int x = llo[0]; x < lhi[0] && all_opaque; x++)
                for (int y = llo[1]; y < lhi[1] && all_opaque; y++)
                    for (int z = llo[2]; z < lhi[2]; z++) {
                        HostVoxel v;
                        std::memset(&v, 0, sizeof(v));
                        hb.get(b, I3h{x, y, z}, &v);
                        if (!(v.color[3] >= 1.0f)) { all_opaque = false; break; }  // ... and is fully opaque
                    }
        if (all_opaque) d.flags |= 1u << f;
    }
    return d;
}

// The voxel pool past the cube grid and the palette, read back into `out` for HostBlocks::get. only_if_voxels: nothing is read unless a block has voxels
// (a single-voxel block needs neither pool). On `stream`, and waited for there; a null `stream` is the null stream, whose copies block: light_prepare's,
// which reads the grid and the volume back the same way. The other callers pass their own stream, which runs beside the frames in flight: nothing of
// theirs waits for a frame or goes through the null stream.
int read_host_blocks(aic_ctx *c, Layer &l, hipStream_t stream, bool only_if_voxels, HostBlocks *out) {
    HostBlocks &hb = *out;
    const size_t n = l.n_cubes();
    hb.blocks = &l.host_blocks;
    hb.n_cubes = n;
    if (only_if_voxels) {
        bool any_voxels = false;
        for (const DevBlock &b : l.host_blocks) any_voxels = any_voxels || (b.kind & 255u) != 0u;
        if (!any_voxels) return AIC_OK;
    }
    hb.vox.resize(l.pool.n > n ? l.pool.n - n : 0);
    hb.pal.resize(l.palette.n);
    if (!stream) {
        if (!hb.vox.empty()) HIP_TRY(c, hipMemcpy(hb.vox.data(), l.pool.p + n, hb.vox.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
        if (!hb.pal.empty()) HIP_TRY(c, hipMemcpy(hb.pal.data(), l.palette.p, hb.pal.size() * sizeof(DevPaletteEntry), hipMemcpyDeviceToHost));
        return AIC_OK;
    }
    if (!hb.vox.empty()) HIP_TRY(c, hipMemcpyAsync(hb.vox.data(), l.pool.p + n, hb.vox.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, stream));
    if (!hb.pal.empty()) HIP_TRY(c, hipMemcpyAsync(hb.pal.data(), l.palette.p, hb.pal.size() * sizeof(DevPaletteEntry), hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    return AIC_OK;
}

int derive_blocks(aic_ctx *c, Layer &l, hipStream_t stream, bool only_if_voxels, std::vector<DevDerived> *out) {
    HostBlocks hb;
    if (const int rc = read_host_blocks(c, l, stream, only_if_voxels, &hb)) return rc;
    out->resize(l.host_blocks.size());
    for (size_t i = 0; i < l.host_blocks.size(); i++) (*out)[i] = compute_derived_h(hb, l.host_blocks[i]);
    return AIC_OK;
}

}  // namespace

namespace aic {

int light_prepare_derived(aic_ctx *c, Layer &l, std::vector<DevDerived> *out) { return derive_blocks(c, l, nullptr, false, out); }
int light_rays_derived(aic_ctx *c, Layer &l, hipStream_t stream, std::vector<DevDerived> *out) { return derive_blocks(c, l, stream, true, out); }

// The luminance sampler's bitmap (aic_exposure.h): bit i of `bits` = derived_visible_h of block i, kVisibleBitsWords words whatever the table's size. The
// voxel and palette pools are read back only if a block has voxels, and on `stream` -- the caller's (read_host_blocks).
int light_visible_bits(aic_ctx *c, Layer &l, hipStream_t stream, std::vector<uint32_t> *bits) {
    HostBlocks hb;
    if (const int rc = read_host_blocks(c, l, stream, true, &hb)) return rc;
    bits->assign(kVisibleBitsWords, 0u);
    for (size_t i = 0; i < l.host_blocks.size() && i < 32u * kVisibleBitsWords; i++)
        if (derived_visible_h(hb, l.host_blocks[i])) (*bits)[i >> 5] |= 1u << (i & 31u);
    return AIC_OK;
}

}  // namespace aic
