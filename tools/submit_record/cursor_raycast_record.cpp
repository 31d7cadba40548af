// cursor_raycast_record.cpp -- drives aic_cursor_raycast (csrc/aic_ray_queries.cpp) and what convert_block (csrc/aic_abi.cpp) leaves of
// "selectable" in the block table and the palette pool, against the recording fake (fake_hip.cpp), and prints the record: every runtime call and launch
// with its arguments, each call's return code and message, and after every scene write the bits the cursor raycast will read. The fake's device memory
// is host memory, so the tables are read where the context keeps them. tests/test_cursor_cpu.py builds this with -fsanitize=address,undefined and reads
// the record; a line that begins with FAILED is an expectation of this file that did not hold.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "aic_ctx.h"
#include "record.h"

namespace {

const double kInf = std::numeric_limits<double>::infinity();

void scenario(const char *name) { rec("== %s", name); }
void rec_rc(const aic_ctx *c, const char *call, int rc) { rec("%s rc %d%s%s", call, rc, rc ? " : " : "", rc ? aic_last_error(c) : ""); }
void *dev(size_t bytes) {
    void *p = nullptr;
    (void)hipMalloc(&p, bytes ? bytes : 1);
    return p;
}

// One block of the scenes below: a descriptor with its own voxels and palette
struct Block {
    aic_block_desc d;
    std::vector<uint16_t> vox;
    std::vector<float> pal;  // [n][8]
};
Block block(int resolution, int vs, uint32_t flags, std::vector<uint16_t> vox, std::vector<float> pal) {
    Block b;
    std::memset(&b.d, 0, sizeof(b.d));
    b.d.resolution = resolution;
    b.d.vsize[0] = b.d.vsize[1] = b.d.vsize[2] = vs;
    b.d.pal_len = (uint32_t)(pal.size() / 8);
    b.d.flags = flags;
    b.vox = std::move(vox);
    b.pal = std::move(pal);
    return b;
}
std::vector<float> entry(float a, float emission, float eighth) { return {0.5f, 0.5f, 0.5f, a, emission, 0.f, 0.f, eighth}; }
std::vector<float> entries(std::initializer_list<std::vector<float>> list) {
    std::vector<float> out;
    for (const auto &e : list) out.insert(out.end(), e.begin(), e.end());
    return out;
}
std::vector<uint16_t> cycle(size_t n, uint16_t modulus) {
    std::vector<uint16_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint16_t)(i % modulus);
    return v;
}

// The blocks of the uploaded scene, by what the rule tells apart. The eighth float of an unflagged palette is 0.37: a pad nobody reads.
std::vector<Block> scene_blocks() {
    std::vector<Block> b;
    b.push_back(block(1, 1, AIC_BLOCK_ONE | AIC_BLOCK_AIR, {0}, entry(0.f, 0.f, 0.37f)));                              // 0 AIR
    b.push_back(block(1, 1, AIC_BLOCK_ONE, {0}, entry(1.f, 0.f, 0.37f)));                                              // 1 a visible atom
    b.push_back(block(1, 1, AIC_BLOCK_ONE | AIC_BLOCK_UNSELECTABLE, {0}, entry(1.f, 0.f, 0.37f)));                     // 2 ... unselectable
    b.push_back(block(1, 1, AIC_BLOCK_ONE, {0}, entry(0.f, 0.f, 0.37f)));                                              // 3 an invisible atom, default rule
    b.push_back(block(1, 1, AIC_BLOCK_ONE | AIC_BLOCK_VOXEL_SELECTABLE, {0}, entry(0.f, 0.f, 1.f)));                   // 4 an invisible atom flagged selectable
    b.push_back(block(1, 1, AIC_BLOCK_ONE | AIC_BLOCK_VOXEL_SELECTABLE, {0}, entry(1.f, 0.f, 0.f)));                   // 5 a visible atom flagged unselectable
    b.push_back(block(1, 1, AIC_BLOCK_ONE | AIC_BLOCK_VOXEL_SELECTABLE | AIC_BLOCK_AIR, {0}, entry(0.f, 0.f, 1.f)));   // 6 AIR with a selectable voxel: AIR wins
    // 7 voxels, default rule: invisible, visible, emitting (the device order puts the invisible entry first whatever the order here)
    b.push_back(block(2, 2, 0, cycle(8, 3), entries({entry(1.f, 0.f, 0.37f), entry(0.f, 0.f, 0.37f), entry(0.f, 2.f, 0.37f)})));
    // 8 voxels, flagged: visible and unselectable, invisible and selectable, visible and selectable, invisible and unselectable
    b.push_back(block(2, 2, AIC_BLOCK_VOXEL_SELECTABLE, cycle(8, 4), entries({entry(1.f, 0.f, 0.f), entry(0.f, 0.f, 1.f), entry(0.5f, 0.f, 1.f), entry(0.f, 0.f, 0.f)})));
    // 9 the same voxels in an unselectable block
    b.push_back(block(2, 2, AIC_BLOCK_VOXEL_SELECTABLE | AIC_BLOCK_UNSELECTABLE, cycle(8, 4), entries({entry(1.f, 0.f, 0.f), entry(0.f, 0.f, 1.f), entry(0.5f, 0.f, 1.f), entry(0.f, 0.f, 0.f)})));
    // 10 resolution 1 with a stored voxel, not Evoxels::One: a single voxel all the same
    b.push_back(block(1, 1, AIC_BLOCK_VOXEL_SELECTABLE, {1}, entries({entry(1.f, 0.f, 1.f), entry(1.f, 0.f, 0.f)})));
    return b;
}

aic_ctx *make_ctx(const std::vector<Block> &blocks, int expect = AIC_OK) {
    int st = 0;
    aic_ctx *c = aic_create(0, &st);
    static const std::vector<uint16_t> cubes(64, 1);
    static const std::vector<uint8_t> light(64 * 4, 0);
    std::vector<aic_block_desc> descs;
    std::vector<uint16_t> vox;
    std::vector<float> pal;
    for (const Block &b : blocks) {
        aic_block_desc d = b.d;
        d.vox_off = (uint32_t)vox.size();
        d.pal_off = (uint32_t)(pal.size() / 8);
        vox.insert(vox.end(), b.vox.begin(), b.vox.end());
        pal.insert(pal.end(), b.pal.begin(), b.pal.end());
        descs.push_back(d);
    }
    aic_space_desc s;
    std::memset(&s, 0, sizeof(s));
    s.size[0] = s.size[1] = s.size[2] = 4;
    s.block_index = cubes.data(); s.light = light.data(); s.n_blocks = (uint32_t)descs.size(); s.blocks = descs.data();
    s.voxels = vox.data(); s.n_voxels = vox.size(); s.palette = pal.data(); s.n_palette = pal.size() / 8;
    const int rc = aic_upload_space(c, 0, &s);
    rec_rc(c, "aic_upload_space", rc);
    if (rc != expect) rec("FAILED aic_upload_space: rc %d, expected %d", rc, expect);
    return c;
}

// What the kernel will read of block i: the block's bit, and for a block with voxels each palette entry's visibility and float in the device's order
void rec_bits(const aic_ctx *c, const char *when) {
    const Layer &l = c->layers[0];
    rec("-- bits %s: %zu blocks", when, l.host_blocks.size());
    for (size_t i = 0; i < l.host_blocks.size(); i++) {
        const DevBlock &b = l.blocks.p[i];
        if (std::memcmp(&b, &l.host_blocks[i], sizeof(b))) rec("FAILED block %zu: the table on the device differs from its mirror", i);
        if (b.pad[0] & ~kBlockSelectable || b.pad[1] || b.pad[2]) rec("FAILED block %zu: pad words %u %u %u", i, b.pad[0], b.pad[1], b.pad[2]);
        std::string line = "  block " + std::to_string(i) + " resolution " + std::to_string(b.kind & 255u) + " selectable " + std::to_string(b.pad[0] & kBlockSelectable);
        if (b.kind & 255u) {
            const uint32_t sz = b.vsize_packed;
            const size_t nvox = (size_t)(sz & 255u) * ((sz >> 8) & 255u) * ((sz >> 16) & 255u);
            uint32_t n_pal = 0;
            for (size_t v = 0; v < nvox; v++) n_pal = std::max<uint32_t>(n_pal, l.pool.p[b.vox_off + v] + 1u);
            line += " palette";
            for (uint32_t k = 0; k < n_pal; k++) {
                const DevPaletteEntry &e = l.palette.p[b.pal_off + k];
                const bool inv = e.color[3] == 0.f && e.emission[0] == 0.f && e.emission[1] == 0.f && e.emission[2] == 0.f;
                if (inv != (k < b.n_invisible)) line += " FAILED(order)";
                uint32_t bits;
                std::memcpy(&bits, &e.pad, 4);
                if (bits != 0u && bits != 0x3f800000u) line += " FAILED(pattern)";
                line += std::string(" ") + (inv ? "i" : "v") + (e.pad != 0.f ? "1" : "0");
            }
        }
        rec("%s", line.c_str());
    }
}

int raycast(aic_ctx *c, int layer, uint32_t n, const double *rays, double maximum_distance, uint32_t flags, aic_cursor_hit *out) {
    const int rc = aic_cursor_raycast(c, layer, n, rays, maximum_distance, flags, out);
    rec_rc(c, "aic_cursor_raycast", rc);
    return rc;
}

const char *const kQueued[] = {"hipMalloc", "hipMemcpyAsync", "hipMemcpy", "hipMemsetAsync", "hipStreamSynchronize", "launch_cursor_raycast"};
int queued() {
    int n = 0;
    for (const char *fn : kQueued) n += fake_calls(fn);
    return n;
}

void rejections() {
    scenario("rejections");
    aic_ctx *c = make_ctx(scene_blocks());
    std::vector<double> rays(6 * 10, 0.25);
    std::vector<aic_cursor_hit> out(10);
    std::memset(out.data(), 0x5a, out.size() * sizeof(aic_cursor_hit));
    const std::vector<aic_cursor_hit> untouched = out;
    char *d_rays = (char *)dev(48 * 10 + 8), *d_out = (char *)dev(144 * 10 + 8);
    struct Case { const char *what; aic_ctx *c; int layer; uint32_t n; const double *rays; double md; uint32_t flags; aic_cursor_hit *out; };
    const Case cases[] = {
        {"no context", nullptr, 0, 10, rays.data(), kInf, 0, out.data()},
        {"no rays", c, 0, 10, nullptr, kInf, 0, out.data()},
        {"no out", c, 0, 10, rays.data(), kInf, 0, nullptr},
        {"unknown flag", c, 0, 10, rays.data(), kInf, 1, out.data()},
        {"unknown flag beside AIC_RAYS_DEVICE", c, 0, 10, (const double *)d_rays, kInf, AIC_RAYS_DEVICE | 128u, (aic_cursor_hit *)d_out},
        {"a layer with no space", c, AIC_LAYER_UI, 10, rays.data(), kInf, 0, out.data()},
        {"no such layer", c, 2, 10, rays.data(), kInf, 0, out.data()},
        {"NaN maximum_distance", c, 0, 10, rays.data(), std::nan(""), 0, out.data()},
        {"negative maximum_distance", c, 0, 10, rays.data(), -1.0, 0, out.data()},
        {"minus infinity", c, 0, 10, rays.data(), -kInf, 0, out.data()},
        {"too many rays", c, 0, (1u << 20) + 1u, rays.data(), kInf, 0, out.data()},
        {"device rays off by 4", c, 0, 10, (const double *)(d_rays + 4), kInf, AIC_RAYS_DEVICE, (aic_cursor_hit *)d_out},
        {"device out off by 4", c, 0, 10, (const double *)d_rays, kInf, AIC_RAYS_DEVICE, (aic_cursor_hit *)(d_out + 4)},
        {"NULL pointers with n = 0 and a bad distance", c, 0, 0, nullptr, std::nan(""), 0, nullptr},
    };
    for (const Case &k : cases) {
        rec("-- reject: %s", k.what);
        const int before = queued();
        const int rc = raycast(k.c, k.layer, k.n, k.rays, k.md, k.flags, k.out);
        if (rc != AIC_ERR_INVALID) rec("FAILED %s: rc %d", k.what, rc);
        if (queued() != before) rec("FAILED %s: something was queued", k.what);
        if (std::memcmp(out.data(), untouched.data(), out.size() * sizeof(aic_cursor_hit))) rec("FAILED %s: out was written", k.what);
        // ... and the context is usable: the good call
        rec("-- after: %s", k.what);
        const int launches = fake_calls("launch_cursor_raycast");
        std::vector<aic_cursor_hit> good(10);
        if (raycast(c, 0, 10, rays.data(), kInf, 0, good.data()) != AIC_OK || fake_calls("launch_cursor_raycast") != launches + 1) rec("FAILED after %s: the good call", k.what);
    }
    rec("-- legal: n = 0 with NULL pointers; maximum_distance 0 and +infinity");
    const int before = queued();
    if (raycast(c, 0, 0, nullptr, kInf, 0, nullptr) != AIC_OK || queued() != before) rec("FAILED n = 0 did something");
    if (raycast(c, 0, 10, rays.data(), 0.0, 0, out.data()) != AIC_OK) rec("FAILED maximum_distance 0");
    (void)hipFree(d_rays); (void)hipFree(d_out);
    aic_destroy(c);
}

void launches() {
    for (uint32_t n : {1u, 10u, 64u, 65u, 130u, 4096u}) {
        for (int on_device = 0; on_device < 2; on_device++) {
            scenario(("launch " + std::to_string(n) + " " + std::to_string(on_device)).c_str());
            fake_reset();
            aic_ctx *c = make_ctx(scene_blocks());
            std::vector<double> rays(6 * (size_t)n, 0.25);
            std::vector<aic_cursor_hit> out(n);
            void *d_rays = on_device ? dev(48 * (size_t)n) : nullptr, *d_out = on_device ? dev(144 * (size_t)n) : nullptr;
            for (int turn = 0; turn < 2; turn++) {  // (the second call finds the staging where the first left it)
                rec("-- call %d", turn);
                const int l0 = fake_calls("launch_cursor_raycast"), m0 = fake_calls("hipMemcpyAsync"), a0 = fake_calls("hipMalloc");
                const int rc = on_device ? raycast(c, 0, n, (const double *)d_rays, 6.0, AIC_RAYS_DEVICE, (aic_cursor_hit *)d_out) : raycast(c, 0, n, rays.data(), 6.0, 0, out.data());
                if (rc != AIC_OK) rec("FAILED launch %u", n);
                if (fake_calls("launch_cursor_raycast") != l0 + 1) rec("FAILED launch %u: not one launch", n);
                if (fake_calls("hipMemcpyAsync") != m0 + (on_device ? 0 : 2)) rec("FAILED launch %u: copies", n);
                if (fake_calls("hipMalloc") != a0 + (!on_device && turn == 0 ? 1 : 0)) rec("FAILED launch %u: allocations", n);
            }
            if (d_rays) { (void)hipFree(d_rays); (void)hipFree(d_out); }
            aic_destroy(c);
        }
    }
}

void bits() {
    scenario("bits");
    fake_reset();
    std::vector<Block> blocks = scene_blocks();
    aic_ctx *c = make_ctx(blocks);
    rec_bits(c, "after aic_upload_space");
    // in place: the visible atom becomes unselectable; the flagged voxel block swaps its two visible entries' floats (the same ranges hold it)
    Block dull = blocks[2];
    rec_rc(c, "aic_replace_block", aic_replace_block(c, 0, 1, &dull.d, dull.vox.data(), dull.pal.data()));
    Block swapped = block(2, 2, AIC_BLOCK_VOXEL_SELECTABLE, cycle(8, 4), entries({entry(1.f, 0.f, 1.f), entry(0.f, 0.f, 1.f), entry(0.5f, 0.f, 0.f), entry(0.f, 0.f, 0.f)}));
    const uint32_t pal_off_before = c->layers[0].host_blocks[8].pal_off;
    rec_rc(c, "aic_replace_block", aic_replace_block(c, 0, 8, &swapped.d, swapped.vox.data(), swapped.pal.data()));
    if (c->layers[0].host_blocks[8].pal_off != pal_off_before) rec("FAILED the replacement that fits was not made in place");
    rec_bits(c, "after two replacements in place");
    // appended: block 7 outgrows its ranges (2^3 -> 4^3 voxels, five palette entries, flagged now); a new block 11 at the table's end, unselectable
    Block grown = block(4, 4, AIC_BLOCK_VOXEL_SELECTABLE, cycle(64, 5),
                        entries({entry(0.f, 0.f, 1.f), entry(1.f, 0.f, 0.f), entry(0.f, 0.f, 0.f), entry(1.f, 0.f, 1.f), entry(0.f, 3.f, 0.f)}));
    const uint32_t vox_off_before = c->layers[0].host_blocks[7].vox_off;
    rec_rc(c, "aic_replace_block", aic_replace_block(c, 0, 7, &grown.d, grown.vox.data(), grown.pal.data()));
    if (c->layers[0].host_blocks[7].vox_off == vox_off_before) rec("FAILED the replacement that does not fit was made in place");
    Block extra = blocks[9];
    const uint32_t idx[2] = {11u, 12u};
    Block extra2 = blocks[4];
    const aic_block_desc descs[2] = {extra.d, extra2.d};
    const uint16_t *voxs[2] = {extra.vox.data(), extra2.vox.data()};
    const float *pals[2] = {extra.pal.data(), extra2.pal.data()};
    rec_rc(c, "aic_replace_blocks", aic_replace_blocks(c, 0, 2, idx, descs, voxs, pals));
    rec_bits(c, "after a block grown past its ranges and two appended");
    rec_rc(c, "aic_compact", aic_compact(c, 0));
    rec_bits(c, "after aic_compact");
    // a palette that does not say 1.0f or +0.0f under the flag is refused whole, by the upload and by a replacement, and nothing changes
    const float bad_values[] = {0.5f, -0.0f, 2.f, std::nanf(""), -1.f};
    for (float bad : bad_values) {
        Block b = block(2, 2, AIC_BLOCK_VOXEL_SELECTABLE, cycle(8, 2), entries({entry(1.f, 0.f, 1.f), entry(0.f, 0.f, bad)}));
        const int rc = aic_replace_block(c, 0, 8, &b.d, b.vox.data(), b.pal.data());
        rec_rc(c, "aic_replace_block", rc);
        if (rc != AIC_ERR_INVALID) rec("FAILED eighth float %a accepted", bad);
        b.d.flags = 0;  // ... and is an ignored pad without it
        Block atom1 = block(1, 1, AIC_BLOCK_ONE, {0}, entry(1.f, 0.f, bad));
        if (aic_replace_block(c, 0, 12, &atom1.d, atom1.vox.data(), atom1.pal.data()) != AIC_OK) rec("FAILED eighth float %a refused without the flag", bad);
    }
    rec_bits(c, "after the refused palettes");
    aic_destroy(c);
    scenario("bits: an upload with a bad palette");
    fake_reset();
    blocks[8].pal[7] = 0.25f;
    aic_ctx *c2 = make_ctx(blocks, AIC_ERR_INVALID);
    std::vector<double> rays(6, 0.25);
    aic_cursor_hit out;
    if (raycast(c2, 0, 1, rays.data(), kInf, 0, &out) != AIC_ERR_INVALID) rec("FAILED a raycast of the layer whose upload was refused");
    aic_destroy(c2);
}

void failures() {
    for (int on_device = 0; on_device < 2; on_device++) {
        struct Fail { const char *fn; int nth; };
        const Fail fails[] = {{"hipSetDevice", 0}, {"hipMalloc", 0}, {"hipMemcpyAsync", 0}, {"hipMemcpyAsync", 1}, {"launch_cursor_raycast", 0}, {"hipStreamSynchronize", 0}};
        for (const Fail &f : fails) {
            if (on_device && (!std::strcmp(f.fn, "hipMalloc") || !std::strcmp(f.fn, "hipMemcpyAsync"))) continue;  // (a device list stages nothing)
            scenario(("failures: " + std::to_string(on_device) + " " + f.fn + " " + std::to_string(f.nth)).c_str());
            fake_reset();
            aic_ctx *c = make_ctx(scene_blocks());
            std::vector<double> rays(6 * 70, 0.25);
            std::vector<aic_cursor_hit> out(70);
            void *d_rays = on_device ? dev(48 * 70) : nullptr, *d_out = on_device ? dev(144 * 70) : nullptr;
            auto call = [&]() { return on_device ? raycast(c, 0, 70, (const double *)d_rays, kInf, AIC_RAYS_DEVICE, (aic_cursor_hit *)d_out) : raycast(c, 0, 70, rays.data(), kInf, 0, out.data()); };
            fake_fail(f.fn, f.nth);
            if (call() == AIC_OK) rec("FAILED the failing call returned AIC_OK");
            rec("-- the same call again");
            if (call() != AIC_OK) rec("FAILED the call after the failure");
            if (d_rays) { (void)hipFree(d_rays); (void)hipFree(d_out); }
            aic_destroy(c);
        }
    }
}

}  // namespace

int main() {
    rejections();
    launches();
    bits();
    failures();
    scenario("end");
    fake_reset();
    return 0;
}
