// light_rays_record.cpp -- drives aic_light_rays (csrc/aic_light_rays_host.cpp) against the recording fake (fake_hip.cpp) and prints the record: every
// runtime call and launch with its arguments, each call's return code and message. The fake's tree has ten positions and a bound of three records a
// cube; its scan answers two records a cube and stores what the capacity holds; its emitters write every byte they may. tests/test_light_rays_cpu.py
// builds this with -fsanitize=address,undefined and reads the record; a line that begins with FAILED is an expectation of this file that did not hold.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "aic_ctx.h"
#include "record.h"

namespace {

void scenario(const char *name) { rec("== %s", name); }
void rec_rc(const aic_ctx *c, const char *call, int rc) { rec("%s rc %d%s%s", call, rc, rc ? " : " : "", rc ? aic_last_error(c) : ""); }
void *dev(size_t bytes) {
    void *p = nullptr;
    (void)hipMalloc(&p, bytes ? bytes : 1);
    return p;
}

aic_ctx *make_ctx() {
    int st = 0;
    aic_ctx *c = aic_create(0, &st);
    static const std::vector<uint16_t> cubes(64, 1);
    static const std::vector<uint8_t> light(64 * 4, 0);
    static const float pal[2][8] = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f, 1.f, 0.f, 0.f, 0.f, 0.f}};
    static const uint16_t vox[2] = {0, 0};
    aic_block_desc descs[2];
    std::memset(descs, 0, sizeof(descs));
    for (int i = 0; i < 2; i++) {
        descs[i].resolution = 1;
        descs[i].vsize[0] = descs[i].vsize[1] = descs[i].vsize[2] = 1;
        descs[i].pal_len = 1;
        descs[i].vox_off = (uint32_t)i;
        descs[i].pal_off = (uint32_t)i;
        descs[i].flags = AIC_BLOCK_ONE | (i == 0 ? AIC_BLOCK_AIR : 0u);
    }
    aic_space_desc s;
    std::memset(&s, 0, sizeof(s));
    s.size[0] = s.size[1] = s.size[2] = 4;
    s.block_index = cubes.data(); s.light = light.data(); s.n_blocks = 2; s.blocks = descs;
    s.voxels = vox; s.n_voxels = 2; s.palette = &pal[0][0]; s.n_palette = 2;
    const int rc = aic_upload_space(c, 0, &s);
    rec_rc(c, "aic_upload_space", rc);
    if (rc != AIC_OK) rec("FAILED aic_upload_space");
    return c;
}

int call(aic_ctx *c, int layer, uint32_t n, const int32_t *cubes, int32_t md, uint32_t flags, uint32_t capacity, aic_light_cube_info *infos, aic_light_ray *rays,
         aic_line_vertex *lines, uint64_t *totals) {
    const int rc = aic_light_rays(c, layer, n, cubes, md, flags, capacity, infos, rays, lines, totals);
    rec_rc(c, "aic_light_rays", rc);
    return rc;
}

const char *const kQueued[] = {"hipMalloc", "hipMemcpyAsync", "hipMemcpy", "hipMemsetAsync", "hipStreamSynchronize", "launch_light_rays_walk", "launch_light_rays_scan",
                               "launch_light_rays_emit", "light_rays_derived"};
int queued() {
    int n = 0;
    for (const char *fn : kQueued) n += fake_calls(fn);
    return n;
}

int g_finished = 0;
int finish_hook(aic_ctx *c) {
    if (c->ljob.pending) {
        rec("light_job_finish: a pending update");
        c->ljob.pending = false;
        g_finished++;
    }
    return 0;
}

void rejections() {
    scenario("rejections");
    aic_ctx *c = make_ctx();
    const uint32_t n = 10;
    std::vector<int32_t> cubes(3 * n, 1);
    std::vector<aic_light_cube_info> infos(n);
    std::vector<aic_light_ray> rays(2 * n);
    std::vector<aic_line_vertex> lines(2 * (12 * n + 29 * 2 * n));
    std::memset(infos.data(), 0x5a, infos.size() * sizeof(infos[0]));
    std::memset(rays.data(), 0x5a, rays.size() * sizeof(rays[0]));
    const std::vector<aic_light_cube_info> infos0 = infos;
    char *d_rays = (char *)dev(40 * 2 * n + 8), *d_lines = (char *)dev(sizeof(aic_line_vertex) * lines.size() + 8);
    struct Case { const char *what; aic_ctx *c; int layer; uint32_t n; const int32_t *cubes; int32_t md; uint32_t flags; aic_light_ray *rays; aic_line_vertex *lines; };
    const Case cases[] = {
        {"no context", nullptr, 0, n, cubes.data(), 6, 0, rays.data(), lines.data()},
        {"no cubes", c, 0, n, nullptr, 6, 0, rays.data(), lines.data()},
        {"unknown flag", c, 0, n, cubes.data(), 6, 2, rays.data(), lines.data()},
        {"unknown flag beside AIC_LIGHT_RAYS_DEVICE", c, 0, n, cubes.data(), 6, AIC_LIGHT_RAYS_DEVICE | 256u, (aic_light_ray *)d_rays, (aic_line_vertex *)d_lines},
        {"a layer with no space", c, AIC_LAYER_UI, n, cubes.data(), 6, 0, rays.data(), lines.data()},
        {"no such layer", c, 2, n, cubes.data(), 6, 0, rays.data(), lines.data()},
        {"negative maximum_distance", c, 0, n, cubes.data(), -1, 0, rays.data(), lines.data()},
        {"maximum_distance 256", c, 0, n, cubes.data(), 256, 0, rays.data(), lines.data()},
        {"too many cubes", c, 0, (1u << 16) + 1u, cubes.data(), 6, 0, rays.data(), lines.data()},
        {"device rays off by 2", c, 0, n, cubes.data(), 6, AIC_LIGHT_RAYS_DEVICE, (aic_light_ray *)(d_rays + 2), (aic_line_vertex *)d_lines},
        {"device lines off by 1", c, 0, n, cubes.data(), 6, AIC_LIGHT_RAYS_DEVICE, (aic_light_ray *)d_rays, (aic_line_vertex *)(d_lines + 1)},
    };
    for (const Case &k : cases) {
        rec("-- reject: %s", k.what);
        const int before = queued();
        uint64_t totals[2] = {7, 7};
        const int rc = call(k.c, k.layer, k.n, k.cubes, k.md, k.flags, 2 * n, infos.data(), k.rays, k.lines, totals);
        if (rc != AIC_ERR_INVALID) rec("FAILED %s: rc %d", k.what, rc);
        if (queued() != before) rec("FAILED %s: something was queued", k.what);
        if (std::memcmp(infos.data(), infos0.data(), infos.size() * sizeof(infos[0])) || totals[0] != 7 || totals[1] != 7) rec("FAILED %s: an output was written", k.what);
        rec("-- after: %s", k.what);
        const int launches = fake_calls("launch_light_rays_walk");
        std::vector<aic_light_cube_info> good(n);
        if (call(c, 0, n, cubes.data(), 6, 0, 2 * n, good.data(), rays.data(), lines.data(), totals) != AIC_OK || fake_calls("launch_light_rays_walk") != launches + 1 ||
            totals[0] != 2 * n || totals[1] != 12 * n + 29 * 2 * n)
            rec("FAILED after %s: the good call", k.what);
    }
    rec("-- legal: n = 0 with NULL pointers; maximum_distance 0 and 255; every output NULL");
    const int before = queued();
    uint64_t totals[2] = {7, 7};
    if (call(c, 0, 0, nullptr, 6, 0, 0, nullptr, nullptr, nullptr, totals) != AIC_OK || queued() != before || totals[0] || totals[1]) rec("FAILED n = 0 did something");
    if (call(c, 0, n, cubes.data(), 0, 0, 2 * n, infos.data(), rays.data(), lines.data(), totals) != AIC_OK) rec("FAILED maximum_distance 0");
    if (call(c, 0, n, cubes.data(), 255, 0, 2 * n, infos.data(), rays.data(), lines.data(), totals) != AIC_OK) rec("FAILED maximum_distance 255");
    const int emits = fake_calls("launch_light_rays_emit");
    if (call(c, 0, n, cubes.data(), 6, 0, 2 * n, nullptr, nullptr, nullptr, nullptr) != AIC_OK || fake_calls("launch_light_rays_emit") != emits) rec("FAILED every output NULL");
    (void)hipFree(d_rays); (void)hipFree(d_lines);
    aic_destroy(c);
}

// host lists are staged in context scratch and copied back; device lists stage nothing; the second call allocates nothing and makes no tables again
void launches() {
    for (uint32_t n : {1u, 63u, 64u, 65u, 300u}) {
        for (int on_device = 0; on_device < 2; on_device++) {
            for (uint32_t capacity : {2u * n, 2u * n - 1u, 0u}) {
                scenario(("launch " + std::to_string(n) + " " + std::to_string(on_device) + " " + std::to_string(capacity)).c_str());
                fake_reset();
                aic_ctx *c = make_ctx();
                std::vector<int32_t> cubes(3 * (size_t)n, 1);
                std::vector<aic_light_cube_info> infos(n);
                const uint32_t stored = capacity / 2u < n ? capacity / 2u : n;
                // exactly what the header promises to need: the sanitizer sees a byte more
                std::vector<aic_light_ray> rays(capacity);
                std::vector<aic_line_vertex> lines(2 * (12 * (size_t)n + 29 * (size_t)capacity));
                aic_light_ray *d_rays = on_device ? (aic_light_ray *)dev(sizeof(aic_light_ray) * capacity) : nullptr;
                aic_line_vertex *d_lines = on_device ? (aic_line_vertex *)dev(sizeof(aic_line_vertex) * lines.size()) : nullptr;
                for (int turn = 0; turn < 2; turn++) {
                    rec("-- call %d", turn);
                    const int w0 = fake_calls("launch_light_rays_walk"), s0 = fake_calls("launch_light_rays_scan"), e0 = fake_calls("launch_light_rays_emit"),
                              m0 = fake_calls("hipMemcpyAsync"), a0 = fake_calls("hipMalloc"), t0 = fake_calls("light_rays_derived");
                    uint64_t totals[2] = {0, 0};
                    const int rc = on_device ? call(c, 0, n, cubes.data(), 6, AIC_LIGHT_RAYS_DEVICE, capacity, infos.data(), d_rays, d_lines, totals)
                                             : call(c, 0, n, cubes.data(), 6, 0, capacity, infos.data(), rays.data(), lines.data(), totals);
                    if (rc != AIC_OK) rec("FAILED launch %u", n);
                    if (totals[0] != 2ull * n || totals[1] != 12ull * n + 58ull * n) rec("FAILED launch %u: totals", n);
                    if (fake_calls("launch_light_rays_walk") != w0 + 1 || fake_calls("launch_light_rays_scan") != s0 + 1 || fake_calls("launch_light_rays_emit") != e0 + 1)
                        rec("FAILED launch %u: not one launch each", n);
                    // copies: the tables (three of the tree, one of the derived properties) the first time; the cubes, the totals, the infos; a host list's records and lines
                    const int copies = (turn == 0 ? 4 : 0) + 3 + (!on_device && stored ? 2 : 0);
                    if (fake_calls("hipMemcpyAsync") != m0 + copies) rec("FAILED launch %u: %d copies, expected %d", n, fake_calls("hipMemcpyAsync") - m0, copies);
                    if (fake_calls("hipMalloc") != a0 + (turn == 0 ? 3 : 0)) rec("FAILED launch %u: allocations", n);
                    if (fake_calls("light_rays_derived") != t0 + (turn == 0 ? 1 : 0)) rec("FAILED launch %u: the derived properties were made %d times", n, fake_calls("light_rays_derived") - t0);
                    uint32_t n_stored = 0;
                    for (const aic_light_cube_info &i : infos) n_stored += (i.flags & AIC_LIGHT_CUBE_STORED) ? 1u : 0u;
                    if (n_stored != stored) rec("FAILED launch %u: %u cubes stored, expected %u", n, n_stored, stored);
                    if (!on_device && stored && (((const unsigned char *)rays.data())[0] != 0x11 || ((const unsigned char *)lines.data())[0] != 0x22)) rec("FAILED launch %u: nothing was copied back", n);
                }
                if (d_rays) { (void)hipFree(d_rays); (void)hipFree(d_lines); }
                aic_destroy(c);
            }
        }
    }
}

void tables() {
    scenario("tables: another distance makes the tree again, a scene write the derived properties");
    fake_reset();
    aic_ctx *c = make_ctx();
    std::vector<int32_t> cubes(3, 1);
    aic_light_cube_info info;
    auto one = [&](int32_t md) { return call(c, 0, 1, cubes.data(), md, 0, 0, &info, nullptr, nullptr, nullptr); };
    (void)one(6);
    const int d0 = fake_calls("light_rays_derived");
    rec("-- the same again");
    (void)one(6);
    if (fake_calls("light_rays_derived") != d0) rec("FAILED the derived properties were made again");
    rec("-- distance 7");
    (void)one(7);
    if (fake_calls("light_rays_derived") != d0) rec("FAILED the derived properties were made again for another distance");
    rec("-- after aic_update_cubes");
    const int32_t xyz[3] = {0, 0, 0};
    const uint16_t bi[1] = {0};
    rec_rc(c, "aic_update_cubes", aic_update_cubes(c, 0, 1, xyz, bi, nullptr));
    (void)one(7);
    if (fake_calls("light_rays_derived") != d0 + 1) rec("FAILED the derived properties were not made again after a scene write");
    aic_destroy(c);
}

void pending_update() {
    scenario("a pending light update is finished first");
    fake_reset();
    aic_ctx *c = make_ctx();
    fake_light_job_finish = finish_hook;
    std::vector<int32_t> cubes(3, 1);
    aic_light_cube_info info;
    c->ljob.pending = true;
    g_finished = 0;
    if (call(c, 0, 1, cubes.data(), 6, 0, 0, &info, nullptr, nullptr, nullptr) != AIC_OK || g_finished != 1) rec("FAILED the pending update was not finished");
    c->ljob.pending = true;
    rec("-- a rejected call finishes nothing");
    if (call(c, 0, 1, cubes.data(), 300, 0, 0, &info, nullptr, nullptr, nullptr) != AIC_ERR_INVALID || g_finished != 1 || !c->ljob.pending) rec("FAILED a rejected call finished the update");
    c->ljob.pending = false;
    fake_light_job_finish = nullptr;
    aic_destroy(c);
}

// aic_light_rays_cursor_lines: the caller's lines and the cube's behind them in one device list of the context's
void cursor_lines() {
    scenario("cursor lines: one device list");
    fake_reset();
    aic_ctx *c = make_ctx();
    const int32_t cube[3] = {1, 1, 1};
    std::vector<aic_line_vertex> first(2 * 28);
    std::memset(first.data(), 0x66, first.size() * sizeof(first[0]));
    const aic_line_vertex *list = nullptr;
    uint32_t n = 0;
    aic_light_cube_info info;
    for (int turn = 0; turn < 2; turn++) {
        rec("-- call %d", turn);
        const int a0 = fake_calls("hipMalloc");
        const int rc = aic_light_rays_cursor_lines(c, 0, cube, 6, first.data(), 28, &info, &list, &n);
        rec_rc(c, "aic_light_rays_cursor_lines", rc);
        rec("  list %s n_lines %u", rec_ptr(list).c_str(), n);
        if (rc != AIC_OK || n != 28u + 12u + 29u * 2u || rec_ptr(list) == "host" || rec_ptr(list) == "null") rec("FAILED the list");
        else if (std::memcmp(list, first.data(), first.size() * sizeof(first[0])) || ((const unsigned char *)(list + 2 * 28))[0] != 0x22) rec("FAILED the list's contents");
        if (info.n_rays != 2 || !(info.flags & AIC_LIGHT_CUBE_STORED)) rec("FAILED the info");
        if (fake_calls("hipMalloc") != a0 + (turn == 0 ? 4 : 0)) rec("FAILED allocations");
    }
    rec("-- no lines first");
    if (aic_light_rays_cursor_lines(c, 0, cube, 6, nullptr, 0, nullptr, &list, &n) != AIC_OK || n != 12u + 58u) rec("FAILED no lines first");
    struct Case { const char *what; int layer; const int32_t *cube; int32_t md; const aic_line_vertex *first; uint32_t n_first; const aic_line_vertex **list; uint32_t *n; };
    const Case cases[] = {
        {"no cube", 0, nullptr, 6, first.data(), 28, &list, &n},       {"no list", 0, cube, 6, first.data(), 28, nullptr, &n},
        {"no count", 0, cube, 6, first.data(), 28, &list, nullptr},    {"lines first without a pointer", 0, cube, 6, nullptr, 28, &list, &n},
        {"maximum_distance 256", 0, cube, 256, first.data(), 28, &list, &n}, {"a layer with no space", AIC_LAYER_UI, cube, 6, first.data(), 28, &list, &n},
        {"too many lines", 0, cube, 6, first.data(), AIC_LINES_MAX, &list, &n},
    };
    for (const Case &k : cases) {
        rec("-- reject: %s", k.what);
        const int before = queued();
        const int rc = aic_light_rays_cursor_lines(c, k.layer, k.cube, k.md, k.first, k.n_first, nullptr, k.list, k.n);
        rec_rc(c, "aic_light_rays_cursor_lines", rc);
        if (rc != AIC_ERR_INVALID || queued() != before) rec("FAILED %s", k.what);
    }
    aic_destroy(c);
}

void failures() {
    for (int on_device = 0; on_device < 2; on_device++) {
        struct Fail { const char *fn; int nth; };
        const Fail fails[] = {{"hipSetDevice", 0}, {"hipMalloc", 0}, {"hipMalloc", 1}, {"hipMalloc", 2}, {"hipMemcpyAsync", 0}, {"hipMemcpyAsync", 3}, {"hipMemcpyAsync", 4},
                              {"hipMemcpyAsync", 5}, {"hipMemcpyAsync", 7}, {"light_rays_derived", 0}, {"launch_light_rays_walk", 0}, {"launch_light_rays_scan", 0},
                              {"launch_light_rays_emit", 0}, {"hipStreamSynchronize", 0}, {"hipStreamSynchronize", 2}, {"hipStreamSynchronize", 3}};
        for (const Fail &f : fails) {
            if (on_device && !std::strcmp(f.fn, "hipMemcpyAsync") && f.nth == 7) continue;  // (a device list copies nothing back)
            scenario(("failures: " + std::to_string(on_device) + " " + f.fn + " " + std::to_string(f.nth)).c_str());
            fake_reset();
            aic_ctx *c = make_ctx();
            const uint32_t n = 70;
            std::vector<int32_t> cubes(3 * n, 1);
            std::vector<aic_light_cube_info> infos(n);
            std::vector<aic_light_ray> rays(2 * n);
            std::vector<aic_line_vertex> lines(2 * (12 * n + 29 * 2 * n));
            aic_light_ray *d_rays = on_device ? (aic_light_ray *)dev(sizeof(aic_light_ray) * rays.size()) : nullptr;
            aic_line_vertex *d_lines = on_device ? (aic_line_vertex *)dev(sizeof(aic_line_vertex) * lines.size()) : nullptr;
            auto go = [&]() {
                return on_device ? call(c, 0, n, cubes.data(), 6, AIC_LIGHT_RAYS_DEVICE, 2 * n, infos.data(), d_rays, d_lines, nullptr)
                                 : call(c, 0, n, cubes.data(), 6, 0, 2 * n, infos.data(), rays.data(), lines.data(), nullptr);
            };
            fake_fail(f.fn, f.nth);
            if (go() == AIC_OK) rec("FAILED the failing call returned AIC_OK");
            rec("-- the same call again");
            if (go() != AIC_OK) rec("FAILED the call after the failure");
            if (d_rays) { (void)hipFree(d_rays); (void)hipFree(d_lines); }
            aic_destroy(c);
        }
    }
}

}  // namespace

int main() {
    rejections();
    launches();
    tables();
    pending_update();
    cursor_lines();
    failures();
    scenario("end");
    fake_reset();
    return 0;
}
