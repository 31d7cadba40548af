// pick_check.cpp -- the host side of aic_pick_pixels (csrc/aic_split_ops.cpp) against the recording fake (fake_hip.cpp), as a program of its own: every
// rejection the header lists, the state aic_reproject_split keeps for it, and the calls a good pick makes. Exits 0 when every expectation holds.
// Host code only, so it can be built with sanitizers (build.sh ... pick_check.cpp -Xarch_host -fsanitize=address,undefined) and run anywhere.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "aic_ctx.h"
#include "aic_pick.h"
#include "record.h"

namespace {

int n_failed = 0, n_checked = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        n_checked++;                                                       \
        if (!(cond)) { n_failed++; std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

void *dev(size_t bytes) {
    void *p = nullptr;
    (void)hipMalloc(&p, bytes ? bytes : 1);
    return p;
}

// (driver.cpp's world: an 8 x 8 x 8 space of two blocks; no kernel ever runs)
aic_ctx *make_ctx() {
    int st = 0;
    aic_ctx *c = aic_create(0, &st);
    static const std::vector<uint16_t> cubes(512, 1);
    static const std::vector<uint8_t> light(512 * 4, 0);
    static const float palette[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.5f, 0.5f, 1.f, 0, 0, 0, 0};
    static const uint16_t voxels[1] = {0};
    aic_block_desc blocks[2];
    std::memset(blocks, 0, sizeof(blocks));
    for (int i = 0; i < 2; i++) { blocks[i].resolution = 1; blocks[i].pal_off = (uint32_t)i; blocks[i].pal_len = 1; blocks[i].flags = AIC_BLOCK_ONE | (i ? 0u : AIC_BLOCK_AIR); }
    aic_space_desc s;
    std::memset(&s, 0, sizeof(s));
    s.size[0] = s.size[1] = s.size[2] = 8;
    s.block_index = cubes.data(); s.light = light.data(); s.n_blocks = 2; s.blocks = blocks; s.voxels = voxels; s.n_voxels = 1; s.palette = palette; s.n_palette = 2;
    EXPECT(aic_upload_space(c, 0, &s) == AIC_OK);
    return c;
}

aic_pick_desc desc(uint32_t w, uint32_t h, uint32_t n, uint32_t max_unknown = 0, uint32_t flags = 0) {
    aic_pick_desc d;
    std::memset(&d, 0, sizeof(d));
    d.width = w; d.height = h; d.n = n; d.max_unknown = max_unknown; d.flags = flags;
    return d;
}

aic_reproject_desc reproject_desc(uint32_t w, uint32_t h) {
    aic_reproject_desc d;
    std::memset(&d, 0, sizeof(d));
    d.width = w; d.height = h;
    for (int i = 0; i < 4; i++) d.reprojection[5 * i] = 1.f;
    d.inverse_projection_zw[1] = d.inverse_projection_zw[2] = 1.f;
    return d;
}

}  // namespace

int main() {
    fake_reset();
    aic_ctx *c = make_ctx();
    const uint32_t W = 40, H = 24, N = 100;
    uint32_t *out = (uint32_t *)dev(N * 4), *order = (uint32_t *)dev(W * H * 4);
    void *src = dev(W * H * 12), *dst = dev(W * H * 12);
    aic_pick_info info;
    const aic_pick_info zero = {};
    auto rejected = [&](const aic_pick_desc *d, const uint32_t *ord, uint32_t *o, aic_pick_info *i) {
        const int launches = fake_calls("hipEventRecord"), allocs = fake_calls("hipMalloc");
        if (i) std::memset(i, 0xff, sizeof(*i));
        EXPECT(aic_pick_pixels(c, d, ord, o, i) == AIC_ERR_INVALID);
        EXPECT(fake_calls("hipEventRecord") == launches && fake_calls("hipMalloc") == allocs);  // nothing queued, nothing allocated
        EXPECT(std::strstr(aic_last_error(c), "aic_pick_pixels") != nullptr);
        if (i && d) EXPECT(!std::memcmp(i, &zero, sizeof(zero)));
    };
    aic_pick_desc d = desc(W, H, N);
    EXPECT(aic_pick_pixels(nullptr, &d, order, out, &info) == AIC_ERR_INVALID);
    rejected(nullptr, order, out, &info);
    rejected(&d, order, out, nullptr);
    rejected(&d, order, nullptr, &info);
    for (uintptr_t off = 1; off < 4; off++) {
        rejected(&d, order, (uint32_t *)((char *)out + off), &info);
        rejected(&d, (const uint32_t *)((const char *)order + off), out, &info);
    }
    d = desc(0, H, N); rejected(&d, order, out, &info);
    d = desc(W, 0, N); rejected(&d, order, out, &info);
    d = desc(65536, 1, N); rejected(&d, order, out, &info);
    d = desc(1, 65536, N); rejected(&d, order, out, &info);
    d = desc(W, H, 2048u * 65535u + 1u); rejected(&d, order, out, &info);
    d = desc(W, H, N, 0, 1); rejected(&d, order, out, &info);
    d = desc(W, H, N, 0, 0x80000000u); rejected(&d, order, out, &info);
    // max_unknown before any reprojection
    d = desc(W, H, N, N); rejected(&d, order, out, &info);
    EXPECT(!c->pick_scratch.p);
    // the pure picker needs none, allocates nothing and reads nothing back
    d = desc(W, H, N);
    d.cursor = (1ull << 40) + 3;
    {
        const int allocs = fake_calls("hipMalloc"), copies = fake_calls("hipMemcpyAsync");
        EXPECT(aic_pick_pixels(c, &d, order, out, &info) == AIC_OK);
        EXPECT(fake_calls("hipMalloc") == allocs && fake_calls("hipMemcpyAsync") == copies);
        EXPECT(info.n_unknown == 0 && info.n_from_unknown == 0 && info.n_from_order == N && info.next_cursor == d.cursor + N);
    }
    // n = 0 and an empty frame: AIC_OK, the info zeroed, nothing queued
    for (const aic_pick_desc &e : {desc(W, H, 0, 5), desc(0, 0, 0), desc(0, H, 0, 5)}) {
        const int launches = fake_calls("hipEventRecord");
        std::memset(&info, 0xff, sizeof(info));
        EXPECT(aic_pick_pixels(c, &e, nullptr, nullptr, &info) == AIC_OK);
        EXPECT(!std::memcmp(&info, &zero, sizeof(zero)) && fake_calls("hipEventRecord") == launches);
    }
    // a reprojection of W x H opens max_unknown for W x H alone
    aic_reproject_desc rd = reproject_desc(W, H);
    EXPECT(aic_reproject_split(c, &rd, src, dst, nullptr) == AIC_OK);
    EXPECT(c->reproject_valid_w == W && c->reproject_valid_h == H);
    d = desc(W, H, N, N);
    {
        const int copies = fake_calls("hipMemcpyAsync");
        EXPECT(aic_pick_pixels(c, &d, order, out, &info) == AIC_OK);
        EXPECT(fake_calls("hipMemcpyAsync") == copies + 1);  // the record, once
        EXPECT(c->pick_scratch.p && c->pick_scratch.n == pick_scratch_words((uint64_t)W * H));
    }
    d = desc(H, W, N, N); rejected(&d, order, out, &info);
    d = desc(W, H + 1, N, N); rejected(&d, order, out, &info);
    // a rejected reprojection and an empty one leave the state; one of another size replaces it
    EXPECT(aic_reproject_split(c, &rd, src, src, nullptr) == AIC_ERR_INVALID);
    rd = reproject_desc(0, H);
    EXPECT(aic_reproject_split(c, &rd, src, dst, nullptr) == AIC_OK);
    EXPECT(c->reproject_valid_w == W && c->reproject_valid_h == H);
    rd = reproject_desc(W / 2, H);
    EXPECT(aic_reproject_split(c, &rd, src, dst, nullptr) == AIC_OK);
    d = desc(W, H, N, N); rejected(&d, order, out, &info);
    d = desc(W / 2, H, N, N);
    EXPECT(aic_pick_pixels(c, &d, nullptr, out, &info) == AIC_OK);
    // a failed one that did not re-allocate leaves it; one that re-allocated its scratch and then failed has lost the splat image
    fake_fail("hipStreamSynchronize", 0);
    EXPECT(aic_reproject_split(c, &rd, src, dst, nullptr) == AIC_ERR_DEVICE);
    EXPECT(c->reproject_valid_w == W / 2 && c->reproject_valid_h == H);
    void *src2 = dev(4 * W * H * 12), *dst2 = dev(4 * W * H * 12);
    rd = reproject_desc(2 * W, 2 * H);
    fake_fail("hipStreamSynchronize", 0);
    EXPECT(aic_reproject_split(c, &rd, src2, dst2, nullptr) == AIC_ERR_DEVICE);
    EXPECT(c->reproject_valid_w == 0 && c->reproject_valid_h == 0);
    d = desc(W / 2, H, N, N); rejected(&d, nullptr, out, &info);
    // the scratch cannot grow: the old one and its splat image stay
    rd = reproject_desc(W, H);
    EXPECT(aic_reproject_split(c, &rd, src, dst, nullptr) == AIC_OK);
    rd = reproject_desc(8 * W, 8 * H);
    void *big = dev(64 * W * H * 12), *big2 = dev(64 * W * H * 12);
    fake_fail("hipMalloc", 0);
    EXPECT(aic_reproject_split(c, &rd, big, big2, nullptr) == AIC_ERR_OOM);
    EXPECT(c->reproject_valid_w == W && c->reproject_valid_h == H);
    // a failing pick-scratch allocation is reported and leaves the context usable
    d = desc(2 * W, 2 * H, N, N);
    rd = reproject_desc(2 * W, 2 * H);
    EXPECT(aic_reproject_split(c, &rd, src2, dst2, nullptr) == AIC_OK);
    c->pick_scratch.release();
    fake_fail("hipMalloc", 0);
    EXPECT(aic_pick_pixels(c, &d, nullptr, out, &info) == AIC_ERR_OOM);
    EXPECT(aic_pick_pixels(c, &d, nullptr, out, &info) == AIC_OK);
    // a frame still occupying slot 0
    aic_frame_desc f;
    std::memset(&f, 0, sizeof(f));
    f.width = 8; f.height = 8;
    for (int i = 0; i < 4; i++) f.world.inverse_projection_view[5 * i] = f.ui.inverse_projection_view[5 * i] = 1.0;
    f.world.exposure = f.ui.exposure = 1.f;
    void *frame_out = dev(8 * 8 * 4);
    EXPECT(aic_render_submit(c, &f, frame_out, 0) == AIC_OK);
    rejected(&d, nullptr, out, &info);
    aic_frame_info fi;
    EXPECT(aic_render_wait(c, 0, &fi) == AIC_OK);
    EXPECT(aic_pick_pixels(c, &d, nullptr, out, &info) == AIC_OK);
    for (void *p : {(void *)out, (void *)order, src, dst, src2, dst2, big, big2, frame_out}) (void)hipFree(p);
    aic_destroy(c);  // releases the pick scratch: a leak would show in fake_reset's line and under the sanitizer
    fake_reset();
    std::fprintf(stderr, "pick_check: %d of %d expectations failed\n", n_failed, n_checked);
    return n_failed ? 1 : 0;
}
