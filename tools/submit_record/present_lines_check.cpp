// present_lines_check.cpp -- the host side of aic_present_split_lines (csrc/aic_split_ops.cpp) against the recording fake (fake_hip.cpp), as a program of its
// own: every rejection the header lists queues and allocates nothing, a call without lines records what aic_present_split records, the line scratch grows
// and is released, a failing runtime call leaves the context usable; and aic_cursor_wireframe's line counts. Exits 0 when every expectation holds; where it
// writes "# ... clear_keys V" into the record, the next launch_present_lines line must say the same (tests/test_present_lines_host_cpu.py compares).
// Host code only, so it can be built with sanitizers (build.sh ... present_lines_check.cpp -Xarch_host -fsanitize=address,undefined) and run anywhere.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "aic_ctx.h"
#include "aic_present_lines.h"
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

aic_present_desc desc(uint32_t sw, uint32_t sh, uint32_t ow, uint32_t oh, float bloom = 0.f, uint32_t flags = 0) {
    aic_present_desc d;
    std::memset(&d, 0, sizeof(d));
    d.src_width = sw; d.src_height = sh; d.out_width = ow; d.out_height = oh;
    d.bloom_intensity = bloom; d.maximum_intensity = 1.f; d.flags = flags;
    return d;
}

aic_lines_desc lines(const aic_line_vertex *v, uint32_t n, uint32_t flags = 0) {
    aic_lines_desc l;
    std::memset(&l, 0, sizeof(l));
    for (int i = 0; i < 4; i++) l.view_projection[5 * i] = 1.f;
    l.vertices = v; l.n_lines = n; l.flags = flags;
    return l;
}

}  // namespace

int main() {
    fake_reset();
    int st = 0;
    aic_ctx *c = aic_create(0, &st);
    EXPECT(c && st == AIC_OK);
    const uint32_t W = 40, H = 24, N = 28;
    void *src = dev(W * H * 12), *out = dev(4 * W * H * 8);
    std::vector<aic_line_vertex> host(2 * N);
    std::memset(host.data(), 0, host.size() * sizeof(aic_line_vertex));
    aic_line_vertex *on_device = (aic_line_vertex *)dev(2 * N * sizeof(aic_line_vertex) + 8);
    aic_present_info info;
    aic_lines_info li;
    const aic_lines_info zero = {};

    // ---- rejections: AIC_ERR_INVALID, nothing queued, nothing allocated, lines_info zeroed
    auto rejected = [&](const aic_present_desc *d, const aic_lines_desc *l, const void *s, void *o, int is_device = 1) {
        const int events = fake_calls("hipEventRecord"), allocs = fake_calls("hipMalloc"), copies = fake_calls("hipMemcpyAsync"), sets = fake_calls("hipMemsetAsync");
        std::memset(&li, 0xff, sizeof(li));
        EXPECT(aic_present_split_lines(c, d, l, s, o, is_device, &info, &li) == AIC_ERR_INVALID);
        EXPECT(fake_calls("hipEventRecord") == events && fake_calls("hipMalloc") == allocs && fake_calls("hipMemcpyAsync") == copies && fake_calls("hipMemsetAsync") == sets);
        EXPECT(std::strstr(aic_last_error(c), "aic_present_split") != nullptr);
        EXPECT(!std::memcmp(&li, &zero, sizeof(zero)));
        EXPECT(!c->lines_scratch.p);
    };
    aic_present_desc d = desc(W, H, W, H);
    aic_lines_desc l = lines(host.data(), N);
    EXPECT(aic_present_split_lines(nullptr, &d, &l, src, out, 1, &info, &li) == AIC_ERR_INVALID);
    rejected(nullptr, &l, src, out);
    rejected(&d, &l, nullptr, out);
    rejected(&d, &l, src, nullptr);
    rejected(&d, &l, src, nullptr, 0);
    l = lines(nullptr, N); rejected(&d, &l, src, out);
    l = lines(nullptr, N, AIC_LINES_DEVICE); rejected(&d, &l, src, out);
    l = lines(host.data(), AIC_LINES_MAX + 1u); rejected(&d, &l, src, out);
    for (uintptr_t off = 1; off < 4; off++) { l = lines((const aic_line_vertex *)((const char *)on_device + off), N, AIC_LINES_DEVICE); rejected(&d, &l, src, out); }
    for (uint32_t bad : {2u, 3u, 0x80000000u}) { l = lines(host.data(), N, bad); rejected(&d, &l, src, out); }
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()})
        for (int at : {0, 6, 15}) { l = lines(host.data(), N); l.view_projection[at] = bad; rejected(&d, &l, src, out); }
    l = lines(host.data(), N);
    rejected(&d, &l, (const char *)src + 4, out);
    rejected(&d, &l, src, (char *)out + 2);
    d = desc(W, H, W, H, 0.f, AIC_PRESENT_OUT_F16); rejected(&d, &l, src, (char *)out + 4);
    d = desc(W, H, W, H); rejected(&d, &l, src, (void *)src);
    rejected(&d, &l, src, (char *)src + W * H * 12 - 4);
    d = desc(65536, 1, W, H); rejected(&d, &l, src, out);
    d = desc(W, H, 1, 65536); rejected(&d, &l, src, out);
    d = desc(W, H, 65535, 32769); rejected(&d, &l, src, out);
    d = desc(0, H, W, H); rejected(&d, &l, src, out);
    d = desc(W, H, W, H, -0.125f); rejected(&d, &l, src, out);
    d = desc(W, H, W, H, std::numeric_limits<float>::quiet_NaN()); rejected(&d, &l, src, out);
    d = desc(W, H, W, H, std::numeric_limits<float>::infinity()); rejected(&d, &l, src, out);
    d = desc(W, H, W, H); d.maximum_intensity = -1.f; rejected(&d, &l, src, out);
    d = desc(W, H, W, H); d.tone_mapping = 2; rejected(&d, &l, src, out);
    d = desc(W, H, W, H, 0.f, 2u); rejected(&d, &l, src, out);
    // the lines' rejections hold with n_lines = 0 too, where the call would otherwise be aic_present_split's
    d = desc(W, H, W, H);
    l = lines(nullptr, 0, 2u); rejected(&d, &l, src, out);

    // ---- without lines the call is aic_present_split: the same runtime calls and launches, no line scratch
    auto calls = [&] {
        return std::vector<int>{fake_calls("hipEventRecord"), fake_calls("hipMalloc"), fake_calls("hipMemcpyAsync"), fake_calls("hipMemsetAsync"),
                                fake_calls("hipStreamSynchronize"), fake_calls("hipEventElapsedTime")};
    };
    auto delta = [&](const std::vector<int> &before) { std::vector<int> now = calls(); for (size_t i = 0; i < now.size(); i++) now[i] -= before[i]; return now; };
    for (float bloom : {0.f, 0.125f})
        for (uint32_t ow : {W, 2 * W}) {
            d = desc(W, H, ow, ow == W ? H : 2 * H, bloom);
            EXPECT(aic_present_split(c, &d, src, out, 1, &info) == AIC_OK);  // (first: whatever it allocates is there for both)
            std::vector<int> before = calls();
            EXPECT(aic_present_split(c, &d, src, out, 1, &info) == AIC_OK);
            const std::vector<int> plain = delta(before);
            for (int form = 0; form < 2; form++) {
                l = lines(host.data(), 0);
                before = calls();
                std::memset(&li, 0xff, sizeof(li));
                EXPECT(aic_present_split_lines(c, &d, form ? &l : nullptr, src, out, 1, &info, &li) == AIC_OK);
                EXPECT(delta(before) == plain);
                EXPECT(!std::memcmp(&li, &zero, sizeof(zero)) && info.bloomed == (bloom > 0.f ? 1u : 0u));
            }
        }
    EXPECT(!c->lines_scratch.p);

    // ---- with lines: the scratch is allocated on first use, grows when a call needs more, and only then
    d = desc(W, H, W, H);
    l = lines(host.data(), N);
    {
        const int allocs = fake_calls("hipMalloc");
        rec("# first use: clear_keys 1");
        EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
        EXPECT(fake_calls("hipMalloc") == allocs + 1 && c->lines_scratch.n == lines_layout(W, H, N).bytes);
        EXPECT(c->lines_keys_clean == (size_t)W * H);
        uint64_t bytes = 0;
        EXPECT(aic_present_lines_scratch(W, H, W, H, N, &bytes) == AIC_OK && bytes == c->lines_scratch.n);
    }
    {
        const int allocs = fake_calls("hipMalloc"), copies = fake_calls("hipMemcpyAsync");
        rec("# clean keys are not cleared again: clear_keys 0");
        EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
        EXPECT(fake_calls("hipMalloc") == allocs);
        EXPECT(fake_calls("hipMemcpyAsync") == copies + 2);  // the vertices in, the counters out
        l = lines(on_device, N, AIC_LINES_DEVICE);
        rec("# clear_keys 0");
        EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
        EXPECT(fake_calls("hipMemcpyAsync") == copies + 3);  // a device list is not staged
        EXPECT(fake_calls("hipMalloc") == allocs);
    }
    {
        const unsigned char *before = c->lines_scratch.p;
        const int allocs = fake_calls("hipMalloc");
        d = desc(W, H, 2 * W, 2 * H, 0.125f);
        l = lines(host.data(), N);
        rec("# a new allocation: clear_keys 1");
        EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
        EXPECT(c->lines_scratch.p != before && c->lines_scratch.n == lines_layout(2 * W, 2 * H, N).bytes && fake_calls("hipMalloc") == allocs + 1);
        EXPECT(info.bloomed == 1u);
        // a smaller window after a larger one: its scene lies where the larger one's keys were, so the larger clears again
        d = desc(W, H, W, H);
        rec("# clear_keys 0");
        EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
        EXPECT(c->lines_keys_clean == (size_t)W * H && fake_calls("hipMalloc") == allocs + 1);
        d = desc(W, H, 2 * W, 2 * H);
        rec("# clear_keys 1");
        EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
        EXPECT(c->lines_keys_clean == (size_t)4 * W * H);
    }
    // host target: the image is read back through the context's output buffer
    {
        std::vector<uint32_t> image(W * H);
        d = desc(W, H, W, H);
        const int copies = fake_calls("hipMemcpyAsync");
        rec("# clear_keys 0");
        EXPECT(aic_present_split_lines(c, &d, &l, src, image.data(), 0, &info, &li) == AIC_OK);
        EXPECT(fake_calls("hipMemcpyAsync") == copies + 3);
    }
    // an empty output with lines: AIC_OK, nothing queued
    {
        d = desc(W, H, 0, H);
        const int events = fake_calls("hipEventRecord");
        std::memset(&li, 0xff, sizeof(li));
        EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
        EXPECT(fake_calls("hipEventRecord") == events && !std::memcmp(&li, &zero, sizeof(zero)));
    }

    // ---- failing runtime calls are reported and leave the context usable; the keys are cleared again after a call that did not finish
    d = desc(W, H, W, H);
    fake_fail("hipStreamSynchronize", 0);
    rec("# clear_keys 0");
    EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_ERR_DEVICE);
    EXPECT(c->lines_keys_clean == 0);
    rec("# after a call that did not finish: clear_keys 1");
    EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
    EXPECT(c->lines_keys_clean == (size_t)W * H);
    fake_fail("hipMemcpyAsync", 0);
    EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_ERR_DEVICE);
    EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
    fake_fail("hipEventRecord", 1);
    EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_ERR_DEVICE);
    EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
    // the scratch cannot grow: the old one stays, and serves the next call that fits
    {
        const unsigned char *before = c->lines_scratch.p;
        d = desc(W, H, 8 * W, 8 * H);
        void *big = dev((size_t)64 * W * H * 4);
        fake_fail("hipMalloc", 0);
        EXPECT(aic_present_split_lines(c, &d, &l, src, big, 1, &info, &li) == AIC_ERR_OOM);
        EXPECT(c->lines_scratch.p == before);
        d = desc(W, H, W, H);
        EXPECT(aic_present_split_lines(c, &d, &l, src, out, 1, &info, &li) == AIC_OK);
        (void)hipFree(big);
    }
    EXPECT(aic_present_split(c, &d, src, out, 1, &info) == AIC_OK);

    // ---- aic_present_lines_scratch and aic_cursor_wireframe need no context
    {
        uint64_t bytes = 1;
        EXPECT(aic_present_lines_scratch(960, 540, 1920, 1080, 28, &bytes) == AIC_OK && bytes == 1920ull * 1080 * 16 + 32 + 28 * 56);
        EXPECT(aic_present_lines_scratch(W, H, W, H, 0, &bytes) == AIC_OK && bytes == 0);
        EXPECT(aic_present_lines_scratch(W, H, 0, H, 5, &bytes) == AIC_OK && bytes == 0);
        EXPECT(aic_present_lines_scratch(W, H, W, H, 5, nullptr) == AIC_OK);
        EXPECT(aic_present_lines_scratch(W, H, W, H, AIC_LINES_MAX + 1u, &bytes) == AIC_ERR_INVALID);
        EXPECT(aic_present_lines_scratch(65536, H, W, H, 5, &bytes) == AIC_ERR_INVALID);
        aic_cursor_desc cur;
        std::memset(&cur, 0, sizeof(cur));
        cur.voxel_size[0] = cur.voxel_size[1] = cur.voxel_size[2] = cur.resolution = 1;
        cur.distance_to_point = 1.0;
        aic_line_vertex v[2 * AIC_CURSOR_MAX_LINES + 1];
        std::memset(v, 0x5a, sizeof(v));
        const aic_line_vertex guard = v[2 * AIC_CURSOR_MAX_LINES];
        uint32_t n = 99;
        for (int entered = 0; entered < 7; entered++)
            for (int selected = 0; selected < 7; selected++) {
                cur.face_entered = entered; cur.face_selected = selected;
                EXPECT(aic_cursor_wireframe(&cur, v, &n) == AIC_OK && n == 12u + (selected ? 12u : 0u) + (entered ? 4u : 0u));
                for (uint32_t i = 0; i < 2 * n; i++) EXPECT(std::isfinite(v[i].position[0]) && v[i].color[3] == 1.f && v[i].color[0] == 0.f);
            }
        EXPECT(!std::memcmp(&guard, &v[2 * AIC_CURSOR_MAX_LINES], sizeof(guard)));
        EXPECT(aic_cursor_wireframe(nullptr, v, &n) == AIC_ERR_INVALID && aic_cursor_wireframe(&cur, nullptr, &n) == AIC_ERR_INVALID && aic_cursor_wireframe(&cur, v, nullptr) == AIC_ERR_INVALID);
        cur.face_entered = 7; EXPECT(aic_cursor_wireframe(&cur, v, &n) == AIC_ERR_INVALID && n == 0);
        cur.face_entered = -1; EXPECT(aic_cursor_wireframe(&cur, v, &n) == AIC_ERR_INVALID);
        cur.face_entered = 0; cur.resolution = 0; EXPECT(aic_cursor_wireframe(&cur, v, &n) == AIC_ERR_INVALID);
        cur.resolution = 1; cur.voxel_size[1] = -1; EXPECT(aic_cursor_wireframe(&cur, v, &n) == AIC_ERR_INVALID);
    }

    for (void *p : {src, out, (void *)on_device}) (void)hipFree(p);
    aic_destroy(c);  // releases the line scratch: a leak would show in fake_reset's line and under the sanitizer
    fake_reset();
    std::fprintf(stderr, "present_lines_check: %d of %d expectations failed\n", n_failed, n_checked);
    return n_failed ? 1 : 0;
}
