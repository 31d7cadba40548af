// srgb8_bucket_check.cpp -- the bucket table of sRGB8 (all_is_cubes_amd/csrc/aic_encode.h) against the thresholds it is made from, on the host:
// every bit pattern from 0x38000000 to 0x3f800000, and the values outside the table. Driven by tests/test_srgb8_bucket_host.py; prints one summary
// line and exits 0, or the first mismatches and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "aic_encode.h"

namespace {

float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// component_to_srgb8 (color.rs:1038-1054)
int reference_encoding(float c) {
    const float v = c <= 0.0031308f ? c * (323.f / 25.f) : (211.f * std::pow(c, 5.f / 12.f) - 11.f) / 200.f;
    const float r = std::round(v * 255.f);
    if (!(r > 0.f)) return 0;
    return r >= 255.f ? 255 : (int)r;
}

// thr[k]: the smallest f32 whose reference encoding is >= k -- bisection, then settled on the lowest float of the neighbourhood (libm's powf need not be
// monotone at the last bit), as the context makes them
void make_thresholds(float thr[256]) {
    thr[0] = 0.f;
    for (int k = 1; k < 256; k++) {
        uint32_t lo = 0u, hi = 0x40000000u;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (reference_encoding(from_bits(mid)) >= k) hi = mid; else lo = mid;
        }
        for (int back = 0; back < 8 && hi > 1u; back++) {
            const uint32_t probe = hi - 1u;
            bool lower_found = false;
            for (uint32_t d = 0; d < 8u && probe > d; d++)
                if (reference_encoding(from_bits(probe - d)) >= k) { hi = probe - d; lower_found = true; }
            if (!lower_found) break;
        }
        thr[k] = from_bits(hi);
    }
}

int n_bad = 0;
void expect(float c, uint32_t got, uint32_t want, const char *what) {
    if (got == want) return;
    if (n_bad++ < 10) {
        uint32_t b;
        std::memcpy(&b, &c, 4);
        std::printf("MISMATCH %s: pattern 0x%08x encodes to %u, thresholds say %u\n", what, b, got, want);
    }
}

}  // namespace

int main() {
    float thr[256];
    make_thresholds(thr);
    static uint32_t table[aic::kSrgbBucketWords];
    if (!aic::srgb8_bucket_build(thr, table)) {
        std::printf("srgb8_bucket_build refused the thresholds\n");
        return 1;
    }
    // no bucket holds two thresholds, every threshold lies in the table's range, and the spacing the table's layout rests on
    uint32_t min_gap = 0xffffffffu;
    for (int k = 1; k < 256; k++) {
        const uint32_t bk = aic::srgb8_float_bits(thr[k]);
        if ((bk >> 16) < aic::kSrgbBucketFirst || (bk >> 16) >= aic::kSrgbBucketLast) { std::printf("threshold %d outside the table\n", k); return 1; }
        if (k > 1) {
            const uint32_t bp = aic::srgb8_float_bits(thr[k - 1]);
            if ((bk >> 16) == (bp >> 16)) { std::printf("thresholds %d and %d share bucket 0x%04x\n", k - 1, k, bk >> 16); return 1; }
            if (bk - bp < min_gap) min_gap = bk - bp;
        }
    }
    if (min_gap <= 0x10000u) { std::printf("thresholds %u patterns apart\n", min_gap); return 1; }
    // every pattern of the range: the encoding is the number of thresholds <= c (the patterns ascend, so the count only moves up)
    uint32_t count = 0u;
    unsigned long long checked = 0ull;
    for (uint32_t b = 0x38000000u; b <= 0x3f800000u; b++) {
        const float c = from_bits(b);
        while (count < 255u && thr[count + 1u] <= c) count++;
        expect(c, aic::srgb8_bucket_channel(c, table), count, "range");
        checked++;
    }
    if (count != 255u) { std::printf("1.0 counts %u thresholds\n", count); return 1; }
    // outside it: zero, denormals and small normals (below thr[1]: 0), above 1 and +inf (255), NaN and negatives (0)
    auto by_count = [&](float c) { uint32_t n = 0u; for (int k = 1; k < 256; k++) n += thr[k] <= c ? 1u : 0u; return n; };
    const uint32_t small[] = {0x00000000u, 0x00000001u, 0x00000fffu, 0x007fffffu, 0x00800000u, 0x12345678u, 0x37ffffffu};
    for (uint32_t b : small) { expect(from_bits(b), aic::srgb8_bucket_channel(from_bits(b), table), 0u, "small"); if (by_count(from_bits(b)) != 0u) return 1; }
    const uint32_t large[] = {0x3f800001u, 0x3fc00000u, 0x40000000u, 0x7f7fffffu, 0x7f800000u};
    for (uint32_t b : large) { expect(from_bits(b), aic::srgb8_bucket_channel(from_bits(b), table), 255u, "large"); if (by_count(from_bits(b)) != 255u) return 1; }
    const uint32_t none[] = {0x7fc00000u, 0x7f800001u, 0xffc00000u, 0x80000000u, 0xbf800000u, 0xff800000u};
    for (uint32_t b : none) expect(from_bits(b), aic::srgb8_bucket_channel(from_bits(b), table), 0u, "not > 0");
    if (n_bad) return 1;
    std::printf("ok %llu patterns, %u entries, first bucket 0x%04x, smallest gap %u\n", checked, aic::kSrgbBucketWords, aic::srgb8_float_bits(thr[1]) >> 16, min_gap);
    return 0;
}
