// exposure_state_check.cpp -- a stand-alone run of the host-only half of automatic exposure (csrc/aic_exposure_state.cpp: aic_exposure_init,
// aic_exposure_rays, aic_exposure_advance), to be built with -fsanitize=address,undefined and run on the CPU (tests/test_exposure_cpu.py): every buffer is
// heap memory of exactly the size the header promises, so a read or write past it is reported. Prints one line and returns 0 when all is well.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "../../include/aic_hip.h"

#define EXPECT(x)                                                    \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);      \
            return 1;                                                \
        }                                                            \
    } while (0)

int main() {
    std::unique_ptr<aic_exposure_state> s(new aic_exposure_state);
    std::memset(s.get(), 0xff, sizeof(*s));
    EXPECT(aic_exposure_init(s.get()) == AIC_OK);
    EXPECT(s->luminance_sample_index == 0 && s->exposure_log == 0.0f && s->luminance_samples[0] == 1.0f && s->luminance_samples[99] == 1.0f);
    EXPECT(aic_exposure_init(nullptr) == AIC_ERR_INVALID);

    // rays: every count up to a few rings, first indices that wrap, into a buffer of exactly n * 6 doubles
    const double q[4] = {0.1, -0.7, 0.2, 0.68}, t[3] = {5.0, -3.0, 1e6};
    for (uint32_t n : {0u, 1u, 10u, 99u, 100u, 101u, 250u})
        for (uint32_t first : {0u, 95u, 99u, 100u, 4294967295u}) {
            std::unique_ptr<double[]> rays(new double[6 * (size_t)n + (n ? 0 : 1)]);
            EXPECT(aic_exposure_rays(q, t, first, n, n ? rays.get() : nullptr) == AIC_OK);
            for (uint32_t k = 0; k < n; k++) EXPECT(rays[6 * k] == 5.0 && rays[6 * k + 1] == -3.0 && rays[6 * k + 2] == 1e6 && std::isfinite(rays[6 * k + 5]));
        }
    EXPECT(aic_exposure_rays(nullptr, t, 0, 0, nullptr) == AIC_ERR_INVALID);
    EXPECT(aic_exposure_rays(q, t, 0, 1, nullptr) == AIC_ERR_INVALID);

    // advance: every n from 0 to 100 from every few starting indices, from a buffer of exactly n floats; specials among the samples
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    float e = 0.f;
    for (uint32_t n = 0; n <= 100; n++) {
        std::unique_ptr<float[]> smp(new float[n ? n : 1]);
        for (uint32_t k = 0; k < n; k++) smp[k] = 0.01f * (float)(k + n);
        if (n == 7) smp[3] = inf;
        if (n == 8) smp[0] = nan;
        if (n == 9) smp[8] = -inf;
        if (n == 50) for (uint32_t k = 0; k < n; k++) smp[k] = 0.f;
        EXPECT(aic_exposure_advance(s.get(), n, n ? smp.get() : nullptr, n % 3 == 0 ? 0.0 : 0.1, &e) == AIC_OK);
        EXPECT(s->luminance_sample_index < 100u && e > 0.f);
    }
    EXPECT(aic_exposure_advance(s.get(), 0, nullptr, 0.1, nullptr) == AIC_OK);
    EXPECT(aic_exposure_advance(s.get(), 101, &e, 0.1, nullptr) == AIC_ERR_INVALID);
    EXPECT(aic_exposure_advance(s.get(), 1, nullptr, 0.1, nullptr) == AIC_ERR_INVALID);
    EXPECT(aic_exposure_advance(nullptr, 0, nullptr, 0.1, nullptr) == AIC_ERR_INVALID);
    s->luminance_sample_index = 100;  // a state no call of the library leaves: rejected, not indexed with
    EXPECT(aic_exposure_advance(s.get(), 1, &e, 0.1, nullptr) == AIC_ERR_INVALID);
    std::printf("exposure state ok: exposure %.6f\n", e);
    return 0;
}
