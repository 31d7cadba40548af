// light_report_check.cpp -- a stand-alone run of the light updater's changed-cube report (csrc/aic_light_report.h) on the CPU, to be built with
// -fsanitize=address,undefined (tests/test_light_report_cpu.py). The report is driven as the library drives it -- the updater's writes, a full relight,
// the caller's own texels, takes, re-reads of the mirror -- beside a brute-force model kept as two whole volumes: the baseline, and a flag per texel
// "the updater wrote it since the last take". Prints one line and returns 0 when all is well.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../all_is_cubes_amd/csrc/aic_light_report.h"

#define EXPECT(x)                                                    \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);      \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

namespace {

struct Model {
    std::vector<uint32_t> base;
    std::vector<bool> wrote;
    // a cube is reported if and only if the updater wrote it since the last take and its texel differs from the baseline; ascending
    std::vector<uint32_t> reported(const std::vector<uint32_t> &light) const {
        std::vector<uint32_t> out;
        for (size_t i = 0; i < light.size(); i++)
            if (wrote[i] && light[i] != base[i]) out.push_back((uint32_t)i);
        return out;
    }
    void afresh(const std::vector<uint32_t> &light) {
        base = light;
        wrote.assign(light.size(), false);
    }
};

struct Counts {
    uint64_t lists[2] = {0, 0}, cubes[2] = {0, 0};  // non-empty reports and their cubes, by mode (cand, cand_all)
    uint64_t kept[2] = {0, 0}, dropped[2] = {0, 0};  // pending reports a re-read kept / let go, by reread_own
    uint64_t own_only = 0;                           // pending reports that reread_own kept and a caller's re-read would have let go
    uint64_t afresh = 0;
};

void run(uint64_t seed, Counts *n) {
    std::mt19937_64 rng(seed);
    auto pick = [&](uint32_t m) { return (uint32_t)(rng() % m); };
    size_t cubes = 6 * 7 * 8;
    uint64_t serial = 1;
    std::vector<uint32_t> light(cubes);
    for (auto &t : light) t = pick(4);
    aic::LightReport report;
    Model model;
    report.report_reread(light, serial, {});  // the mirror as first read
    model.afresh(light);

    auto check = [&] {
        std::vector<uint32_t> got{12345u};  // (changed_list clears what it is given)
        report.changed_list(light, &got);
        const std::vector<uint32_t> want = model.reported(light);
        EXPECT(got == want);
        for (size_t k = 1; k < got.size(); k++) EXPECT(got[k - 1] < got[k]);
        if (!got.empty()) { n->lists[report.cand_all]++; n->cubes[report.cand_all] += got.size(); }
    };
    // The mirror is read again from the device, where `moved` texels hold other values: light_prepare's steps, and the rule restated on the whole volumes.
    auto reread = [&](bool own, uint64_t new_serial, size_t new_cubes, uint32_t moved) {
        std::vector<uint32_t> before;
        if (report.report_serial == new_serial && light.size() == new_cubes && (report.cand_all || !report.cand.empty())) before = light;
        const std::vector<uint32_t> old = light;
        light.resize(new_cubes);
        for (size_t i = old.size(); i < new_cubes; i++) light[i] = pick(4);
        for (uint32_t k = 0; k < moved && new_cubes; k++) light[pick((uint32_t)new_cubes)] = pick(4);
        if (own) report.reread_own = true;  // (as a failed update leaves it)
        report.report_reread(light, new_serial, before);
        EXPECT(!report.reread_own && report.report_serial == new_serial && !report.cand_all);
        if (new_serial != serial || new_cubes != cubes) {  // another space, or another size: the report starts afresh
            model.afresh(light);
            n->afresh++;
        } else {
            for (size_t i = 0; i < cubes; i++) {
                const bool pending = model.wrote[i] && old[i] != model.base[i];
                const bool keep_own = pending && light[i] != model.base[i];  // a failed update's re-read: every candidate the device still differs in
                const bool keep_caller = pending && light[i] == old[i];      // a caller's: only what the re-read did not move
                if (own && keep_own && !keep_caller) n->own_only++;
                const bool keep = own ? keep_own : keep_caller;
                if (pending) (keep ? n->kept : n->dropped)[own]++;
                if (!keep) { model.base[i] = light[i]; model.wrote[i] = false; }  // whoever replaced the texel owns it: the baseline follows
            }
        }
        serial = new_serial;
        cubes = new_cubes;
        check();
    };

    for (int step = 0; step < 6000; step++) {
        const uint32_t what = pick(100);
        if (what < 55) {  // the updater writes a texel (sometimes the value it held, sometimes the baseline's)
            const uint32_t i = pick((uint32_t)cubes);
            light[i] = pick(4);
            report.cand_add(i);
            model.wrote[i] = true;
        } else if (what < 65) {  // the caller replaces a texel: never reported
            const uint32_t i = pick((uint32_t)cubes);
            light[i] = pick(4);
            report.caller_wrote(light, i);
            model.base[i] = light[i];
            std::vector<uint32_t> now;
            report.changed_list(light, &now);
            EXPECT(!std::binary_search(now.begin(), now.end(), i));
            check();
        } else if (what < 80) {
            check();
        } else if (what < 86) {  // take: what was reported is handed over, the report is empty
            check();
            report.take(light);
            for (size_t i = 0; i < cubes; i++)
                if (model.wrote[i]) { model.base[i] = light[i]; model.wrote[i] = false; }
            std::vector<uint32_t> left{1u};
            report.changed_list(light, &left);
            EXPECT(left.empty() && report.cand.empty() && !report.cand_all);
        } else if (what < 89) {  // a full relight: every texel written
            for (auto &t : light) t = pick(4);
            report.cand_clear();
            report.cand_all = true;
            model.wrote.assign(cubes, true);
            check();
        } else if (what < 93) {
            reread(false, serial, cubes, pick(2) ? 40 : 0);
        } else if (what < 97) {
            reread(true, serial, cubes, pick(2) ? 40 : 0);
        } else if (what < 99) {
            reread(pick(2) != 0, serial + 1, cubes, 40);
        } else {
            reread(pick(2) != 0, serial, cubes == 336 ? 5 * 5 * 5 : 336, 0);
        }
    }
    check();
}

}  // namespace

int main() {
    Counts n;
    for (uint64_t seed = 1; seed <= 8; seed++) run(0x11907000u + seed, &n);
    // every case was met, in both modes and under both kinds of re-read
    EXPECT(n.lists[0] > 100 && n.lists[1] > 10 && n.cubes[1] > n.lists[1]);
    EXPECT(n.kept[0] > 100 && n.kept[1] > 100 && n.dropped[0] > 10 && n.dropped[1] > 10);
    EXPECT(n.own_only > 10);  // reread_own true and false differ
    EXPECT(n.afresh > 10);
    std::printf("light report ok: %llu reports in cand mode, %llu in cand_all mode, %llu kept by a re-read, %llu by reread_own alone\n", (unsigned long long)n.lists[0],
                (unsigned long long)n.lists[1], (unsigned long long)(n.kept[0] + n.kept[1]), (unsigned long long)n.own_only);
    return 0;
}
