// aic_light_report.h -- the changed-cube report of the light updater: what aic_light_changed_count / _take (include/aic_hip.h) answer from. `std` alone
// (no HIP include), so a stand-alone program can check the rule on the CPU against two whole volumes. A member of LightState (aic_light_host.h), whose
// mirror of the light volume every operation here takes as `light`.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

// (hidden: these inline members were internal to one unit before they had a header; a call that is not inlined stays a direct one, not one through the
// library's procedure linkage table, and the shared object exports none of them)
#pragma GCC visibility push(hidden)
namespace aic {

// `baseline` is the volume the report is measured against -- the mirror as first read, then following the caller's own texels and every take --, `cand`
// the cubes the updater wrote since (each once: `cand_bits`, a bit per cube; `cand_all`: fast = 1 wrote them all). A cube is reported iff it is a
// candidate and light[i] != baseline[i]: exact, and the apply loop gets no work per update -- deliver_changed() hands over what a batch changed, which
// it has sorted already.
struct LightReport {
    std::vector<uint32_t> baseline, cand;
    std::vector<uint64_t> cand_bits;
    bool cand_all = false;
    bool reread_own = false;          // the mirrors were marked stale by a failed update, not by the caller: the next re-read keeps every candidate
    uint64_t report_serial = ~0ull;   // Layer::upload_serial the baseline belongs to
    std::vector<uint32_t> published;  // while a submitted update runs: the answer for the published volume, taken at the submit (the worker owns the rest)
    void cand_add(uint32_t i) {
        if (cand_all) return;
        uint64_t &w = cand_bits[i >> 6];
        const uint64_t b = 1ull << (i & 63u);
        if (w & b) return;
        w |= b;
        cand.push_back(i);
    }
    void cand_clear() {
        for (uint32_t i : cand) cand_bits[i >> 6] = 0;
        if (cand_all) std::fill(cand_bits.begin(), cand_bits.end(), 0);
        cand.clear();
        cand_all = false;
    }
    // the caller replaced texel i of the mirror itself: the caller's own texel is never reported (aic_light_changed_count)
    void caller_wrote(const std::vector<uint32_t> &light, uint32_t i) {
        if (baseline.size() == light.size()) baseline[i] = light[i];
    }
    // the reported cubes, ascending
    void changed_list(const std::vector<uint32_t> &light, std::vector<uint32_t> *out) const {
        out->clear();
        if (cand_all) {
            for (size_t i = 0; i < light.size(); i++)
                if (light[i] != baseline[i]) out->push_back((uint32_t)i);
        } else {
            for (uint32_t i : cand)
                if (light[i] != baseline[i]) out->push_back(i);
            std::sort(out->begin(), out->end());
        }
    }
    // what was reported is taken: the baseline becomes the current volume
    void take(const std::vector<uint32_t> &light) {
        if (cand_all) baseline = light;
        else for (uint32_t i : cand) baseline[i] = light[i];
        cand_clear();
    }
    // The mirror `light` has just been read again from the device, `before` is what it held (empty: nothing was pending). A new space starts the
    // report afresh. Otherwise whoever replaced texels owns them -- the baseline follows, their candidates go --, and a candidate whose texel the
    // re-read did not move keeps its pending report.
    void report_reread(const std::vector<uint32_t> &light, uint64_t serial, const std::vector<uint32_t> &before) {
        const size_t n = light.size();
        const bool keep = report_serial == serial && baseline.size() == n && before.size() == n;
        std::vector<std::pair<uint32_t, uint32_t>> kept;  // (cube, its baseline)
        if (keep) {
            auto consider = [&](uint32_t i) {
                if (before[i] != baseline[i] && (reread_own ? light[i] != baseline[i] : light[i] == before[i])) kept.emplace_back(i, baseline[i]);
            };
            if (cand_all) for (size_t i = 0; i < n; i++) consider((uint32_t)i);
            else for (uint32_t i : cand) consider(i);
        }
        baseline = light;
        cand_bits.assign((n + 63) / 64, 0);
        cand.clear();
        cand_all = false;
        for (const auto &k : kept) { baseline[k.first] = k.second; cand_add(k.first); }
        reread_own = false;
        report_serial = serial;
    }
};

}  // namespace aic
#pragma GCC visibility pop
