// aic_light_queue.h -- the light updater's queue and what it is keyed and fed by: the cube <-> index geometry of a space, the reference's hash of a
// cube, its hash table restated bucket for bucket, the update queue on top of it, and the priorities and texel words the queue's callers speak in.
// `std` alone (no HIP include): a plain C++17 compiler builds it, so a stand-alone program can drive it on the CPU beside the test oracle's own copy,
// which shares no text with this one (tests/test_light_queue_cpu.py). Used by aic_light_host.h (LightState) and through it by the light updater's units.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <utility>
#include <vector>

// (hidden: these inline members were internal to one unit before they had a header; a call that is not inlined stays a direct one, not one through the
// library's procedure linkage table, and the shared object exports none of them)
#pragma GCC visibility push(hidden)
namespace aic {

using I3h = std::array<int32_t, 3>;
inline I3h face_normal_h(int f) {  // 0 nx 1 ny 2 nz 3 px 4 py 5 pz
    I3h n = {0, 0, 0};
    n[(size_t)(f >= 3 ? f - 3 : f)] = f >= 3 ? 1 : -1;
    return n;
}

struct LightGeom {
    int32_t lo[3] = {0, 0, 0}, size[3] = {0, 0, 0};
    I3h cube_of(size_t idx) const {
        const size_t sz = (size_t)size[2], sy = (size_t)size[1];
        return I3h{lo[0] + (int32_t)(idx / (sy * sz)), lo[1] + (int32_t)((idx / sz) % sy), lo[2] + (int32_t)(idx % sz)};
    }
    bool index(const I3h &c, size_t *out) const {
        const uint32_t dx = (uint32_t)c[0] - (uint32_t)lo[0], dy = (uint32_t)c[1] - (uint32_t)lo[1], dz = (uint32_t)c[2] - (uint32_t)lo[2];
        if ((dx >= (uint32_t)size[0]) | (dy >= (uint32_t)size[1]) | (dz >= (uint32_t)size[2])) return false;
        *out = ((size_t)dx * (size_t)size[1] + dy) * (size_t)size[2] + dz;
        return true;
    }
};

// ------------------------------------------------------------------------------------
// queue.rs. The reference keeps one hashbrown::HashTable<Cube> per priority, hashed with rustc_hash::FxBuildHasher,
// and pops "an arbitrary element": the first full bucket in table order (queue.rs:236-243). The last unit of the
// converged 8-bit texels depends on that order, so it is reproduced: FxHasher 2.x (multiply by 0xf1357aea2e62a9c5,
// finish = rotate_left(26)) over Cube's Hash (x | y << 32 as one u64, then z), and hashbrown's open-addressing table
// (group-wise triangular probing, growth at 7/8 load in bucket order, in-place rehash, tombstones on erase).
// `W` is hashbrown's Group::WIDTH: 16 with SSE2 (x86-64), 8 elsewhere; 0 selects plain first-in-first-out.

inline uint64_t fx_hash_cube(const I3h &c) {
    const uint64_t K = 0xf1357aea2e62a9c5ull;
    uint64_t h = 0;
    h = (h + ((uint64_t)(uint32_t)c[0] ^ ((uint64_t)(uint32_t)c[1] << 32))) * K;
    h = (h + (uint64_t)(uint32_t)c[2]) * K;
    return (h << 26) | (h >> 38);
}

struct HbTable {
    static const uint8_t EMPTY = 0xff, DELETED = 0x80;
    int W = 16;
    std::vector<uint8_t> ctrl;      // buckets + W control bytes (the last W mirror the first W)
    std::vector<uint32_t> val;      // element per bucket
    std::vector<uint64_t> hashes;   // its hash
    size_t bucket_mask = 0, items = 0, growth_left = 0;
    bool singleton = true;          // the shared empty table of HashTable::new()

    size_t buckets() const { return bucket_mask + 1; }
    static size_t cap_of(size_t mask) { return mask < 8 ? mask : ((mask + 1) / 8) * 7; }
    static size_t capacity_to_buckets(size_t cap) {
        if (cap < 15) return cap < 4 ? 4 : (cap < 8 ? 8 : 16);
        size_t adjusted = cap * 8 / 7, p = 1;
        while (p < adjusted) p <<= 1;
        return p;
    }
    uint8_t ctrl_at(size_t i) const { return singleton ? EMPTY : ctrl[i]; }
    void set_ctrl(size_t index, uint8_t c) {
        const size_t index2 = ((index - (size_t)W) & bucket_mask) + (size_t)W;
        ctrl[index] = c;
        ctrl[index2] = c;
    }
    static uint8_t h2(uint64_t hash) { return (uint8_t)((hash >> 57) & 0x7f); }
    // first EMPTY/DELETED byte of the group at pos, or -1
    int first_special(size_t pos) const {
        for (int k = 0; k < W; k++) if (ctrl_at(pos + k) & 0x80) return k;
        return -1;
    }
    size_t find_insert_slot(uint64_t hash) const {
        size_t pos = (size_t)hash & bucket_mask, stride = 0;
        for (;;) {
            const int bit = first_special(pos);
            if (bit >= 0) {
                size_t index = (pos + (size_t)bit) & bucket_mask;
                if (!(ctrl_at(index) & 0x80)) index = (size_t)first_special(0);  // tables smaller than a group: fix_insert_slot
                return index;
            }
            stride += (size_t)W;
            pos = (pos + stride) & bucket_mask;
        }
    }
    void resize(size_t capacity) {
        HbTable n;
        n.W = W;
        n.singleton = false;
        const size_t nb = capacity_to_buckets(capacity);
        n.bucket_mask = nb - 1;
        n.ctrl.assign(nb + (size_t)W, EMPTY);
        n.val.assign(nb, 0);
        n.hashes.assign(nb, 0);
        n.items = items;
        n.growth_left = cap_of(n.bucket_mask) - items;
        if (!singleton)
            for (size_t i = 0; i < buckets(); i++)
                if (!(ctrl[i] & 0x80)) {
                    const size_t idx = n.find_insert_slot(hashes[i]);
                    n.set_ctrl(idx, h2(hashes[i]));
                    n.val[idx] = val[i];
                    n.hashes[idx] = hashes[i];
                }
        *this = std::move(n);
    }
    void rehash_in_place() {
        const size_t nb = buckets();
        // full -> DELETED, special -> EMPTY, then restore the mirror bytes
        for (size_t i = 0; i < nb; i++) ctrl[i] = (ctrl[i] & 0x80) ? EMPTY : DELETED;
        if (nb < (size_t)W) { for (size_t i = 0; i < nb; i++) ctrl[(size_t)W + i] = ctrl[i]; }
        else { for (size_t i = 0; i < (size_t)W; i++) ctrl[nb + i] = ctrl[i]; }
        for (size_t i = 0; i < nb; i++) {
            if (ctrl[i] != DELETED) continue;
            for (;;) {
                const uint64_t hash = hashes[i];
                const size_t new_i = find_insert_slot(hash);
                const size_t start = (size_t)hash & bucket_mask;
                if (((i - start) & bucket_mask) / (size_t)W == ((new_i - start) & bucket_mask) / (size_t)W) {
                    set_ctrl(i, h2(hash));
                    break;
                }
                const uint8_t prev = ctrl[new_i];
                set_ctrl(new_i, h2(hash));
                if (prev == EMPTY) {
                    set_ctrl(i, EMPTY);
                    val[new_i] = val[i]; hashes[new_i] = hashes[i];
                    break;
                }
                std::swap(val[new_i], val[i]);
                std::swap(hashes[new_i], hashes[i]);
            }
        }
        growth_left = cap_of(bucket_mask) - items;
    }
    void insert(uint64_t hash, uint32_t v) {
        size_t slot = find_insert_slot(hash);
        uint8_t old = ctrl_at(slot);
        if (growth_left == 0 && (old & 1)) {
            const size_t new_items = items + 1, full = singleton ? 0 : cap_of(bucket_mask);
            if (new_items <= full / 2) rehash_in_place();
            else resize(std::max(new_items, full + 1));
            slot = find_insert_slot(hash);
            old = ctrl[slot];
        }
        growth_left -= (old & 1) ? 1 : 0;
        set_ctrl(slot, h2(hash));
        val[slot] = v;
        hashes[slot] = hash;
        items++;
    }
    void erase(size_t index) {
        const size_t before = (index - (size_t)W) & bucket_mask;
        int lead = 0, trail = 0;  // empty_before.leading_zeros(), empty_after.trailing_zeros()
        for (int k = W - 1; k >= 0 && ctrl[before + (size_t)k] != EMPTY; k--) lead++;
        for (int k = 0; k < W && ctrl[index + (size_t)k] != EMPTY; k++) trail++;
        uint8_t c;
        if (lead + trail >= W) c = DELETED;
        else { growth_left++; c = EMPTY; }
        set_ctrl(index, c);
        items--;
    }
    bool find(uint64_t hash, uint32_t v, size_t *out) const {
        if (singleton) return false;
        size_t pos = (size_t)hash & bucket_mask, stride = 0;
        const uint8_t tag = h2(hash);
        for (;;) {
            bool any_empty = false;
            for (int k = 0; k < W; k++) {
                const uint8_t c = ctrl[pos + (size_t)k];
                if (c == tag) {
                    const size_t idx = (pos + (size_t)k) & bucket_mask;
                    if (val[idx] == v) { *out = idx; return true; }
                }
                if (c == EMPTY) any_empty = true;
            }
            if (any_empty) return false;
            stride += (size_t)W;
            pos = (pos + stride) & bucket_mask;
        }
    }
    bool first_full(size_t *out) const {  // RawIter order: ascending bucket index
        if (singleton) return false;
        for (size_t i = 0; i < buckets(); i++) if (!(ctrl[i] & 0x80)) { *out = i; return true; }
        return false;
    }
    void clear() {
        if (!singleton) std::fill(ctrl.begin(), ctrl.end(), EMPTY);
        items = 0;
        growth_left = singleton ? 0 : cap_of(bucket_mask);
    }
};

struct LightQueue {
    int hb_width;  // 0: first-in-first-out within a priority; 8 / 16: hashbrown table order (see above)
    // FIFO mode: priority -> queue of cube indices; by_cube: priority+1, or 0 = absent
    std::vector<std::deque<uint32_t>> by_priority;
    std::vector<HbTable> tables;
    std::vector<uint16_t> by_cube;
    const LightGeom *geom = nullptr;
    int highest = -1;
    size_t len = 0;
    LightQueue(size_t n_cubes, int width) : hb_width(width), by_priority(width ? 0 : 256), tables(width ? 256 : 0), by_cube(n_cubes, 0) {
        for (auto &t : tables) t.W = width;
    }
    void clear() {
        for (auto &q : by_priority) q.clear();
        for (auto &t : tables) t.clear();
        std::fill(by_cube.begin(), by_cube.end(), 0);
        highest = -1;
        len = 0;
    }
    uint64_t hash_of(uint32_t cube) const { return fx_hash_cube(geom->cube_of(cube)); }
    void insert(uint32_t cube, int priority) {  // queue.rs:264-290: keeps the higher priority
        const int old = (int)by_cube[cube] - 1;
        if (old >= priority) return;
        if (old < 0) len++;
        by_cube[cube] = (uint16_t)(priority + 1);
        if (hb_width) {
            const uint64_t h = hash_of(cube);
            if (old >= 0) {
                size_t idx = 0;
                if (tables[old].find(h, cube, &idx)) tables[old].erase(idx);
            }
            tables[priority].insert(h, cube);
        } else {
            by_priority[priority].push_back(cube);  // a stale entry of the old priority is skipped when popped
        }
        if (highest < priority) highest = priority;
    }
    bool remove(uint32_t cube) {
        if (by_cube[cube] == 0) return false;
        if (hb_width) {
            const int p = (int)by_cube[cube] - 1;
            size_t idx = 0;
            if (tables[p].find(hash_of(cube), cube, &idx)) tables[p].erase(idx);
        }
        by_cube[cube] = 0;
        len--;
        return true;
    }
    void settle() {
        while (highest >= 0) {
            if (hb_width) {
                if (tables[highest].items) return;
            } else {
                auto &q = by_priority[highest];
                while (!q.empty() && (int)by_cube[q.front()] - 1 != highest) q.pop_front();
                if (!q.empty()) return;
            }
            highest--;
        }
    }
    bool pop(uint32_t *cube) {
        settle();
        if (highest < 0) return false;
        if (hb_width) {
            size_t idx = 0;
            tables[highest].first_full(&idx);
            *cube = tables[highest].val[idx];
            tables[highest].erase(idx);
        } else {
            *cube = by_priority[highest].front();
            by_priority[highest].pop_front();
        }
        by_cube[*cube] = 0;
        len--;
        return true;
    }
    int peek_priority() { settle(); return highest < 0 ? 0 : highest; }
};
const int kPriorityNewlyVisible = 250, kPriorityUninit = 210, kPriorityEstimated = 200;  // queue.rs Priority::{NEWLY_VISIBLE, UNINIT, ESTIMATED}
inline int priority_from_difference(int d) { return d / 2 + 1; }

const uint32_t kTexelOpaque = 128u << 24, kTexelNoRays = 1u << 24, kTexelUninit = 0u;
// data.rs:186-211
inline int texel_difference(uint32_t a, uint32_t b) {
    int diff = 0;
    for (int s = 0; s < 24; s += 8) {
        const int x = (int)((a >> s) & 255u), y = (int)((b >> s) & 255u);
        diff = std::max(diff, x > y ? x - y : y - x);
    }
    if ((a >> 24) != (b >> 24)) diff = std::min(255, diff + 255 / 4);
    return diff;
}

}  // namespace aic
#pragma GCC visibility pop
