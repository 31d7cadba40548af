// aic_light.inc -- CPU ORACLE, part 2 (test infrastructure, NOT product code): the light updater.
// Included at the end of aic_oracle.cpp (it reuses that file's Raycaster, PackedLight, BlockSky,
// apply_transmittance and flat-scene accessors).
//
// Restates, sequentially and deterministically, SURVEY.md 8(f) N2:
//   all-is-cubes/src/space/light/chart/generator.rs      the ray-bundle tree ("chart")
//   all-is-cubes/src/space/light/updater.rs:181-537      compute_light, walk_ray_tree, apply_light_update,
//                                                        update_light_from_queue, fast_evaluate_light
//   all-is-cubes/src/space/light/queue.rs                LightUpdateQueue (priorities; see ORDER below)
//   all-is-cubes/src/space/light/data.rs:51-251          PackedLight::{some, guess, difference_priority}
//   all-is-cubes/src/block/eval/derived.rs:78-240        compute_derived: face colours, opacity, visibility
//   all-is-cubes/src/raytracer_components.rs:174-201     trace_for_eval
//   all-is-cubes/src/space.rs:1496-1540                  Mutation::{evaluate_light, fast_evaluate_light}
//
// ORDER. The reference pops "an arbitrary element" of a hashbrown table per priority level
// (queue.rs:236-243), so the order of equal-priority updates -- and with it the last unit of the converged
// 8-bit log-scale texels -- is unspecified there. This restatement pops first-in-first-out within a priority.
// The reference's own image tests hold every renderer to these scenes by thresholds
// (test-renderers/cases/src/lib.rs:501-512, 976-983, 1107-1135), and so do the tests of this oracle.
// With feature "auto-threads" (test-renderers' default, Cargo.toml:62-69) the reference computes batches of 32
// queue entries against the same light state before applying them (updater.rs:231-268): `batch` selects that.

namespace {

// ------------------------------------------------------------------------------------
// derived.rs: properties of an evaluated block that the light updater reads

struct Derived {
    Rgba color;            // derived.rs:34
    Rgba face_colors[6];   // nx ny nz px py pz (derived.rs:37)
    Rgb emission;          // derived.rs:44
    bool opaque[6];        // derived.rs:53
    bool visible;          // derived.rs:57
};

inline bool rgb_is_zero(const Rgb &c) { return c.r == 0.f && c.g == 0.f && c.b == 0.f; }

// voxel_storage.rs:731-733 get_opt_evoxel on the flat layout
inline bool block_get_evoxel(const orc_space *sp, const orc_block &b, const I3 &c, Evoxel *out) {
    if (b.is_one) {
        if (c[0] == 0 && c[1] == 0 && c[2] == 0) { *out = palette_entry(sp, b.pal_off); return true; }
        return false;
    }
    uint32_t dx = (uint32_t)c[0] - (uint32_t)b.vlo[0], dy = (uint32_t)c[1] - (uint32_t)b.vlo[1], dz = (uint32_t)c[2] - (uint32_t)b.vlo[2];
    if ((dx >= (uint32_t)b.vsize[0]) | (dy >= (uint32_t)b.vsize[1]) | (dz >= (uint32_t)b.vsize[2])) return false;
    size_t i = ((size_t)dx * b.vsize[1] + dy) * b.vsize[2] + dz;
    *out = palette_entry(sp, b.pal_off + sp->voxels[b.vox_off + i]);
    return true;
}

// derived.rs:241-292 VoxSum
struct VoxSum {
    f32 color_sum[3] = {0.f, 0.f, 0.f};
    f32 alpha_sum = 0.f;
    f32 emission_sum[3] = {0.f, 0.f, 0.f};
    size_t count = 0;
    void add(const Rgba &color, const f32 emission[3]) {  // AddAssign<EvalTrace>
        f32 alpha = color.a;
        color_sum[0] += color.r * alpha; color_sum[1] += color.g * alpha; color_sum[2] += color.b * alpha;
        alpha_sum += alpha;
        for (int i = 0; i < 3; i++) emission_sum[i] += emission[i];
        count += 1;
    }
    void add(const VoxSum &o) {
        for (int i = 0; i < 3; i++) { color_sum[i] += o.color_sum[i]; emission_sum[i] += o.emission_sum[i]; }
        alpha_sum += o.alpha_sum;
        count += o.count;
    }
    Rgba color(f32 surface_area) const {
        if (!(alpha_sum > 0.0f)) return Rgba{0.f, 0.f, 0.f, 0.f};
        return Rgba{ps_new_clamped(color_sum[0] / alpha_sum), ps_new_clamped(color_sum[1] / alpha_sum),
                    ps_new_clamped(color_sum[2] / alpha_sum), zo_new_clamped(alpha_sum / surface_area)};
    }
    Rgb emission(f32 surface_area) const {
        if (count == 0) return Rgb{0.f, 0.f, 0.f};
        return Rgb{ps_new_clamped(emission_sum[0] / surface_area), ps_new_clamped(emission_sum[1] / surface_area),
                   ps_new_clamped(emission_sum[2] / surface_area)};
    }
};

// raytracer_components.rs:174-201 trace_for_eval
inline void trace_for_eval(const orc_space *sp, const orc_block &b, I3 cube, int direction_face, int resolution, Rgba *out_color,
                           f32 out_emission[3]) {
    const f32 thickness = 1.0f / (f32)resolution;  // Resolution::recip_f32
    const I3 step = face_normal(direction_face);
    ColorBuf buf;
    f32 emission[3] = {0.f, 0.f, 0.f};
    Evoxel v;
    while (block_get_evoxel(sp, b, cube, &v)) {
        Rgba adjusted;
        f32 coeff;
        apply_transmittance(v.color, thickness, &adjusted, &coeff);
        const f32 c = ps_new_clamped(coeff);  // Rgb * f32 (color.rs:912-925)
        emission[0] += ps_mul(v.emission.r, c) * buf.transmittance;
        emission[1] += ps_mul(v.emission.g, c) * buf.transmittance;
        emission[2] += ps_mul(v.emission.b, c) * buf.transmittance;
        buf.add_color_internal(colorbuf_from_rgba(adjusted));
        if (buf.opaque()) break;
        for (int a = 0; a < 3; a++) cube[a] += step[a];
    }
    *out_color = rgba_from_colorbuf(buf);
    for (int i = 0; i < 3; i++) out_emission[i] = emission[i];
}

// derived.rs:78-240 compute_derived. (The per-face sums run over the same voxels as the reference's; the order
// of the f32 additions inside a face follows plain row-major order here, the reference's follows its rotated
// iteration -- a difference far below one PackedLight step.)
Derived compute_derived(const orc_space *sp, const orc_block &b) {
    Derived d;
    Evoxel one;
    if (block_single_voxel(sp, b, &one)) {
        d.color = one.color;
        for (int f = 0; f < 6; f++) { d.face_colors[f] = one.color; d.opaque[f] = one.color.a >= 1.0f; }  // fully_opaque
        d.emission = one.emission;
        d.visible = !(one.color.a <= 0.0f) || !rgb_is_zero(one.emission);
        return d;
    }
    const int res = b.resolution;
    const GridAab data = block_voxel_bounds(b);
    VoxSum all;
    for (int f = 0; f < 6; f++) {
        const int face = f + 1;                     // NX..PZ
        const int axis = f % 3;
        const bool positive = f >= 3;
        const int opposite = positive ? face - 3 : face + 3;
        const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
        VoxSum fs;
        if (b.vsize[0] > 0 && b.vsize[1] > 0 && b.vsize[2] > 0) {
            for (int v = data.lo[a2]; v < data.hi[a2]; v++) {
                for (int u = data.lo[a1]; u < data.hi[a1]; u++) {
                    I3 c;
                    c[axis] = positive ? data.hi[axis] - 1 : data.lo[axis];
                    c[a1] = u; c[a2] = v;
                    Rgba col;
                    f32 em[3];
                    trace_for_eval(sp, b, c, opposite, res, &col, em);
                    fs.add(col, em);
                }
            }
        }
        all.add(fs);
        d.face_colors[f] = fs.color((f32)res * (f32)res);
    }
    const f32 surface_area = (f32)(6.0 * (f64)res * (f64)res);
    d.color = all.color(surface_area);
    d.emission = all.emission(surface_area);
    // opaque: the layer of voxels just inside each face is present and fully opaque
    bool any_visible = false;
    for (int x = data.lo[0]; x < data.hi[0] && !any_visible; x++)
        for (int y = data.lo[1]; y < data.hi[1] && !any_visible; y++)
            for (int z = data.lo[2]; z < data.hi[2]; z++) {
                Evoxel v = Evoxel{Rgba{0, 0, 0, 0}, Rgb{0, 0, 0}};
                block_get_evoxel(sp, b, i3(x, y, z), &v);
                if (!evoxel_invisible(v)) { any_visible = true; break; }
            }
    d.visible = any_visible;
    for (int f = 0; f < 6; f++) {
        const int axis = f % 3;
        const bool positive = f >= 3;
        GridAab layer = {{{0, 0, 0}}, {{res, res, res}}};
        if (positive) layer.lo[axis] = res - 1; else layer.hi[axis] = 1;
        GridAab inter;
        bool covered = intersection_cubes(layer, data, &inter);
        if (covered) for (int a = 0; a < 3; a++) covered = covered && inter.lo[a] == layer.lo[a] && inter.hi[a] == layer.hi[a];
        bool all_opaque = covered;
        if (covered) {
            for (int x = layer.lo[0]; x < layer.hi[0] && all_opaque; x++)
                for (int y = layer.lo[1]; y < layer.hi[1] && all_opaque; y++)
                    for (int z = layer.lo[2]; z < layer.hi[2]; z++) {
                        Evoxel v = Evoxel{Rgba{0, 0, 0, 0}, Rgb{0, 0, 0}};
                        block_get_evoxel(sp, b, i3(x, y, z), &v);
                        if (!(v.color.a >= 1.0f)) { all_opaque = false; break; }
                    }
        }
        d.opaque[f] = all_opaque;
    }
    return d;
}

inline bool derived_all_opaque(const Derived &d) { return d.opaque[0] && d.opaque[1] && d.opaque[2] && d.opaque[3] && d.opaque[4] && d.opaque[5]; }
// updater.rs:1031-1033
inline bool opaque_for_light_computation(const Derived &d) { return derived_all_opaque(d) && rgb_is_zero(d.emission); }

// ------------------------------------------------------------------------------------
// chart/generator.rs

struct FaceMapF {
    f32 v[6];  // nx ny nz px py pz
    f32 sum() const { return (v[0] + v[3]) + (v[1] + v[4]) + (v[2] + v[5]); }  // face.rs:1046-1054
};
struct FlatNode {
    FaceMapF weight;
    uint32_t children[6];  // 0 = none
};

struct TreeNode {
    int8_t cube[3];
    int32_t children[6];
    FaceMapF weight;
};

struct Chart {
    std::vector<FlatNode> nodes;
};

Chart generate_chart() {
    std::vector<TreeNode> tree;
    TreeNode root;
    root.cube[0] = root.cube[1] = root.cube[2] = 0;
    for (int f = 0; f < 6; f++) { root.children[f] = -1; root.weight.v[f] = 0.f; }
    tree.push_back(root);
    const int STEP = 5;  // RAY_DIRECTION_STEP
    for (int x = -STEP; x <= STEP; x++)
        for (int y = -STEP; y <= STEP; y++)
            for (int z = -STEP; z <= STEP; z++) {
                if (!(std::abs(x) == STEP || std::abs(y) == STEP || std::abs(z) == STEP)) continue;
                // Vector3D::<f32>::normalize: self / self.length()
                const f32 fx = (f32)x, fy = (f32)y, fz = (f32)z;
                const f32 len = std::sqrt(fx * fx + fy * fy + fz * fz);
                const f32 d[3] = {fx / len, fy / len, fz / len};
                FaceMapF cos;
                for (int f = 0; f < 6; f++) {
                    const I3 n = face_normal(f + 1);
                    const f32 dotv = (f32)n[0] * d[0] + (f32)n[1] * d[1] + (f32)n[2] * d[2];
                    cos.v[f] = dotv > 0.0f ? dotv : 0.0f;  // f32::max(0.0)
                }
                // ray_to_steps: Ray::new([0.5; 3], direction as f64).cast().take_while(t <= 127)
                Raycaster rc = Raycaster::make(v3(0.5, 0.5, 0.5), v3((f64)d[0], (f64)d[1], (f64)d[2]));
                std::vector<I3> steps;
                RaycastStep st;
                while (rc.next(&st)) {
                    if (!(st.t_distance <= 127.0)) break;
                    steps.push_back(st.cube);
                }
                // tree.insert(&steps[1..], weight)
                int node = 0;
                for (int f = 0; f < 6; f++) tree[0].weight.v[f] += cos.v[f];
                for (size_t k = 1; k < steps.size(); k++) {
                    const I3 c = steps[k];
                    // Face::from_adjacency(parent cube, child cube)
                    int dir = -1;
                    for (int f = 0; f < 6; f++) {
                        const I3 n = face_normal(f + 1);
                        if (tree[node].cube[0] + n[0] == c[0] && tree[node].cube[1] + n[1] == c[1] && tree[node].cube[2] + n[2] == c[2]) dir = f;
                    }
                    if (dir < 0) break;  // unreachable: consecutive raycast steps are adjacent
                    int child = tree[node].children[dir];
                    if (child < 0) {
                        TreeNode n;
                        n.cube[0] = (int8_t)c[0]; n.cube[1] = (int8_t)c[1]; n.cube[2] = (int8_t)c[2];
                        for (int f = 0; f < 6; f++) { n.children[f] = -1; n.weight.v[f] = 0.f; }
                        child = (int)tree.size();
                        tree.push_back(n);
                        tree[node].children[dir] = child;
                    }
                    node = child;
                    for (int f = 0; f < 6; f++) tree[node].weight.v[f] += cos.v[f];
                }
            }
    // tree_to_flat: post-order numbering from the end, so that the root is node 0
    Chart chart;
    chart.nodes.resize(tree.size());
    std::vector<uint32_t> flat_index(tree.size(), 0);
    uint32_t next_index = (uint32_t)tree.size() - 1;
    // iterative post-order
    struct Frame { int node; int child; };
    std::vector<Frame> stack;
    stack.push_back(Frame{0, 0});
    while (!stack.empty()) {
        Frame &fr = stack.back();
        if (fr.child < 6) {
            int c = tree[fr.node].children[fr.child++];
            if (c >= 0) stack.push_back(Frame{c, 0});
            continue;
        }
        const int n = fr.node;
        stack.pop_back();
        const uint32_t this_index = next_index;
        if (this_index != 0) next_index -= 1;
        flat_index[n] = this_index;
        FlatNode fn;
        fn.weight = tree[n].weight;
        for (int f = 0; f < 6; f++) fn.children[f] = tree[n].children[f] >= 0 ? flat_index[tree[n].children[f]] : 0u;
        chart.nodes[this_index] = fn;
    }
    return chart;
}

const Chart &light_chart() {
    static const Chart chart = generate_chart();
    return chart;
}

struct LightSpaceGeom {
    GridAab bounds;
    int32_t size[3];
    I3 cube_of(size_t idx) const {
        const size_t sz = (size_t)size[2], sy = (size_t)size[1];
        return i3(bounds.lo[0] + (int32_t)(idx / (sy * sz)), bounds.lo[1] + (int32_t)((idx / sz) % sy), bounds.lo[2] + (int32_t)(idx % sz));
    }
};

// ------------------------------------------------------------------------------------
// queue.rs
//
// The reference's queue is 256 hashbrown::HashTable<Cube> (one per priority) keyed by rustc_hash::FxBuildHasher,
// and pop() takes "an arbitrary element": the first full bucket in table order (queue.rs:236-243). Neither crate is
// under /root/reference (hashbrown 0.17.0, rustc-hash 2.1.2 in Cargo.lock). Because the converged light depends on
// that order in its last 8-bit log-scale unit, and the reference's image goldens were produced with it, the order
// is restated here from the crates' published algorithms: FxHasher 2.x (multiply by 0xf1357aea2e62a9c5, finish =
// rotate_left(26)) over Cube's Hash impl (cube.rs:51-60: x | y << 32 as one u64, then z), and hashbrown's
// open-addressing table -- group-wise triangular probing, 7/8 load factor growth in bucket order, in-place rehash,
// tombstones on erase. `hb_width` is hashbrown's Group::WIDTH: 16 with SSE2 (x86-64), 8 on other targets; 0 selects a
// plain first-in-first-out order instead. PARITY: this ordering is pinned only through the lighting image goldens
// (tests/test_oracle_light.py); the light unit tests of the reference pass with any order.

inline uint64_t fx_hash_cube(const I3 &c) {
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
    const LightSpaceGeom *geom = nullptr;
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
const int PRIORITY_NEWLY_VISIBLE = 250, PRIORITY_UNINIT = 210, PRIORITY_ESTIMATED = 200;
inline int priority_from_difference(int d) { return d / 2 + 1; }

// ------------------------------------------------------------------------------------
// updater.rs

inline PackedLight pl_guess(Rgb v) { return PackedLight{packed_scalar_in(v.r), packed_scalar_in(v.g), packed_scalar_in(v.b), 0}; }
const PackedLight PL_OPAQUE = {0, 0, 0, 128};
const PackedLight PL_ONE = {144, 144, 144, 255};
inline bool pl_eq(PackedLight a, PackedLight b) { return a.r == b.r && a.g == b.g && a.b == b.b && a.status == b.status; }
// data.rs:186-211
inline int difference_priority(PackedLight a, PackedLight b) {
    auto ad = [](uint8_t x, uint8_t y) { return (int)(x > y ? x - y : y - x); };
    int diff = std::max(ad(a.r, b.r), std::max(ad(a.g, b.g), ad(a.b, b.b)));
    if (a.status != b.status) diff = std::min(255, diff + 255 / 4);
    return diff;
}

struct LightSpace {
    const orc_space *sp;
    GridAab bounds;
    std::vector<Derived> derived;  // per block index
    Derived air;
    std::vector<PackedLight> light;  // per cube, Z-major
    BlockSky block_sky;
    int maximum_distance;
    LightSpaceGeom geom;
    LightQueue queue;

    LightSpace(const orc_space *s, int max_dist, int hb_width = 0)
        : sp(s), maximum_distance(max_dist), queue((size_t)s->size[0] * s->size[1] * s->size[2], hb_width) {
        bounds.lo = i3(s->lo[0], s->lo[1], s->lo[2]);
        bounds.hi = i3(s->lo[0] + s->size[0], s->lo[1] + s->size[1], s->lo[2] + s->size[2]);
        geom.bounds = bounds;
        for (int a = 0; a < 3; a++) geom.size[a] = s->size[a];
        queue.geom = &geom;
        derived.resize(s->n_blocks);
        for (uint32_t i = 0; i < s->n_blocks; i++) derived[i] = compute_derived(s, s->blocks[i]);
        air.color = Rgba{0, 0, 0, 0};
        for (int f = 0; f < 6; f++) { air.face_colors[f] = air.color; air.opaque[f] = false; }
        air.emission = Rgb{0, 0, 0};
        air.visible = false;
        light.assign(queue.by_cube.size(), PL_UNINIT);
        block_sky = sky_for_blocks(*s);
    }
    bool index(const I3 &c, size_t *out) const {  // vol.rs:988-1023
        uint32_t dx = (uint32_t)c[0] - (uint32_t)bounds.lo[0], dy = (uint32_t)c[1] - (uint32_t)bounds.lo[1], dz = (uint32_t)c[2] - (uint32_t)bounds.lo[2];
        if ((dx >= (uint32_t)sp->size[0]) | (dy >= (uint32_t)sp->size[1]) | (dz >= (uint32_t)sp->size[2])) return false;
        *out = ((size_t)dx * sp->size[1] + dy) * sp->size[2] + dz;
        return true;
    }
    I3 cube_of(size_t idx) const { return geom.cube_of(idx); }
    const Derived &evaluated(const I3 &c) const {  // UpdateCtx::get_evaluated
        size_t i;
        if (!index(c, &i)) return air;
        return derived[sp->block_index[i]];
    }
    PackedLight get(const I3 &c) const {  // updater.rs:572-582 (LightPhysics::Rays)
        size_t i;
        if (index(c, &i)) return light[i];
        return light_outside(block_sky, bounds, c);
    }
    void light_needs_update(const I3 &c, int priority) {
        size_t i;
        if (index(c, &i)) queue.insert((uint32_t)i, priority);
    }
};

// updater.rs:693-741 LightBuffer + LightRayState
struct LightBuffer {
    f32 incoming[3] = {0.f, 0.f, 0.f};
    f32 total_ray_weight = 0.f;
    std::vector<I3> dependencies;
    size_t cost = 0;
    f64 maximum_distance_squared;
};
struct LightRayState {
    f32 alpha;
    FaceMapF direction_weights;
};

inline void add_weighted_light(LightBuffer &b, const f32 color[3], f32 weight) {  // updater.rs:934-937
    const f32 w = ps_new_clamped(weight);
    for (int i = 0; i < 3; i++) b.incoming[i] += ps_mul(color[i], w);
    b.total_ray_weight += weight;
}

// updater.rs:899-927
void end_of_ray(LightBuffer &b, const LightRayState &rs, const BlockSky &sky, f32 ray_bundle_weight, const FaceMapF &chart_weights) {
    if (ray_bundle_weight > 0.f) {
        // (FaceMap::from_fn(|face| block_sky.in_direction(face).value() * chart_weights[face])).sum() * chart_weights.sum().recip()
        f32 per_face[6][3];
        for (int f = 0; f < 6; f++) {
            const Rgb v = pl_value(sky.faces[f]);
            const f32 w = ps_new_clamped(chart_weights.v[f]);
            per_face[f][0] = ps_mul(v.r, w); per_face[f][1] = ps_mul(v.g, w); per_face[f][2] = ps_mul(v.b, w);
        }
        const f32 recip = ps_new_clamped(1.0f / chart_weights.sum());
        f32 sky_light[3];
        for (int i = 0; i < 3; i++) {
            const f32 s = (per_face[0][i] + per_face[3][i]) + (per_face[1][i] + per_face[4][i]) + (per_face[2][i] + per_face[5][i]);
            sky_light[i] = ps_mul(ps_mul(s, recip), ps_new_clamped(rs.alpha));
        }
        add_weighted_light(b, sky_light, ray_bundle_weight);
    }
}

// updater.rs:770-895 LightBuffer::traverse
void traverse(LightBuffer &b, LightRayState &rs, const LightSpace &ls, const I3 &hit_cube, int hit_face, const Derived &ev_hit,
              bool *ahead_has, PackedLight *ahead, bool behind_has, PackedLight behind, const FaceMapF &chart_weights) {
    if (!ev_hit.visible) return;  // visible_or_animated (no animation hints in the flat scene)
    const bool hit_opaque_face = hit_face == WITHIN ? derived_all_opaque(ev_hit) : ev_hit.opaque[hit_face - 1];
    if (hit_opaque_face && hit_face == WITHIN) {
        for (int f = 0; f < 6; f++) rs.direction_weights.v[f] = 0.f;
        rs.alpha = 0.f;
        return;
    }
    Rgba sc = hit_face == WITHIN ? ev_hit.color : ev_hit.face_colors[hit_face - 1];  // face7_color
    sc.r = sc.r > 1.f ? 1.f : sc.r; sc.g = sc.g > 1.f ? 1.f : sc.g; sc.b = sc.b > 1.f ? 1.f : sc.b;  // Rgba::clamp (color.rs:692-697)
    const f32 hit_alpha = sc.a;
    FaceMapF wprod;
    for (int f = 0; f < 6; f++) wprod.v[f] = rs.direction_weights.v[f] * chart_weights.v[f];
    if (hit_alpha > 0.f && hit_face != WITHIN) {
        const I3 n = face_normal(hit_face);
        const I3 light_cube = i3(hit_cube[0] + n[0], hit_cube[1] + n[1], hit_cube[2] + n[2]);  // CubeFace::adjacent
        const PackedLight stored = behind_has ? behind : ls.get(light_cube);
        const Rgb sv = pl_value(stored);
        // light_emission + hit_surface_color.reflect(stored.value()) ; reflect = rgb * illumination * alpha
        const f32 from_face[3] = {ev_hit.emission.r + ps_mul(ps_mul(sc.r, sv.r), sc.a), ev_hit.emission.g + ps_mul(ps_mul(sc.g, sv.g), sc.a),
                                  ev_hit.emission.b + ps_mul(ps_mul(sc.b, sv.b), sc.a)};
        const f32 a = ps_new_clamped(rs.alpha), w = ps_new_clamped(wprod.sum());
        for (int i = 0; i < 3; i++) b.incoming[i] += ps_mul(ps_mul(from_face[i], a), w);
        b.cost += 10;
        if (b.dependencies.empty() || !(b.dependencies.back()[0] == light_cube[0] && b.dependencies.back()[1] == light_cube[1] && b.dependencies.back()[2] == light_cube[2]))
            b.dependencies.push_back(light_cube);
        if (hit_opaque_face) rs.alpha = 0.f;
        else rs.alpha *= 1.0f - hit_alpha;
    }
    if (hit_alpha < 1.0f) {
        Rgb stored_light = Rgb{0.f, 0.f, 0.f};
        if (hit_face != WITHIN) {
            if (!*ahead_has) { *ahead = ls.get(hit_cube); *ahead_has = true; }
            stored_light = pl_value(*ahead);
        }
        const f32 ha = hit_alpha;
        const f32 from_block[3] = {ev_hit.emission.r + ps_mul(stored_light.r, ha), ev_hit.emission.g + ps_mul(stored_light.g, ha),
                                   ev_hit.emission.b + ps_mul(stored_light.b, ha)};
        const f32 a = ps_new_clamped(rs.alpha), w = ps_new_clamped(wprod.sum());
        for (int i = 0; i < 3; i++) b.incoming[i] += ps_mul(ps_mul(from_block[i], a), w);
        b.cost += 10;
        b.dependencies.push_back(hit_cube);
        rs.alpha *= 1.0f - hit_alpha;
    }
}

// updater.rs:427-530
f32 walk_ray_tree(const LightSpace &ls, LightBuffer &b, const I3 &origin_cube, const I3 &cube_entered, int face_entered,
                  const Chart &chart, size_t node_index, bool prev_has, PackedLight prev_light, LightRayState rs) {
    const FlatNode &node = chart.nodes[node_index];
    FaceMapF prod;
    for (int f = 0; f < 6; f++) prod.v[f] = node.weight.v[f] * rs.direction_weights.v[f];
    const f32 ray_bundle_weight = prod.sum();
    if (ray_bundle_weight <= 0.0f) return ray_bundle_weight;
    // (cube_entered.center() - origin_cube.center()).square_length()
    f64 d2 = 0.0;
    {
        const f64 dx = ((f64)cube_entered[0] + 0.5) - ((f64)origin_cube[0] + 0.5), dy = ((f64)cube_entered[1] + 0.5) - ((f64)origin_cube[1] + 0.5),
                  dz = ((f64)cube_entered[2] + 0.5) - ((f64)origin_cube[2] + 0.5);
        d2 = dx * dx + dy * dy + dz * dz;
    }
    if (d2 > b.maximum_distance_squared) {
        end_of_ray(b, rs, ls.block_sky, ray_bundle_weight, node.weight);
        return ray_bundle_weight;
    }
    b.cost += 1;
    size_t entered_index;
    if (!ls.index(cube_entered, &entered_index)) {
        end_of_ray(b, rs, ls.block_sky, ray_bundle_weight, node.weight);
        return ray_bundle_weight;
    }
    bool ahead_has = false;
    PackedLight ahead = PL_UNINIT;
    traverse(b, rs, ls, cube_entered, face_entered, ls.derived[ls.sp->block_index[entered_index]], &ahead_has, &ahead, prev_has, prev_light, node.weight);
    if (!(rs.alpha > 0.0f)) {
        end_of_ray(b, rs, ls.block_sky, ray_bundle_weight, node.weight);
        return ray_bundle_weight;
    }
    f32 child_weight_sum = 0.0f;
    for (int f = 0; f < 6; f++) {
        const uint32_t child = node.children[f];
        if (child != 0u) {
            const I3 n = face_normal(f + 1);
            const int opposite = f >= 3 ? f + 1 - 3 : f + 1 + 3;
            child_weight_sum += walk_ray_tree(ls, b, origin_cube, i3(cube_entered[0] + n[0], cube_entered[1] + n[1], cube_entered[2] + n[2]), opposite,
                                              chart, child, ahead_has, ahead, rs);
        }
    }
    const f32 rest = ray_bundle_weight - child_weight_sum;
    end_of_ray(b, rs, ls.block_sky, rest > 0.0f ? rest : 0.0f, node.weight);
    return ray_bundle_weight;
}

struct ComputedLight {
    I3 cube;
    PackedLight light;
    std::vector<I3> dependencies;
    size_t cost;
};

// updater.rs:668-690
FaceMapF directions_to_seek_light(const Derived &origin, const Derived *const nb[6]) {
    FaceMapF w;
    if (origin.visible) {
        for (int f = 0; f < 6; f++) w.v[f] = 1.0f;
    } else {
        for (int f = 0; f < 6; f++) {
            const int opp = f >= 3 ? f - 3 : f + 3;
            w.v[f] = (nb[opp]->visible || !rgb_is_zero(nb[f]->emission)) ? 1.0f : 0.0f;
        }
    }
    return w;
}

// updater.rs:368-417
ComputedLight compute_light(const LightSpace &ls, const I3 &cube) {
    LightBuffer b;
    b.maximum_distance_squared = (f64)ls.maximum_distance * (f64)ls.maximum_distance;
    const Derived &ev_origin = ls.evaluated(cube);
    const bool origin_is_opaque = derived_all_opaque(ev_origin);
    if (origin_is_opaque) {
        if (!opaque_for_light_computation(ev_origin)) {
            const f32 e[3] = {ev_origin.emission.r, ev_origin.emission.g, ev_origin.emission.b};
            add_weighted_light(b, e, 1.0f);
        }
    } else {
        const Derived *nb[6];
        for (int f = 0; f < 6; f++) {
            const I3 n = face_normal(f + 1);
            nb[f] = &ls.evaluated(i3(cube[0] + n[0], cube[1] + n[1], cube[2] + n[2]));
        }
        LightRayState rs;
        rs.alpha = 1.0f;
        rs.direction_weights = directions_to_seek_light(ev_origin, nb);
        walk_ray_tree(ls, b, cube, cube, WITHIN, light_chart(), 0, false, PL_UNINIT, rs);
    }
    // LightBuffer::finish (updater.rs:940-952)
    ComputedLight out;
    out.cube = cube;
    const f32 scale = ps_new_clamped(1.0f / std::max(b.total_ray_weight, 1.0f));
    if (b.total_ray_weight > 0.0f) out.light = pl_some(Rgb{ps_mul(b.incoming[0], scale), ps_mul(b.incoming[1], scale), ps_mul(b.incoming[2], scale)});
    else if (origin_is_opaque) out.light = PL_OPAQUE;
    else out.light = PL_NO_RAYS;
    out.dependencies = std::move(b.dependencies);
    out.cost = b.cost;
    return out;
}

// updater.rs:295-362; returns the difference
int apply_light_update(LightSpace &ls, const ComputedLight &c, std::vector<uint32_t> *changed) {
    size_t ci = 0;
    ls.index(c.cube, &ci);
    const PackedLight old = ls.light[ci];
    const int diff = difference_priority(c.light, old);
    if (diff > 0) {
        ls.light[ci] = c.light;
        if (changed) changed->push_back((uint32_t)ci);
        for (int f = 0; f < 6; f++) {
            const I3 n = face_normal(f + 1);
            const I3 nc = i3(c.cube[0] + n[0], c.cube[1] + n[1], c.cube[2] + n[2]);
            size_t ni;
            if (!ls.index(nc, &ni)) continue;
            PackedLight &nl = ls.light[ni];
            if (nl.status == 0) {  // Uninitialized
                if (pl_eq(nl, c.light)) continue;
                if (derived_all_opaque(ls.evaluated(nc))) continue;
                nl = pl_guess(pl_value(c.light));
                if (changed) changed->push_back((uint32_t)ni);
            }
        }
        if (diff > 1) {
            const int priority = priority_from_difference(diff);
            for (const I3 &dep : c.dependencies) ls.light_needs_update(dep, priority);
        }
    }
    return diff;
}

// updater.rs:537-581 fast_evaluate_light
void fast_evaluate_light(LightSpace &ls) {
    ls.queue.clear();
    for (int x = ls.bounds.lo[0]; x < ls.bounds.hi[0]; x++)
        for (int z = ls.bounds.lo[2]; z < ls.bounds.hi[2]; z++) {
            bool covered = false;
            for (int y = ls.bounds.hi[1] - 1; y >= ls.bounds.lo[1]; y--) {
                const I3 cube = i3(x, y, z);
                size_t idx = 0;
                ls.index(cube, &idx);
                const Derived &ev = ls.derived[ls.sp->block_index[idx]];
                PackedLight v;
                if (opaque_for_light_computation(ev)) {
                    covered = true;
                    v = PL_OPAQUE;
                } else {
                    bool any = ev.visible;
                    for (int f = 0; f < 6 && !any; f++) {
                        const I3 n = face_normal(f + 1);
                        any = ls.evaluated(i3(x + n[0], y + n[1], z + n[2])).visible;
                    }
                    if (any) {
                        ls.queue.insert((uint32_t)idx, PRIORITY_ESTIMATED);
                        v = covered ? PL_UNINIT : ls.block_sky.faces[4];  // in_direction(Face::PY)
                    } else {
                        v = PL_NO_RAYS;
                    }
                }
                ls.light[idx] = v;
            }
        }
}

// update_light_from_queue without a time budget (updater.rs:181-292) until the queue's highest priority is at
// most from_difference(epsilon) -- what Mutation::evaluate_light loops for (space.rs:1496-1527).
// A batch's compute_light calls are independent (they read one light state) and the reference runs them on its rayon pool
// (updater.rs:231-247 `data.par_iter_mut()`): with g_light_threads > 1 they run on that many threads here, for the CPU baseline.
// The results, and the order they are applied in, do not depend on the thread count.
int g_light_threads = 1;

// a small persistent pool: spawning threads per batch would cost more than a batch of 32 walks does
struct LightPool {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_start, cv_done;
    uint64_t generation = 0;
    int running = 0;
    bool quit = false;
    const LightSpace *ls = nullptr;
    const std::vector<uint32_t> *cubes = nullptr;
    std::vector<ComputedLight> *out = nullptr;
    std::atomic<size_t> next{0};
    void work() {
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= cubes->size()) return;
            (*out)[k] = compute_light(*ls, ls->cube_of((*cubes)[k]));
        }
    }
    void loop(uint64_t seen) {  // `seen`: the generation at the time the worker was created
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m);
                cv_start.wait(lk, [&] { return quit || generation != seen; });
                if (quit) return;
                seen = generation;
            }
            work();
            {
                std::lock_guard<std::mutex> lk(m);
                if (--running == 0) cv_done.notify_one();
            }
        }
    }
    void resize(int n_workers) {
        if ((int)threads.size() == n_workers) return;
        stop();
        quit = false;
        const uint64_t now = generation;
        for (int t = 0; t < n_workers; t++) threads.emplace_back([this, now] { loop(now); });
    }
    void stop() {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv_start.notify_all();
        for (auto &t : threads) t.join();
        threads.clear();
    }
    void run(const LightSpace &l, const std::vector<uint32_t> &c, std::vector<ComputedLight> &o) {
        ls = &l; cubes = &c; out = &o;
        next.store(0);
        {
            std::lock_guard<std::mutex> lk(m);
            running = (int)threads.size();
            generation++;
        }
        cv_start.notify_all();
        work();
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return running == 0; });
    }
    ~LightPool() { stop(); }
};

void compute_batch(const LightSpace &ls, const std::vector<uint32_t> &cubes, std::vector<ComputedLight> &out) {
    out.resize(cubes.size());
    const int nt = std::min<int>(g_light_threads, (int)cubes.size());
    if (nt <= 1) {
        for (size_t k = 0; k < cubes.size(); k++) out[k] = compute_light(ls, ls.cube_of(cubes[k]));
        return;
    }
    static LightPool pool;
    pool.resize(g_light_threads - 1);
    pool.run(ls, cubes, out);
}

// Returns the update count; `cost` (if non-null) gets the sum of their ComputedLight::cost.
uint64_t evaluate_light(LightSpace &ls, int epsilon, int batch, uint64_t max_updates, uint64_t *cost = nullptr) {
    const int eps = priority_from_difference(epsilon);
    uint64_t total = 0, cost_sum = 0;
    std::vector<ComputedLight> out;
    std::vector<uint32_t> cubes;
    while (total < max_updates) {
        if (ls.queue.peek_priority() <= eps) break;
        cubes.clear();
        for (int k = 0; k < (batch < 1 ? 1 : batch); k++) {
            uint32_t idx;
            if (!ls.queue.pop(&idx)) break;
            cubes.push_back(idx);
        }
        if (cubes.empty()) break;
        compute_batch(ls, cubes, out);
        for (const ComputedLight &c : out) {
            apply_light_update(ls, c, nullptr);
            cost_sum += c.cost;
            total++;
        }
    }
    if (cost) *cost = cost_sum;
    return total;
}

}  // namespace

extern "C" {

// threads for the compute_light calls of a batch (the CPU baseline's stand-in for the reference's rayon pool); default 1
void orc_set_light_threads(int32_t n) { g_light_threads = n < 1 ? 1 : n; }
// Experiment switch (tests/fog_experiments.py): before fast_evaluate_light, replay what building the scene cube by cube leaves in
// the update queue -- every non-air cube through modified_cube_needs_update (updater.rs:135-173: Priority::NEWLY_VISIBLE for the
// cube unless it is opaque for light, and for every neighbour that is not opaque towards it) -- so that the queue's tables have
// the capacity they would have grown to when fast_evaluate_light clears them (queue.rs:287-298; HbTable::clear keeps its buckets).
static int g_light_build_history = 0;
void orc_set_light_build_history(int32_t on) { g_light_build_history = on; }

}  // extern "C"

namespace {

// modified_cube_needs_update (updater.rs:135-173) for a cube whose block has just been set: an opaque-for-light cube
// takes PackedLight::OPAQUE and leaves the queue, any other is queued at Priority::NEWLY_VISIBLE, and so is every
// neighbour whose face towards the cube is not opaque.
void modified_cube_needs_update(LightSpace &ls, const I3 &cube) {
    size_t idx;
    if (!ls.index(cube, &idx)) return;
    if (opaque_for_light_computation(ls.derived[ls.sp->block_index[idx]])) {
        ls.light[idx] = PL_OPAQUE;
        ls.queue.remove((uint32_t)idx);
    } else {
        ls.queue.insert((uint32_t)idx, PRIORITY_NEWLY_VISIBLE);
    }
    for (int f = 1; f <= 6; f++) {
        const I3 n = face_normal(f);
        const I3 nb = i3(cube[0] + n[0], cube[1] + n[1], cube[2] + n[2]);
        size_t ni;
        if (!ls.index(nb, &ni)) continue;
        const int opposite = f > 3 ? f - 3 : f + 3;
        if (!ls.derived[ls.sp->block_index[ni]].opaque[opposite - 1]) ls.queue.insert((uint32_t)ni, PRIORITY_NEWLY_VISIBLE);
    }
}

// The queue that building the space cube by cube leaves (see orc_set_light_build_history): every visible cube in
// GridAab::interior_iter order; the light texels it writes are overwritten by fast_evaluate_light.
void replay_build_history(LightSpace &ls) {
    const int32_t *lo = ls.sp->lo, *sz = ls.sp->size;
    for (int32_t x = 0; x < sz[0]; x++) for (int32_t y = 0; y < sz[1]; y++) for (int32_t z = 0; z < sz[2]; z++) {
        const I3 cube = i3(lo[0] + x, lo[1] + y, lo[2] + z);
        size_t idx;
        if (!ls.index(cube, &idx)) continue;
        if (!ls.derived[ls.sp->block_index[idx]].visible) continue;  // never set(): still the AIR the space was built with
        modified_cube_needs_update(ls, cube);
    }
}

// A light session: a space, its light and its update queue kept across calls, as the reference's Space keeps its
// LightUpdateQueue between Mutation::evaluate_light calls. What orc_evaluate_light does in one call can be split into
// several -- budgeted calls, calls with different batch sizes -- and block changes can come in between.
struct LightSession {
    std::vector<uint16_t> block_index;  // the session's own copy: orc_light_session_set_cubes changes it
    orc_space space;                    // the caller's space (blocks, voxels, palette: the caller keeps them alive) over that copy
    LightSpace ls;
    LightSession(const orc_space *s, int32_t maximum_distance, int32_t hb_width)
        : block_index(s->block_index, s->block_index + (size_t)s->size[0] * s->size[1] * s->size[2]),
          space(with_block_index(*s, block_index.data())),
          ls(&space, maximum_distance, hb_width) {}
    static orc_space with_block_index(orc_space s, const uint16_t *bi) {
        s.block_index = bi;
        return s;
    }
};

}  // namespace

extern "C" {

// Per-block derived properties: out[n_blocks][32] floats = color rgba, 6 x face colour rgba, emission rgb,
// then opaque[6] and visible as 0/1 floats... laid out as: [0..4) color, [4..28) faces, [28..31) emission, [31] visible,
// and out_opaque[n_blocks][6].
void orc_compute_derived(const orc_space *space, float *out, uint8_t *out_opaque) {
    for (uint32_t i = 0; i < space->n_blocks; i++) {
        const Derived d = compute_derived(space, space->blocks[i]);
        float *o = out + 32 * (size_t)i;
        o[0] = d.color.r; o[1] = d.color.g; o[2] = d.color.b; o[3] = d.color.a;
        for (int f = 0; f < 6; f++) { o[4 + 4 * f] = d.face_colors[f].r; o[5 + 4 * f] = d.face_colors[f].g; o[6 + 4 * f] = d.face_colors[f].b; o[7 + 4 * f] = d.face_colors[f].a; }
        o[28] = d.emission.r; o[29] = d.emission.g; o[30] = d.emission.b;
        o[31] = d.visible ? 1.f : 0.f;
        for (int f = 0; f < 6; f++) out_opaque[6 * (size_t)i + f] = d.opaque[f] ? 1 : 0;
    }
}

// The light propagation chart: number of nodes; copies weights [n][6] and children [n][6] if non-null.
uint32_t orc_light_chart(float *weights, uint32_t *children) {
    const Chart &c = light_chart();
    if (weights && children)
        for (size_t i = 0; i < c.nodes.size(); i++)
            for (int f = 0; f < 6; f++) { weights[6 * i + f] = c.nodes[i].weight.v[f]; children[6 * i + f] = c.nodes[i].children[f]; }
    return (uint32_t)c.nodes.size();
}

// Space::compute_light for one cube against the light texels in space->light. out_texel[4]; returns the cost.
uint64_t orc_compute_light(const orc_space *space, int32_t maximum_distance, const int32_t cube[3], uint8_t out_texel[4]) {
    LightSpace ls(space, maximum_distance);
    const size_t n = ls.light.size();
    for (size_t i = 0; i < n; i++) ls.light[i] = PackedLight{space->light[4 * i], space->light[4 * i + 1], space->light[4 * i + 2], space->light[4 * i + 3]};
    const ComputedLight c = compute_light(ls, i3(cube[0], cube[1], cube[2]));
    out_texel[0] = c.light.r; out_texel[1] = c.light.g; out_texel[2] = c.light.b; out_texel[3] = c.light.status;
    return c.cost;
}

// Mutation::fast_evaluate_light (if `fast`) followed by Mutation::evaluate_light(epsilon) on LightPhysics::Rays
// { maximum_distance }. light_inout [n][4] texels: the starting state when !fast, the result on return. When !fast
// the queue starts with the n_queue entries given (cube, priority), inserted in that order -- e.g. what
// modified_cube_needs_update (updater.rs:135-173) enqueues after a set() -- or, if n_queue < 0, with every cube whose
// texel status is Uninitialized at Priority::UNINIT. hb_width: the order of equal-priority updates (see LightQueue).
// Returns the update count.
uint64_t orc_evaluate_light(const orc_space *space, int32_t maximum_distance, int32_t fast, int32_t epsilon, int32_t batch,
                            uint64_t max_updates, uint8_t *light_inout, int32_t n_queue, const int32_t *queue_cubes,
                            const int32_t *queue_priorities, int32_t hb_width) {
    LightSpace ls(space, maximum_distance, hb_width);
    const size_t n = ls.light.size();
    if (fast) {
        if (g_light_build_history) replay_build_history(ls);
        fast_evaluate_light(ls);
    } else {
        for (size_t i = 0; i < n; i++) {
            ls.light[i] = PackedLight{light_inout[4 * i], light_inout[4 * i + 1], light_inout[4 * i + 2], light_inout[4 * i + 3]};
            if (n_queue < 0 && ls.light[i].status == 0) ls.queue.insert((uint32_t)i, PRIORITY_UNINIT);
        }
        for (int32_t k = 0; k < n_queue; k++)
            ls.light_needs_update(i3(queue_cubes[3 * k], queue_cubes[3 * k + 1], queue_cubes[3 * k + 2]), queue_priorities[k]);
    }
    const uint64_t total = evaluate_light(ls, epsilon, batch, max_updates);
    for (size_t i = 0; i < n; i++) {
        light_inout[4 * i] = ls.light[i].r; light_inout[4 * i + 1] = ls.light[i].g; light_inout[4 * i + 2] = ls.light[i].b; light_inout[4 * i + 3] = ls.light[i].status;
    }
    return total;
}

// light [n][4]: the starting texels (ignored by a `fast` evaluation). The queue starts empty.
orc_light_session *orc_light_session_create(const orc_space *space, int32_t maximum_distance, const uint8_t *light, int32_t hb_width) {
    LightSession *s = new LightSession(space, maximum_distance, hb_width);
    for (size_t i = 0; i < s->ls.light.size(); i++) s->ls.light[i] = PackedLight{light[4 * i], light[4 * i + 1], light[4 * i + 2], light[4 * i + 3]};
    return reinterpret_cast<orc_light_session *>(s);
}

void orc_light_session_free(orc_light_session *h) { delete reinterpret_cast<LightSession *>(h); }

// Mutation::set for each cube in turn, then modified_cube_needs_update for each in the same order (what aic_update_cubes
// followed by aic_light_cubes_changed does). Cubes outside the space are skipped.
void orc_light_session_set_cubes(orc_light_session *h, int32_t n, const int32_t *cubes, const uint16_t *block_index) {
    LightSession *s = reinterpret_cast<LightSession *>(h);
    for (int32_t k = 0; k < n; k++) {
        size_t idx;
        if (s->ls.index(i3(cubes[3 * k], cubes[3 * k + 1], cubes[3 * k + 2]), &idx)) s->block_index[idx] = block_index[k];
    }
    for (int32_t k = 0; k < n; k++) modified_cube_needs_update(s->ls, i3(cubes[3 * k], cubes[3 * k + 1], cubes[3 * k + 2]));
}

// fast_evaluate_light (if `fast`, which replaces the queue) and then evaluate_light(epsilon) continuing the session's
// queue: batches of `batch` until max_updates is reached (checked between batches) or the queue's highest priority is at
// most from_difference(epsilon). Returns the update count; *cost = their summed ComputedLight::cost, *queue_left = the
// entries left in the queue.
uint64_t orc_light_session_evaluate(orc_light_session *h, int32_t fast, int32_t epsilon, int32_t batch, uint64_t max_updates,
                                    uint64_t *cost, uint64_t *queue_left) {
    LightSession *s = reinterpret_cast<LightSession *>(h);
    if (fast) {
        if (g_light_build_history) replay_build_history(s->ls);
        fast_evaluate_light(s->ls);
    }
    const uint64_t total = evaluate_light(s->ls, epsilon, batch, max_updates, cost);
    if (queue_left) *queue_left = s->ls.queue.len;
    return total;
}

void orc_light_session_read_light(const orc_light_session *h, uint8_t *light_out) {
    const LightSession *s = reinterpret_cast<const LightSession *>(h);
    for (size_t i = 0; i < s->ls.light.size(); i++) {
        const PackedLight &t = s->ls.light[i];
        light_out[4 * i] = t.r; light_out[4 * i + 1] = t.g; light_out[4 * i + 2] = t.b; light_out[4 * i + 3] = t.status;
    }
}

}  // extern "C"
