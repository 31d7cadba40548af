// aic_light_rays.hip -- the kernels of aic_light_rays (include/aic_hip.h): Space::compute_light::<LightUpdateCubeInfo>
// (all-is-cubes/src/space/light/updater.rs:368-417, light/debug.rs) for a batch of cubes, and its wireframe.
//
//  * light_rays_walk_kernel, one workgroup per cube: walks the effective ray-bundle tree (DevTreePos, aic_light.h) level by level as
//    compute_light_wave_body does (aic_light.hip) -- what a bundle adds depends only on the state along its own root path --, with every term in the
//    slot its place in the reference's recursion gives it and a bit per slot in LDS; a second LDS bitmap has a bit per tree position whose bundle
//    pushed a record (updater.rs:844-853). The set bits of the first in ascending order are the reference's order of f32 additions, added by one chain
//    per accumulator; those of the second are the reference's order of records, because the tree's positions are its pre-order. Both are compacted by
//    gather_set_bits (aic_bit_gather.h). Neither order depends on which lane visited what.
//  * light_rays_scan_kernel, one workgroup: first_ray and the totals (scan_block_counts, aic_rank_list.h), the infos, which cubes are stored.
//  * light_rays_emit_kernel, a thread per stored record: a record is a function of its cube and its tree position alone.
//  * light_rays_lines_kernel, a thread per line (aic_light_rays_lines.h: the text the host's aic_light_rays_wireframe runs too).
//
// Every f32 and f64 operation is done in the reference's order (built with -ffp-contract=off).
#include "aic_light_rays.h"

#include "aic_bit_gather.h"
#include "aic_light_arith.h"
#include "aic_rank_list.h"

namespace aic {
namespace {

// vol.rs:988-1023
__device__ __forceinline__ bool index_of(const LightRaysParams &P, const int c[3], uint32_t *out) {
    const uint32_t dx = (uint32_t)c[0] - (uint32_t)P.lo[0], dy = (uint32_t)c[1] - (uint32_t)P.lo[1], dz = (uint32_t)c[2] - (uint32_t)P.lo[2];
    if ((dx >= (uint32_t)P.size[0]) | (dy >= (uint32_t)P.size[1]) | (dz >= (uint32_t)P.size[2])) return false;
    *out = (dx * (uint32_t)P.size[1] + dy) * (uint32_t)P.size[2] + dz;
    return true;
}
// sky.rs:113-147 BlockSky::light_outside
__device__ uint32_t light_outside(const LightRaysParams &P, const int c[3]) {
    int n_less = 0, n_equal = 0, which = -1;
    for (int a = 0; a < 3; a++) {
        int lower;
        if (P.lo[a] == (int32_t)0x80000000) lower = -1;
        else {
            const int beyond = P.lo[a] - 1;
            lower = beyond < c[a] ? -1 : (beyond == c[a] ? 0 : 1);
        }
        if (lower == -1) n_less++;
        else if (lower == 0) { n_equal++; which = a; }
    }
    for (int a = 0; a < 3; a++) {
        const long long hi = (long long)P.lo[a] + P.size[a];
        const int upper = (long long)c[a] < hi ? -1 : ((long long)c[a] == hi ? 0 : 1);
        if (upper == -1) n_less++;
        else if (upper == 0) { n_equal++; which = 3 + a; }
    }
    if (n_less == 5 && n_equal == 1) return P.block_sky[which];
    if (n_less == 6) return 0u;
    return 1u << 24;
}
__device__ __forceinline__ uint32_t get_light(const LightRaysParams &P, const int c[3]) {  // updater.rs:572-582
    uint32_t i;
    if (index_of(P, c, &i)) return P.light[i];
    return light_outside(P, c);
}
__device__ __forceinline__ void tree_cube(const int origin[3], uint32_t off, int cube[3]) {
    cube[0] = origin[0] + (int)(off & 1023u) - 256;
    cube[1] = origin[1] + (int)((off >> 10) & 1023u) - 256;
    cube[2] = origin[2] + (int)((off >> 20) & 1023u) - 256;
}

// What the bundle at a record's tree position read and reflected (updater.rs:808-826): a function of the cube and the position alone.
__device__ void ray_record(const LightRaysParams &P, const float *lut, const int origin[3], uint32_t k, aic_light_ray *out) {
    const DevTreePos *nd = &P.tree[k];
    const int fe = (int)(nd->info & 7u);  // a record's bundle entered its cube through a real face
    int cube[3], n[3];
    tree_cube(origin, nd->offset, cube);
    normal_of(fe < 6 ? fe : 0, n);
    const int light_cube[3] = {cube[0] + n[0], cube[1] + n[1], cube[2] + n[2]};
    uint32_t idx = 0u;
    (void)index_of(P, cube, &idx);  // (inside: the walk looked its block up)
    const DevDerived *ev = &P.derived[P.grid[idx] & P.index_mask];
    const float *scp = ev->face[fe < 6 ? fe : 0];
    float sc[4] = {scp[0], scp[1], scp[2], scp[3]};
    for (int i = 0; i < 3; i++) sc[i] = sc[i] > 1.f ? 1.f : sc[i];  // Rgba::clamp (color.rs:692-697)
    const uint32_t stored = get_light(P, light_cube);
    for (int a = 0; a < 3; a++) { out->trigger_cube[a] = cube[a]; out->value_cube[a] = light_cube[a]; }
    for (int i = 0; i < 4; i++) out->value[i] = (uint8_t)(stored >> (8 * i));
    for (int i = 0; i < 3; i++) out->light_from_struck_face[i] = ev->emission[i] + ps_mul(ps_mul(sc[i], lut[(stored >> (8 * i)) & 255u]), sc[3]);
}

struct RayWalk {
    const LightRaysParams &P;
    int origin[3];
    uint32_t m0;            // direction weights of the walk: bit per face (updater.rs:668-690)
    float sky_value[6][3];
    float4 *slots;
    uint32_t *term_bits, *ray_bits;  // LDS bitmaps
    uint32_t cost;
    const float *lut;       // LDS

    __device__ explicit RayWalk(const LightRaysParams &p) : P(p) {}
    __device__ void value_of(uint32_t texel, float v[3]) const {  // data.rs:137-143
        v[0] = lut[texel & 255u];
        v[1] = lut[(texel >> 8) & 255u];
        v[2] = lut[(texel >> 16) & 255u];
    }
    __device__ float bundle_weight(const float w[6]) const {  // (weight * direction_weights).sum(), face.rs:1046-1054
        float p[6];
        for (int f = 0; f < 6; f++) p[f] = ((m0 >> f) & 1u) ? w[f] : 0.f;
        return (p[0] + p[3]) + (p[1] + p[4]) + (p[2] + p[5]);
    }
    __device__ void emit_term(uint32_t seq, float x, float y, float z, float weight) {
        slots[seq] = make_float4(x, y, z, weight);
        atomicOr(&term_bits[seq >> 5], 1u << (seq & 31u));
    }
    // updater.rs:899-927 + add_weighted_light
    __device__ void end_of_ray(uint32_t seq, float alpha, float ray_bundle_weight, const float w[6]) {
        if (!(ray_bundle_weight > 0.f)) return;
        const float recip = ps_new_clamped(1.0f / ((w[0] + w[3]) + (w[1] + w[4]) + (w[2] + w[5])));
        const float ww = ps_new_clamped(ray_bundle_weight);
        float out[3];
        for (int i = 0; i < 3; i++) {
            float pf[6];
            for (int f = 0; f < 6; f++) pf[f] = ps_mul(sky_value[f][i], ps_new_clamped(w[f]));
            const float s = (pf[0] + pf[3]) + (pf[1] + pf[4]) + (pf[2] + pf[5]);
            const float sky_light = ps_mul(ps_mul(s, recip), ps_new_clamped(alpha));
            out[i] = ps_mul(sky_light, ww);
        }
        emit_term(seq, out[0], out[1], out[2], ray_bundle_weight);
    }
    // walk_ray_tree (updater.rs:427-530) for the bundle at tree position k, entered with alpha_in. Returns whether its children are to be walked, then
    // *alpha_out is the alpha behind the cube. Everything the bundle adds -- on entering and, if it lives, after its children -- goes into its numbered
    // slots: 4 k - depth is the number of additions the recursion makes before it enters position k (three per bundle entered before: face term,
    // volume term, end of ray; one per bundle left before: the "rest" term).
    __device__ bool visit(uint32_t k, float alpha_in, float *alpha_out) {
        const DevTreePos *nd = &P.tree[k];
        float w[6];
        for (int f = 0; f < 6; f++) w[f] = nd->weight[f];
        const uint32_t info = nd->info, off = nd->offset, end = nd->end;
        const float rbw = bundle_weight(w);
        if (rbw <= 0.0f) return false;
        const uint32_t depth = (info >> 8) & 0xffffu;
        const uint32_t seq = 4u * k - depth;
        float alpha = alpha_in;
        bool alive = false;
        uint32_t eseq = seq;
        float eweight = rbw;
        int cube[3];
        tree_cube(origin, off, cube);
        uint32_t idx = 0u;
        if (!(info & 8u)) {  // within maximum_distance
            cost += 1u;
            if (index_of(P, cube, &idx)) {
                const int fe = (info & 7u) == 7u ? -1 : (int)(info & 7u);
                // LightBuffer::traverse (updater.rs:770-895)
                const DevDerived *ev = &P.derived[P.grid[idx] & P.index_mask];
                const uint32_t flags = ev->flags;
                if (flags & kDerivedVisible) {
                    const bool hit_opaque_face = fe < 0 ? (flags & 63u) == 63u : ((flags >> fe) & 1u) != 0u;
                    if (hit_opaque_face && fe < 0) {
                        alpha = 0.f;
                    } else {
                        const float *scp = fe < 0 ? ev->color : ev->face[fe];
                        float sc[4] = {scp[0], scp[1], scp[2], scp[3]};
                        for (int i = 0; i < 3; i++) sc[i] = sc[i] > 1.f ? 1.f : sc[i];
                        const float hit_alpha = sc[3];
                        const float em[3] = {ev->emission[0], ev->emission[1], ev->emission[2]};
                        if (hit_alpha > 0.f && fe >= 0) {
                            int n[3];
                            normal_of(fe, n);
                            const int light_cube[3] = {cube[0] + n[0], cube[1] + n[1], cube[2] + n[2]};
                            float sv[3];
                            value_of(get_light(P, light_cube), sv);
                            const float a = ps_new_clamped(alpha), ww = ps_new_clamped(rbw);
                            float t[3];
                            for (int i = 0; i < 3; i++) t[i] = ps_mul(ps_mul(em[i] + ps_mul(ps_mul(sc[i], sv[i]), sc[3]), a), ww);
                            emit_term(seq, t[0], t[1], t[2], 0.f);
                            cost += 10u;
                            if (hit_opaque_face) {
                                alpha = 0.f;
                                atomicOr(&ray_bits[k >> 5], 1u << (k & 31u));  // D::push_ray (updater.rs:844-853)
                            } else {
                                alpha *= 1.0f - hit_alpha;
                            }
                        }
                        if (hit_alpha < 1.0f) {
                            float sl[3] = {0.f, 0.f, 0.f};
                            if (fe >= 0) value_of(P.light[idx], sl);
                            const float a = ps_new_clamped(alpha), ww = ps_new_clamped(rbw);
                            float t[3];
                            for (int i = 0; i < 3; i++) t[i] = ps_mul(ps_mul(em[i] + ps_mul(sl[i], hit_alpha), a), ww);
                            emit_term(seq + 1u, t[0], t[1], t[2], 0.f);
                            cost += 10u;
                            alpha *= 1.0f - hit_alpha;
                        }
                    }
                }
                if (alpha > 0.0f) {
                    // After the children: the weight they did not take (updater.rs:507-528). What a child returns is its own bundle weight
                    // (updater.rs:437-441), a function of its chart weights and this walk's direction weights only.
                    alive = true;
                    const float *cw = P.child_w + (size_t)k * 36u;
                    float cws = 0.0f;
                    for (int f = 0; f < 6; f++) cws += bundle_weight(cw + 6 * f);  // no child on that face: zeros, and x + 0 = x
                    const float rest = rbw - cws;
                    eweight = rest > 0.0f ? rest : 0.0f;
                    eseq = 4u * end - depth - 1u;
                } else {
                    eseq = seq + 2u;
                }
            }
        }
        end_of_ray(eseq, alpha, eweight, w);
        *alpha_out = alpha;
        return alive && end > k + 1u;
    }
};

__global__ void __launch_bounds__(kLightRaysBlock) light_rays_walk_kernel(const LightRaysParams P) {
    extern __shared__ uint32_t s_dyn[];  // term bitmap, record bitmap
    __shared__ float s_lut[256];
    __shared__ uint32_t s_count[3], s_scan[4];
    __shared__ float s_sum[4];
    __shared__ float4 s_stage[kLightRaysBlock];
    __shared__ uint32_t s_order[kOrderCap];
    const uint32_t tid = threadIdx.x, nt = kLightRaysBlock;
    const uint32_t term_words = (4u * P.n_tree + 31u) / 32u, ray_words = (P.n_tree + 31u) / 32u;
    uint32_t *const term_bits = s_dyn, *const ray_bits = s_dyn + term_words;
    for (uint32_t i = tid; i < 256u; i += nt) s_lut[i] = P.lut[i];
    __syncthreads();
    RayWalk b(P);
    b.lut = s_lut;
    b.term_bits = term_bits;
    b.ray_bits = ray_bits;
    b.slots = P.slots + (size_t)blockIdx.x * 4u * P.n_tree;
    uint2 *const queue = P.queue + (size_t)blockIdx.x * P.n_tree;
    for (int f = 0; f < 6; f++) b.value_of(P.block_sky[f], b.sky_value[f]);

    for (uint32_t item = blockIdx.x; item < P.n; item += gridDim.x) {  // (every branch below is taken by the whole workgroup alike)
        for (int a = 0; a < 3; a++) b.origin[a] = P.cubes[3u * item + (uint32_t)a];
        uint32_t ci = 0u, texel = 0u, cost = 0u, n_rays = 0u, flags = 0u;
        if (!index_of(P, b.origin, &ci)) {
            flags = AIC_LIGHT_CUBE_OUTSIDE;
        } else {
            const DevDerived *ev_origin = &P.derived[P.grid[ci] & P.index_mask];
            const bool origin_is_opaque = (ev_origin->flags & 63u) == 63u;
            const bool origin_emits = !(ev_origin->emission[0] == 0.f && ev_origin->emission[1] == 0.f && ev_origin->emission[2] == 0.f);
            float inc[3] = {0.f, 0.f, 0.f}, total = 0.f;
            b.cost = 0u;
            if (origin_is_opaque) {
                if (origin_emits) {  // add_weighted_light(emission, 1.0): !opaque_for_light_computation (updater.rs:1031-1033)
                    for (int i = 0; i < 3; i++) inc[i] += ps_mul(ev_origin->emission[i], ps_new_clamped(1.0f));
                    total += 1.0f;
                }
            } else {
                for (uint32_t i = tid; i < term_words + ray_words; i += nt) s_dyn[i] = 0u;
                // directions_to_seek_light (updater.rs:668-690); every thread works it out for itself
                uint32_t m0 = 0u;
                if (ev_origin->flags & kDerivedVisible) m0 = 63u;
                else {
                    uint32_t vis = 0u, emi = 0u;
                    for (int f = 0; f < 6; f++) {
                        int n[3];
                        normal_of(f, n);
                        const int c[3] = {b.origin[0] + n[0], b.origin[1] + n[1], b.origin[2] + n[2]};
                        uint32_t i;
                        if (index_of(P, c, &i)) {
                            const DevDerived *d = &P.derived[P.grid[i] & P.index_mask];
                            if (d->flags & kDerivedVisible) vis |= 1u << f;
                            if (!(d->emission[0] == 0.f && d->emission[1] == 0.f && d->emission[2] == 0.f)) emi |= 1u << f;
                        }
                    }
                    for (int f = 0; f < 6; f++) {
                        const int opp = f >= 3 ? f - 3 : f + 3;
                        if (((vis >> opp) & 1u) || ((emi >> f) & 1u)) m0 |= 1u << f;
                    }
                }
                b.m0 = m0;
                if (tid == 0u) {
                    queue[0] = make_uint2(0u, __float_as_uint(1.0f));
                    s_count[0] = 0u;  // this level's first entry
                    s_count[1] = 1u;  // ... and one past its last
                    s_count[2] = 1u;  // entries appended
                }
                // The walk, a level of the queue at a time. A thread follows a bundle's only child at once (nearly all of the tree is chains) and
                // appends the children of a bundle that branches for the next level; each position is appended at most once, so n_tree entries hold them.
                for (;;) {
                    __syncthreads();
                    const uint32_t begin = s_count[0], end = s_count[1];
                    __syncthreads();
                    if (begin == end) break;
                    for (uint32_t i = begin + tid; i < end; i += nt) {
                        const uint2 ent = queue[i];
                        uint32_t k = ent.x;
                        float alpha = __uint_as_float(ent.y);
                        for (uint32_t guard = 0u; guard < P.n_tree; guard++) {  // (a chain is shorter than the tree)
                            float behind;
                            if (!b.visit(k, alpha, &behind)) break;
                            const uint2 *ce = P.child_ent + (size_t)k * 6u;
                            uint32_t ch[6], nch = 0u, only = 0u;
                            for (int f = 0; f < 6; f++) {
                                ch[f] = ce[f].x & 0x3fffffu;
                                if (ch[f] != 0u) { nch++; only = ch[f]; }
                            }
                            if (nch == 1u && only < P.n_tree) {
                                k = only;
                                alpha = behind;
                                continue;
                            }
                            uint32_t at = atomicAdd(&s_count[2], nch);
                            for (int f = 0; f < 6; f++)
                                if (ch[f] != 0u && ch[f] < P.n_tree) {
                                    if (at < P.n_tree) queue[at] = make_uint2(ch[f], __float_as_uint(behind));
                                    at++;
                                }
                            break;
                        }
                    }
                    __syncthreads();
                    if (tid == 0u) {
                        s_count[0] = end;
                        s_count[1] = min(s_count[2], P.n_tree);
                    }
                }
                // Ordered reduction, as in compute_light_wave_body: the set bits in ascending order are the reference's order of additions; lanes 0..3
                // add red, green, blue and the weight, one chain of f32 additions each, which is what LightBuffer does to its four accumulators.
                float acc = 0.f;
                uint32_t word = 0u;
                for (;;) {
                    const uint32_t got = gather_set_bits(term_bits, term_words, &word, s_order, tid, nt, s_scan);
                    if (got == 0u) break;
                    if (got == 0xffffffffu) continue;
                    for (uint32_t c0 = 0u; c0 < got; c0 += nt) {
                        const uint32_t m = min(nt, got - c0);
                        if (tid < m) s_stage[tid] = b.slots[s_order[c0 + tid]];
                        __syncthreads();
                        if (tid < 4u) {
                            const float *sf = reinterpret_cast<const float *>(s_stage) + tid;
                            for (uint32_t i = 0u; i < m; i++) acc += sf[4u * i];
                        }
                        __syncthreads();
                    }
                }
                if (tid < 4u) s_sum[tid] = acc;
                // The records: the set bits of the record bitmap in ascending order are walk_ray_tree's depth-first order.
                word = 0u;
                for (;;) {
                    const uint32_t got = gather_set_bits(ray_bits, ray_words, &word, s_order, tid, nt, s_scan);
                    if (got == 0u) break;
                    if (got == 0xffffffffu) continue;
                    for (uint32_t i = tid; i < got; i += nt)
                        if (n_rays + i < P.bound) P.positions[(size_t)item * P.bound + n_rays + i] = s_order[i];
                    n_rays += got;
                    __syncthreads();  // s_order is written again by the next gather
                }
                n_rays = min(n_rays, P.bound);  // (never more: aic_light_rays_bound)
                __syncthreads();
                inc[0] = s_sum[0]; inc[1] = s_sum[1]; inc[2] = s_sum[2]; total = s_sum[3];
            }
            // cost, summed over the workgroup: an integer, any order
            cost = b.cost;
            for (int d = 32; d > 0; d >>= 1) cost += __shfl_down(cost, d, 64);
            __syncthreads();
            if ((tid & 63u) == 0u) s_scan[tid >> 6] = cost;
            __syncthreads();
            cost = s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
            // LightBuffer::finish (updater.rs:940-952)
            const float scale = ps_new_clamped(1.0f / fmaxf(total, 1.0f));
            if (total > 0.0f) {
                texel = packed_scalar_in(ps_mul(inc[0], scale)) | (packed_scalar_in(ps_mul(inc[1], scale)) << 8) | (packed_scalar_in(ps_mul(inc[2], scale)) << 16) |
                        (255u << 24);
            } else if (origin_is_opaque) {
                texel = 128u << 24;
            } else {
                texel = 1u << 24;
            }
        }
        if (tid == 0u) {
            LightRayResult r;
            r.texel = texel; r.cost = cost; r.flags = flags; r.pad = 0u;
            P.results[item] = r;
            P.counts[item] = n_rays;
        }
        __syncthreads();  // LDS, the slots and the queue are reused by the workgroup's next cube
    }
}

// first_ray, which cubes are stored, the infos and the totals: one workgroup of 1024
__global__ void __launch_bounds__(1024) light_rays_scan_kernel(const LightRaysParams P) {
    __shared__ uint32_t s_stored[2];
    if (threadIdx.x == 0u) s_stored[0] = s_stored[1] = 0u;
    const uint32_t total = scan_block_counts(P.counts, P.offsets, P.n);  // (its barriers order s_stored too)
    for (uint32_t i = threadIdx.x; i < P.n; i += 1024u) {  // (offsets[i] was written by this thread)
        const uint32_t first = P.offsets[i], count = P.counts[i];
        const LightRayResult r = P.results[i];
        const bool stored = (unsigned long long)first + count <= (unsigned long long)P.capacity;
        aic_light_cube_info info;
        for (int a = 0; a < 3; a++) info.cube[a] = P.cubes[3u * i + (uint32_t)a];
        for (int q = 0; q < 4; q++) info.result[q] = (uint8_t)(r.texel >> (8 * q));
        info.cost = r.cost;
        info.n_rays = count;
        info.first_ray = first;
        info.flags = r.flags | (stored ? AIC_LIGHT_CUBE_STORED : 0u);
        P.infos[i] = info;
        if (stored) {  // the stored cubes are a prefix of the batch: first_ray never decreases
            atomicAdd(&s_stored[0], 1u);
            atomicMax(&s_stored[1], first + count);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        P.totals[0] = total;
        P.totals[1] = s_stored[0];
        P.totals[2] = s_stored[1];
        P.totals[3] = 0ull;
    }
}

// the last of the first `n` entries of a non-decreasing list that is <= x (entry 0 is 0 <= x)
template <class F>
__device__ __forceinline__ uint32_t last_not_above(uint32_t n, unsigned long long x, F entry) {
    uint32_t lo = 0u, hi = n;  // entry(lo) <= x < entry(hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (entry(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) light_rays_emit_kernel(const LightRaysParams P) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= P.n_stored_rays) return;
    const uint32_t k = last_not_above(P.n_stored, r, [&](uint32_t i) { return (unsigned long long)P.offsets[i]; });
    const uint32_t j = r - P.offsets[k];
    if (j >= P.counts[k]) return;  // (never: r lies in the records of the last cube that starts at or before it)
    const int origin[3] = {P.cubes[3u * k], P.cubes[3u * k + 1u], P.cubes[3u * k + 2u]};
    ray_record(P, P.lut, origin, P.positions[(size_t)k * P.bound + j], &P.rays[r]);
}

__global__ void __launch_bounds__(256) light_rays_lines_kernel(const LightRaysParams P) {
    const unsigned long long n_lines = (unsigned long long)kLightRayBoxLines * P.n_stored + (unsigned long long)kLightRayLines * P.n_stored_rays;
    const unsigned long long line = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (line >= n_lines) return;
    auto start = [&](uint32_t i) { return (unsigned long long)kLightRayBoxLines * i + (unsigned long long)kLightRayLines * P.offsets[i]; };
    const uint32_t k = last_not_above(P.n_stored, line, start);
    const uint32_t j = (uint32_t)(line - start(k));
    if (j >= kLightRayBoxLines + kLightRayLines * P.counts[k]) return;  // (never)
    const int32_t cube[3] = {P.cubes[3u * k], P.cubes[3u * k + 1u], P.cubes[3u * k + 2u]};
    aic_line_vertex v[2];
    light_rays_line(cube, P.rays + P.offsets[k], P.angles, j, v);
    P.lines[2ull * line] = v[0];
    P.lines[2ull * line + 1ull] = v[1];
}

}  // namespace

hipError_t launch_light_rays_walk(const LightRaysParams &p, uint32_t workgroups, hipStream_t stream) {
    const uint32_t lds = light_rays_bitmap_words(p.n_tree) * 4u;
    // more dynamic LDS than the default limit needs an opt-in, per device
    static uint32_t lds_allowed[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    uint32_t &allowed = lds_allowed[dev & 63];
    if (lds > allowed) {
        if (const hipError_t e = hipFuncSetAttribute((const void *)light_rays_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
        allowed = lds;
    }
    hipLaunchKernelGGL(light_rays_walk_kernel, dim3(workgroups), dim3(kLightRaysBlock), lds, stream, p);
    return hipGetLastError();
}

hipError_t launch_light_rays_scan(const LightRaysParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(light_rays_scan_kernel, dim3(1), dim3(1024), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_light_rays_emit(const LightRaysParams &p, hipStream_t stream) {
    if (p.n_stored_rays) {
        hipLaunchKernelGGL(light_rays_emit_kernel, dim3((p.n_stored_rays + 255u) / 256u), dim3(256), 0, stream, p);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    const unsigned long long n_lines = (unsigned long long)kLightRayBoxLines * p.n_stored + (unsigned long long)kLightRayLines * p.n_stored_rays;
    if (p.lines && n_lines) {
        hipLaunchKernelGGL(light_rays_lines_kernel, dim3((uint32_t)((n_lines + 255ull) / 256ull)), dim3(256), 0, stream, p);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace aic
