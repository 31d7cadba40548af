// aic_light_chart.cpp -- the light updater's ray chart and the trees made of it (aic_light_host.h). Cold: the chart is generated once per process, a
// tree once per maximum_distance. Follows
//   all-is-cubes/src/space/light/chart/generator.rs   the chart
// Built like the other host units (-x hip): DevLightNode and DevTreePos are the device's records (aic_light.h).

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "aic_light_host.h"

using namespace aic;

namespace {

// ------------------------------------------------------------------------------------
// chart/generator.rs: rays towards every cell of the surface of an 11x11x11 cube (602 of them), stepped through the
// grid from the centre of the origin cube up to distance 127, merged into a tree by shared prefixes, then flattened in
// post-order from the end so that the root is node 0.

LightChart generate_light_chart() {
    struct TreeNode {
        int32_t cube[3];
        int32_t children[6];
        float weight[6];
    };
    std::vector<TreeNode> tree;
    {
        TreeNode root;
        for (int a = 0; a < 3; a++) root.cube[a] = 0;
        for (int f = 0; f < 6; f++) { root.children[f] = -1; root.weight[f] = 0.f; }
        tree.push_back(root);
    }
    const int STEP = 5;  // RAY_DIRECTION_STEP (generator.rs)
    std::vector<I3h> steps;
    for (int x = -STEP; x <= STEP; x++)
        for (int y = -STEP; y <= STEP; y++)
            for (int z = -STEP; z <= STEP; z++) {
                if (!(std::abs(x) == STEP || std::abs(y) == STEP || std::abs(z) == STEP)) continue;
                const float fx = (float)x, fy = (float)y, fz = (float)z;
                const float len = std::sqrt(fx * fx + fy * fy + fz * fz);
                const float d[3] = {fx / len, fy / len, fz / len};  // Vector3D::normalize
                float cosw[6];
                for (int f = 0; f < 6; f++) {
                    const I3h n = face_normal_h(f);
                    const float dotv = (float)n[0] * d[0] + (float)n[1] * d[1] + (float)n[2] * d[2];
                    cosw[f] = dotv > 0.0f ? dotv : 0.0f;
                }
                // Ray::new([0.5; 3], direction).cast().take_while(|step| step.t_distance() <= 127.0): the raycaster of
                // math/raycast.rs from the cube centre -- t_max = 0.5 / |d| per moving axis, the smallest strictly-less
                // t_max steps, ties to the later axis (raycast.rs:577-626)
                double t_max[3], t_delta[3];
                int stepdir[3];
                for (int a = 0; a < 3; a++) {
                    const double da = (double)d[a];
                    stepdir[a] = da > 0.0 ? 1 : (da < 0.0 ? -1 : 0);
                    t_delta[a] = 1.0 / std::fabs(da);
                    t_max[a] = da == 0.0 ? INFINITY : (1.0 - 0.5) / std::fabs(da);
                }
                steps.clear();
                I3h cube = {0, 0, 0};
                double t = 0.0;
                while (t <= 127.0) {
                    steps.push_back(cube);
                    int axis;
                    if (t_max[0] < t_max[1]) axis = (t_max[0] < t_max[2]) ? 0 : 2;
                    else axis = (t_max[1] < t_max[2]) ? 1 : 2;
                    t = t_max[axis];
                    cube[(size_t)axis] += stepdir[axis];
                    t_max[axis] += t_delta[axis];
                }
                // tree.insert(&steps[1..], weight)
                int node = 0;
                for (int f = 0; f < 6; f++) tree[0].weight[f] += cosw[f];
                for (size_t k = 1; k < steps.size(); k++) {
                    const I3h c = steps[k];
                    int dir = -1;
                    for (int f = 0; f < 6; f++) {
                        const I3h n = face_normal_h(f);
                        if (tree[(size_t)node].cube[0] + n[0] == c[0] && tree[(size_t)node].cube[1] + n[1] == c[1] && tree[(size_t)node].cube[2] + n[2] == c[2]) dir = f;
                    }
                    if (dir < 0) break;
                    int child = tree[(size_t)node].children[dir];
                    if (child < 0) {
                        TreeNode n;
                        for (int a = 0; a < 3; a++) n.cube[a] = c[(size_t)a];
                        for (int f = 0; f < 6; f++) { n.children[f] = -1; n.weight[f] = 0.f; }
                        child = (int)tree.size();
                        tree.push_back(n);
                        tree[(size_t)node].children[dir] = child;
                    }
                    node = child;
                    for (int f = 0; f < 6; f++) tree[(size_t)node].weight[f] += cosw[f];
                }
            }
    LightChart chart;
    chart.nodes.resize(tree.size());
    std::vector<uint32_t> flat_index(tree.size(), 0);
    uint32_t next_index = (uint32_t)tree.size() - 1;
    struct Frame { int node; int child; };
    std::vector<Frame> stack;
    stack.push_back(Frame{0, 0});
    while (!stack.empty()) {
        chart.depth = std::max(chart.depth, (uint32_t)stack.size());
        Frame &fr = stack.back();
        if (fr.child < 6) {
            const int c = tree[(size_t)fr.node].children[fr.child++];
            if (c >= 0) stack.push_back(Frame{c, 0});
            continue;
        }
        const int n = fr.node;
        stack.pop_back();
        const uint32_t this_index = next_index;
        if (this_index != 0) next_index -= 1;
        flat_index[(size_t)n] = this_index;
        DevLightNode fn;
        for (int f = 0; f < 6; f++) {
            fn.weight[f] = tree[(size_t)n].weight[f];
            fn.child[f] = tree[(size_t)n].children[f] >= 0 ? flat_index[(size_t)tree[(size_t)n].children[f]] : 0u;
        }
        chart.nodes[this_index] = fn;
    }
    return chart;
}

}  // namespace

namespace aic {

const LightChart &light_chart() {
    static const LightChart chart = generate_light_chart();
    return chart;
}

// The part of the chart a walk with the given maximum_distance can reach, in pre-order with children in face order:
// a bundle whose cube centre is farther than maximum_distance from the origin's ends the ray (updater.rs:456-462), so it
// is a leaf here. What the wave-per-cube kernel walks (aic_light.h).
std::vector<DevTreePos> build_light_tree(int maximum_distance, uint32_t *depth_out, std::vector<float> *child_w, std::vector<uint32_t> *child_pos) {
    const LightChart &ch = light_chart();
    std::vector<DevTreePos> out;
    struct Frame { uint32_t node, pos; int32_t off[3]; int next_face; };
    std::vector<Frame> stack;
    const double max2 = (double)maximum_distance * (double)maximum_distance;
    uint32_t depth = 0;
    auto push = [&](uint32_t node, uint32_t parent_pos, const int32_t off[3], uint32_t fe) {
        DevTreePos t;
        for (int f = 0; f < 6; f++) t.weight[f] = ch.nodes[node].weight[f];
        t.end = 0;
        t.parent = parent_pos;
        t.offset = (uint32_t)(off[0] + 256) | ((uint32_t)(off[1] + 256) << 10) | ((uint32_t)(off[2] + 256) << 20);
        const double d2 = (double)off[0] * off[0] + (double)off[1] * off[1] + (double)off[2] * off[2];
        const bool far_ = d2 > max2;
        t.info = fe | (far_ ? 8u : 0u) | ((uint32_t)stack.size() << 8);  // depth = number of ancestors
        const uint32_t pos = (uint32_t)out.size();
        out.push_back(t);
        Frame fr;
        fr.node = node; fr.pos = pos; fr.next_face = far_ ? 6 : 0;
        for (int a = 0; a < 3; a++) fr.off[a] = off[a];
        stack.push_back(fr);
    };
    const int32_t zero[3] = {0, 0, 0};
    push(0, 0, zero, 7u);
    while (!stack.empty()) {
        depth = std::max(depth, (uint32_t)stack.size());
        Frame &fr = stack.back();
        if (fr.next_face < 6) {
            const int f = fr.next_face++;
            const uint32_t c = ch.nodes[fr.node].child[f];
            if (c != 0u) {
                const I3h n = face_normal_h(f);
                const int32_t off[3] = {fr.off[0] + n[0], fr.off[1] + n[1], fr.off[2] + n[2]};
                const uint32_t parent_pos = fr.pos;
                if (child_w) {
                    if (child_w->size() < ((size_t)parent_pos + 1) * 36) child_w->resize(((size_t)parent_pos + 1) * 36, 0.f);
                    for (int g = 0; g < 6; g++) (*child_w)[(size_t)parent_pos * 36 + (size_t)f * 6 + (size_t)g] = ch.nodes[c].weight[g];
                }
                if (child_pos) {
                    if (child_pos->size() < ((size_t)parent_pos + 1) * 6) child_pos->resize(((size_t)parent_pos + 1) * 6, 0u);
                    (*child_pos)[(size_t)parent_pos * 6 + (size_t)f] = (uint32_t)out.size();
                }
                push(c, parent_pos, off, (uint32_t)(f >= 3 ? f - 3 : f + 3));  // entered through the opposite face
            }
            continue;
        }
        out[fr.pos].end = (uint32_t)out.size();
        stack.pop_back();
    }
    if (depth_out) *depth_out = depth;
    if (child_w) child_w->resize(out.size() * 36, 0.f);
    if (child_pos) child_pos->resize(out.size() * 6, 0u);
    return out;
}

// What aic_light_rays (aic_light_rays_host.cpp) takes from here. The effective tree of a maximum_distance with its children's weights and entries
// (the entry's first word is the child's position; the rest of it is the updater's own); the bound counts the bundles within the distance, the root
// apart, that have no child within it: a record ends its bundle (updater.rs:838-853), so no two of a cube's records lie on one root path, and those
// are the most positions no two of which do.
void light_rays_tree(int maximum_distance, LightRaysTree *out) {
    std::vector<uint32_t> child_pos;
    out->tree = build_light_tree(maximum_distance, nullptr, &out->child_w, &child_pos);
    out->child_ent.resize(child_pos.size());
    for (size_t q = 0; q < child_pos.size(); q++) out->child_ent[q] = child_pos[q] ? make_uint2(child_pos[q], out->tree[child_pos[q]].offset) : make_uint2(0u, 0u);
    out->bound = 0;
    for (size_t k = 1; k < out->tree.size(); k++) {
        if (out->tree[k].info & 8u) continue;
        bool child_within = false;
        for (int f = 0; f < 6; f++) {
            const uint32_t cp = child_pos[k * 6 + (size_t)f];
            child_within = child_within || (cp != 0u && !(out->tree[cp].info & 8u));
        }
        if (!child_within) out->bound++;
    }
}
uint32_t light_rays_bound(int maximum_distance) {
    static std::mutex mu;
    static int64_t known[256];
    static bool init = false;
    std::lock_guard<std::mutex> lk(mu);
    if (!init) { for (auto &k : known) k = -1; init = true; }
    if (known[maximum_distance] < 0) {
        LightRaysTree t;
        light_rays_tree(maximum_distance, &t);
        known[maximum_distance] = t.bound;
    }
    return (uint32_t)known[maximum_distance];
}

}  // namespace aic

extern "C" uint32_t aic_light_chart(float *weights, uint32_t *children, uint32_t *depth) {
    const LightChart &ch = light_chart();
    if (weights && children)
        for (size_t i = 0; i < ch.nodes.size(); i++)
            for (int f = 0; f < 6; f++) { weights[6 * i + (size_t)f] = ch.nodes[i].weight[f]; children[6 * i + (size_t)f] = ch.nodes[i].child[f]; }
    if (depth) *depth = ch.depth;
    return (uint32_t)ch.nodes.size();
}
