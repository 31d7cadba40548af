// aic_cursor.cpp -- aic_cursor_wireframe: impl Wireframe for Cursor (all-is-cubes/src/character/cursor.rs:219-278) restated on the host, in f64 and in
// the reference's order of operations, as the line list aic_present_split_lines draws. No device, no context.
#include <cmath>

#include "../../include/aic_hip.h"

namespace {

struct Box { double lo[3], hi[3]; };

// Aab::wireframe_points (all-is-cubes-base/src/math/aab.rs:569-588): pairs of octants, a set bit = the upper bound on that axis (bit 2 x, 1 y, 0 z)
const int kWireframe[12][2] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};

void put(aic_line_vertex *&out, double x, double y, double z) {
    out->position[0] = (float)x; out->position[1] = (float)y; out->position[2] = (float)z;
    out->color[0] = out->color[1] = out->color[2] = 0.f;  // palette::CURSOR_OUTLINE, linear (vertex.rs:404-409)
    out->color[3] = 1.f;
    out++;
}

void box_edges(const Box &b, aic_line_vertex *&out) {
    for (const auto &edge : kWireframe)
        for (int corner : edge) put(out, corner & 4 ? b.hi[0] : b.lo[0], corner & 2 ? b.hi[1] : b.lo[1], corner & 1 ? b.hi[2] : b.lo[2]);
}

}  // namespace

extern "C" int aic_cursor_wireframe(const aic_cursor_desc *c, aic_line_vertex *out, uint32_t *n_lines) {
    if (!c || !out || !n_lines) return AIC_ERR_INVALID;
    *n_lines = 0;
    if (c->face_entered < 0 || c->face_entered > 6 || c->face_selected < 0 || c->face_selected > 6 || c->resolution < 1) return AIC_ERR_INVALID;
    for (int v : c->voxel_size)
        if (v < 0) return AIC_ERR_INVALID;
    aic_line_vertex *const first = out;
    const double offset = 0.001 * c->distance_to_point;  // against Z-fighting
    const double recip = 1.0 / (double)c->resolution;
    Box e;  // voxels_bounds().to_free().scale(recip).translate(cube).expand(offset)
    for (int a = 0; a < 3; a++) {
        e.lo[a] = ((double)c->voxel_lo[a] * recip + (double)c->cube[a]) - offset;
        e.hi[a] = ((double)((int64_t)c->voxel_lo[a] + c->voxel_size[a]) * recip + (double)c->cube[a]) + offset;
    }
    box_edges(e, out);
    if (c->face_selected != 0) {  // the selected face framed: the box shrunk by 1/128, flat on the expanded box's face
        const double inset = -1. / 128.;
        const int axis = (c->face_selected - 1) % 3;
        Box f;
        for (int a = 0; a < 3; a++) { f.lo[a] = e.lo[a] - inset; f.hi[a] = e.hi[a] + inset; }
        f.lo[axis] = f.hi[axis] = c->face_selected <= 3 ? e.lo[axis] : e.hi[axis];
        box_edges(f, out);
    }
    if (c->face_entered != 0) {  // the point of entry framed with a diamond in the face's plane
        // where Face::rotation_from_nz (face.rs:395-405) sends +X and +Y, as {axis, sign}: RYZX, RZXY, RXYZ, RyZx, RZxy, RXyz
        static const int kBasis[6][2][2] = {{{1, 1}, {2, 1}}, {{2, 1}, {0, 1}}, {{0, 1}, {1, 1}}, {{1, -1}, {2, 1}}, {{2, 1}, {0, -1}}, {{0, 1}, {1, -1}}};
        const int axis = (c->face_entered - 1) % 3;
        double centre[3];
        for (int a = 0; a < 3; a++) centre[a] = c->point_entered[a] + (a == axis ? (c->face_entered <= 3 ? -offset : offset) : 0.0);
        double tips[4][3];
        for (int k = 0; k < 4; k++) {  // Face7::PX, PY, NX, NY
            const int(&b)[2] = kBasis[c->face_entered - 1][k & 1];
            for (int a = 0; a < 3; a++) tips[k][a] = centre[a] + (a == b[0] ? (double)((k & 2) ? -b[1] : b[1]) / 32.0 : 0.0);
        }
        for (int k = 0; k < 4; k++)  // lines::line_loop (lines.rs:69-71)
            for (int end = 0; end < 2; end++) put(out, tips[(k + end) % 4][0], tips[(k + end) % 4][1], tips[(k + end) % 4][2]);
    }
    *n_lines = (uint32_t)((out - first) / 2);
    return AIC_OK;
}
