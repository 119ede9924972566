// kicp_elev_host.hpp -- the arithmetic of the height columns (kicp_elev_*, include/kicp.h): the class of one point, the ground of one
// column, BODY and STEP of one cell.  ONE text for the kernels (kicp_elev.hpp), for the pure-host entry
// (kicp_elev_traversability_from_columns) and for elev_host::integrate / elev_host::classify, the host restatements that a
// stand-alone program runs under sanitizers (tests/cpp/elev_host_test.cpp).  Everything is exact and integer from the floor on.
#pragma once
#include "kicp_grid_host.hpp"

namespace kicp {

constexpr uint32_t kElevSlabs = 64;      // bits of a column
constexpr uint8_t kElevNoGround = 255u;  // the ground byte of an empty column
constexpr uint32_t kElevMaxStep = 62;    // step_slabs; step_slabs < robot_slabs <= 64

// the layer's geometry: the plane is the grid's (its band is not used: every return counts), the vertical is z_origin + b * slab
struct ElevGeom {
    GridGeom plane;
    double z_origin, slab;
};
// One frame's constants: the grid's (rows 0 and 1, the sensor's cell, the window's corner) and row 2 of pose_to_rt's R and t.
struct ElevFrame {
    GridFrame plane;
    double r2[3], t2;
};
struct ElevParams {
    uint32_t step_slabs, robot_slabs;  // S, H: 0 <= S <= 62, S < H <= 64
};
struct ElevRect {
    uint32_t x0, y0, w, h;
};

enum ElevClass : int { kElevSkipped = 0, kElevOutsideGrid = 1, kElevOutsideColumn = 2, kElevUsed = 3 };

// The class of one point, tested in the header's order; for a used point the cell's index and the slab.  Every comparison is made on
// doubles before any conversion, and a comparison with a NaN is false: a sensor cell that is not finite skips everything.
KICP_HD ElevClass elev_point(const ElevGeom &g, const ElevFrame &f, double px, double py, double pz, size_t &cell_index, uint32_t &slab) {
    if (!(fabs(px) <= DBL_MAX && fabs(py) <= DBL_MAX && fabs(pz) <= DBL_MAX)) return kElevSkipped;
    const double wx = grid_world(f.plane.r, f.plane.t[0], px, py, pz), wy = grid_world(f.plane.r + 3, f.plane.t[1], px, py, pz);
    const double wz = grid_world(f.r2, f.t2, px, py, pz);
    if (!(fabs(wx) <= DBL_MAX && fabs(wy) <= DBL_MAX && fabs(wz) <= DBL_MAX)) return kElevSkipped;
    const double cx = grid_cell(wx, g.plane.origin_x, g.plane.cell), cy = grid_cell(wy, g.plane.origin_y, g.plane.cell);
    const double reach = static_cast<double>(g.plane.reach);
    if (!(fabs(cx - f.plane.sx) <= reach && fabs(cy - f.plane.sy) <= reach)) return kElevSkipped;
    if (!(cx >= 0.0 && cx < static_cast<double>(g.plane.width) && cy >= 0.0 && cy < static_cast<double>(g.plane.height))) return kElevOutsideGrid;
    const double s = floor((wz - g.z_origin) / g.slab);
    if (!(s >= 0.0 && s <= 63.0)) return kElevOutsideColumn;
    cell_index = static_cast<size_t>(cy) * g.plane.width + static_cast<size_t>(cx);
    slab = static_cast<uint32_t>(s);
    return kElevUsed;
}

// the frame constants of a pose and a sensor origin (host: pose_to_rt is evaluated here, once per frame)
inline ElevFrame elev_frame(const ElevGeom &g, const double pose_qt[7], const double sensor_xyz[3]) {
    const Rt m = pose_to_rt(Pose{pose_qt[0], pose_qt[1], pose_qt[2], pose_qt[3], pose_qt[4], pose_qt[5], pose_qt[6]});
    ElevFrame f;
    f.plane = grid_frame(g.plane, pose_qt, sensor_xyz);
    f.r2[0] = m.r[6], f.r2[1] = m.r[7], f.r2[2] = m.r[8], f.t2 = m.t[2];
    return f;
}

// bits lo .. 63 of a column; lo reaches 64 and beyond (g + S + 1, g + H + 1), where a shift is undefined in C++ and modulo 64 on the
// hardware: there the set is empty
KICP_HD uint64_t elev_bits_from(uint32_t lo) { return lo >= kElevSlabs ? 0ull : ~0ull << lo; }
// the ground of a column: the index of its lowest set bit, 255 for an empty one
KICP_HD uint8_t elev_ground(uint64_t column) { return column ? static_cast<uint8_t>(__builtin_ctzll(column)) : kElevNoGround; }
// BODY: some bit b of the column with g + S < b <= g + H (g its ground; the column is not empty)
KICP_HD bool elev_body(uint64_t column, uint32_t ground, const ElevParams &p) {
    return (column & elev_bits_from(ground + p.step_slabs + 1u) & ~elev_bits_from(ground + p.robot_slabs + 1u)) != 0ull;
}
// STEP against one neighbour: it is known and its ground lies more than S slabs below this cell's
KICP_HD bool elev_step(uint32_t ground, uint8_t neighbour_ground, const ElevParams &p) {
    return neighbour_ground != kElevNoGround && ground > static_cast<uint32_t>(neighbour_ground) + p.step_slabs;
}
// the value of a cell and the count it adds to: 0 unknown, 1 traversable, 2 BODY, 3 STEP only
KICP_HD int8_t elev_value(bool known, bool body, bool step, uint32_t &which) {
    which = !known ? 0u : body ? 2u : step ? 3u : 1u;
    return !known ? static_cast<int8_t>(-1) : static_cast<int8_t>((body || step) ? 100 : 0);
}

namespace elev_host {
// One frame on the host, as k_elev_mark does it.  columns: one 64-bit word per cell.  stats: used, skipped, outside_grid,
// outside_column, new_bits, new_cells.
inline void integrate(const ElevGeom &g, uint64_t *columns, const double *xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                      unsigned long long stats[6]) {
    const ElevFrame f = elev_frame(g, pose_qt, sensor_xyz);
    for (int k = 0; k < 6; ++k) stats[k] = 0;
    for (size_t i = 0; i < n; ++i) {
        size_t c = 0;
        uint32_t s = 0;
        switch (elev_point(g, f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], c, s)) {
            case kElevSkipped: ++stats[1]; break;
            case kElevOutsideGrid: ++stats[2]; break;
            case kElevOutsideColumn: ++stats[3]; break;
            case kElevUsed: {
                ++stats[0];
                const uint64_t bit = 1ull << s;
                if (!(columns[c] & bit)) ++stats[4];
                if (!columns[c]) ++stats[5];
                columns[c] |= bit;
            }
        }
    }
}
// The classes of a rectangle (inside the grid; checked by the caller), as k_elev_classify computes them: out and ground (nullable) are
// h * w values, row-major from (x0, y0); counts (nullable): unknown, traversable, BODY, STEP only.
inline void classify(const uint64_t *columns, uint32_t width, uint32_t height, const ElevParams &p, const ElevRect &r, int8_t *out, uint8_t *ground,
                     unsigned long long counts[4]) {
    unsigned long long sums[4] = {0, 0, 0, 0};
    for (uint32_t ry = 0; ry < r.h; ++ry)
        for (uint32_t rx = 0; rx < r.w; ++rx) {
            const uint32_t x = r.x0 + rx, y = r.y0 + ry;
            const uint64_t c = columns[static_cast<size_t>(y) * width + x];
            const uint8_t gr = elev_ground(c);
            bool body = false, step = false;
            if (c) {
                body = elev_body(c, gr, p);
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int64_t nx = static_cast<int64_t>(x) + dx, ny = static_cast<int64_t>(y) + dy;
                        if ((dx == 0 && dy == 0) || nx < 0 || ny < 0 || nx >= static_cast<int64_t>(width) || ny >= static_cast<int64_t>(height)) continue;
                        step = step || elev_step(gr, elev_ground(columns[static_cast<size_t>(ny) * width + static_cast<size_t>(nx)]), p);
                    }
            }
            uint32_t which;
            const size_t o = static_cast<size_t>(ry) * r.w + rx;
            out[o] = elev_value(c != 0ull, body, step, which);
            if (ground) ground[o] = gr;
            ++sums[which];
        }
    if (counts)
        for (int k = 0; k < 4; ++k) counts[k] = sums[k];
}
}  // namespace elev_host

}  // namespace kicp
