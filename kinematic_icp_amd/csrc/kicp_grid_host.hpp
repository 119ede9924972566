// kicp_grid_host.hpp -- the geometry of the 2-D occupancy grid (kicp_grid_*, include/kicp.h): the cell of a coordinate, one step of
// the ray walk, the readout of one cell, the pixel of one value and the fill of one unknown cell from another grid.  ONE text for the
// kernels (kicp_grid.hpp), for the pure-host entries (kicp_grid_occupancy_from_counts, kicp_grid_write_map,
// kicp_grid_fill_unknown_counts) and for grid_host::integrate and grid_host::fill_unknown, the host restatements that stand-alone
// programs run under sanitizers (tests/cpp/grid_host_test.cpp, tests/cpp/elev_rough_host_test.cpp).  Everything is exact and integer
// from the floor on.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "kicp_se3.hpp"

namespace kicp {

constexpr uint32_t kGridSaturated = 65535u;     // both counters of a cell stop here
constexpr int32_t kGridMaxReach = 4095;         // cells: keeps 2 * k * a + m inside 32 bits and a frame's window at or below 2^26 cells
constexpr uint64_t kGridMaxCells = 1ull << 28;  // width * height
constexpr int32_t kGridFarAway = -(1 << 30);    // window corner of a sensor whose cell no grid can be near: every window cell is outside

struct GridGeom {
    double cell, origin_x, origin_y, z_min, z_max;
    uint32_t width, height;
    int32_t reach;  // ceil(max_ray / cell)
};
// One frame's constants, evaluated on the host: rows 0 and 1 of pose_to_rt's R and t, the sensor's cell (integer valued doubles; not
// finite when the pose or the sensor origin is not) and the grid index of the window's lower corner (window cell (wx, wy) is grid
// cell (gx0 + wx, gy0 + wy); the window is the (2 reach + 1)^2 square around the sensor's cell).
struct GridFrame {
    double r[6], t[2];
    double sx, sy;
    int32_t gx0, gy0;
};

// ((r0 p.x + r1 p.y) + r2 p.z) + t0, every operation rounded on its own (-ffp-contract=off)
KICP_HD double grid_world(const double *r, double t, double px, double py, double pz) { return ((r[0] * px + r[1] * py) + r[2] * pz) + t; }
KICP_HD double grid_cell(double w, double origin, double cell) { return floor((w - origin) / cell); }
// Is the point used, and if so where is its endpoint cell relative to the sensor's (|dx|, |dy| <= reach)?  Used: finite coordinates,
// z_min <= p.z < z_max in the base frame, finite world coordinates, and an endpoint cell within `reach` of the sensor's cell
// (Chebyshev).  A comparison with a NaN is false, so a sensor cell that is not finite uses no point.
KICP_HD bool grid_endpoint(const GridGeom &g, const GridFrame &f, double px, double py, double pz, int32_t &dx, int32_t &dy) {
    if (!(fabs(px) <= DBL_MAX && fabs(py) <= DBL_MAX && fabs(pz) <= DBL_MAX)) return false;
    if (!(g.z_min <= pz && pz < g.z_max)) return false;
    const double wx = grid_world(f.r, f.t[0], px, py, pz), wy = grid_world(f.r + 3, f.t[1], px, py, pz);
    if (!(fabs(wx) <= DBL_MAX && fabs(wy) <= DBL_MAX)) return false;
    const double ox = grid_cell(wx, g.origin_x, g.cell) - f.sx, oy = grid_cell(wy, g.origin_y, g.cell) - f.sy;
    const double reach = static_cast<double>(g.reach);
    if (!(fabs(ox) <= reach && fabs(oy) <= reach)) return false;
    dx = static_cast<int32_t>(ox), dy = static_cast<int32_t>(oy);
    return true;
}
// Step k (0 <= k < m) of the walk from the sensor's cell to the endpoint cell at offset (dx, dy), m = max(|dx|, |dy|) >= 1: the
// visited cell's offset from the sensor's cell.  Integer divisions of non-negative numbers; 2 k a + m < 2^26 for m <= 4095.
KICP_HD void grid_step(int32_t dx, int32_t dy, uint32_t m, uint32_t k, int32_t &ox, int32_t &oy) {
    const uint32_t a = static_cast<uint32_t>(dx < 0 ? -dx : dx), b = static_cast<uint32_t>(dy < 0 ? -dy : dy);
    const int32_t sa = static_cast<int32_t>((2u * k * a + m) / (2u * m)), sb = static_cast<int32_t>((2u * k * b + m) / (2u * m));
    ox = dx < 0 ? -sa : sa, oy = dy < 0 ? -sb : sb;
}
KICP_HD uint32_t grid_walk_length(int32_t dx, int32_t dy) {
    const uint32_t a = static_cast<uint32_t>(dx < 0 ? -dx : dx), b = static_cast<uint32_t>(dy < 0 ? -dy : dy);
    return a > b ? a : b;
}
KICP_HD uint16_t grid_bump(uint16_t v) { return v >= kGridSaturated ? static_cast<uint16_t>(kGridSaturated) : static_cast<uint16_t>(v + 1u); }
// the readout of one cell: -1 below min_observations, else round(100 hits / (hits + misses)), ties up, in integers
KICP_HD int8_t grid_readout(uint32_t hits, uint32_t misses, uint32_t min_observations) {
    const uint32_t seen = hits + misses;
    if (seen < min_observations || seen == 0u) return static_cast<int8_t>(-1);
    return static_cast<int8_t>((100u * hits + seen / 2u) / seen);
}
// the pixel of one value in the trinary map image: 0 occupied, 254 free, 205 neither (unknown cells too)
KICP_HD uint8_t grid_pixel(int8_t value, double occupied_thresh, double free_thresh) {
    const double v = static_cast<double>(value);
    if (v > occupied_thresh * 100.0) return 0u;
    if (value >= 0 && v < free_thresh * 100.0) return 254u;
    return 205u;
}

// ---- the fill of one grid's unknown cells from another (kicp_grid_fill_unknown*) ---------------------------------------------------
constexpr uint32_t kGridFillCounts = 7;
struct GridFillParams {
    uint32_t min_observations, free_max, occupied_min;  // >= 1; free_max <= 100; free_max < occupied_min <= 101
};
// One cell: the pairs (hits | misses << 16) of the destination and the source -> the destination's pair afterwards.  `which` is the
// tally the cell adds to - 0 kept obstacle, 1 kept traversable, 2 filled free, 3 filled occupied, 4 left unknown - and `disagree` 0, or
// 5: traversable over a source OCCUPIED, or 6: obstacle over a source FREE.  Only an unknown destination (0, 0) changes: to (0, 1) where
// the source is FREE, to (1, 0) where it is OCCUPIED.
KICP_HD uint32_t grid_fill_pair(uint32_t dst, uint32_t src, const GridFillParams &p, uint32_t &which, uint32_t &disagree) {
    const int32_t v = grid_readout(src & 0xFFFFu, src >> 16, p.min_observations);
    const bool is_free = v >= 0 && v <= static_cast<int32_t>(p.free_max), is_occupied = v >= static_cast<int32_t>(p.occupied_min);
    disagree = 0u;
    if (dst & 0xFFFFu) {  // an obstacle
        which = 0u, disagree = is_free ? 6u : 0u;
        return dst;
    }
    if (dst) {  // traversable
        which = 1u, disagree = is_occupied ? 5u : 0u;
        return dst;
    }
    which = is_free ? 2u : is_occupied ? 3u : 4u;
    return is_free ? 0x10000u : is_occupied ? 1u : 0u;
}

// the frame constants of a pose and a sensor origin (host: pose_to_rt is evaluated here, once per frame)
inline GridFrame grid_frame(const GridGeom &g, const double pose_qt[7], const double sensor_xyz[3]) {
    const Rt m = pose_to_rt(Pose{pose_qt[0], pose_qt[1], pose_qt[2], pose_qt[3], pose_qt[4], pose_qt[5], pose_qt[6]});
    GridFrame f;
    for (int i = 0; i < 6; ++i) f.r[i] = m.r[i];
    f.t[0] = m.t[0], f.t[1] = m.t[1];
    f.sx = grid_cell(grid_world(f.r, f.t[0], sensor_xyz[0], sensor_xyz[1], sensor_xyz[2]), g.origin_x, g.cell);
    f.sy = grid_cell(grid_world(f.r + 3, f.t[1], sensor_xyz[0], sensor_xyz[1], sensor_xyz[2]), g.origin_y, g.cell);
    auto corner = [&](double s) {
        const double c = s - static_cast<double>(g.reach);
        return (c >= -1073741824.0 && c <= 1073741824.0) ? static_cast<int32_t>(c) : kGridFarAway;
    };
    f.gx0 = corner(f.sx), f.gy0 = corner(f.sy);
    return f;
}
KICP_HD bool grid_inside(const GridGeom &g, const GridFrame &f, uint32_t wx, uint32_t wy, size_t &cell_index) {
    const int64_t gx = static_cast<int64_t>(f.gx0) + wx, gy = static_cast<int64_t>(f.gy0) + wy;
    if (gx < 0 || gy < 0 || gx >= static_cast<int64_t>(g.width) || gy >= static_cast<int64_t>(g.height)) return false;
    cell_index = static_cast<size_t>(gy) * g.width + static_cast<size_t>(gx);
    return true;
}

namespace grid_host {
// One frame on the host, as the three kernels do it: mark the endpoint cells in a hit plane over the window, walk one ray per marked
// cell into a miss plane, then bump the counters of window cells inside the grid - hit wins over miss.  counts: cells x 2 (hits,
// misses).  stats: points used, points skipped, cells HIT, cells MISS.
inline void integrate(const GridGeom &g, uint16_t *counts, const double *xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                      unsigned long long stats[4]) {
    const GridFrame f = grid_frame(g, pose_qt, sensor_xyz);
    const uint32_t side = 2u * static_cast<uint32_t>(g.reach) + 1u;
    std::vector<uint8_t> hit(static_cast<size_t>(side) * side, 0), miss(static_cast<size_t>(side) * side, 0);
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    for (size_t i = 0; i < n; ++i) {
        int32_t dx, dy;
        if (!grid_endpoint(g, f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], dx, dy)) {
            ++stats[1];
            continue;
        }
        ++stats[0];
        hit[static_cast<size_t>(dy + g.reach) * side + static_cast<size_t>(dx + g.reach)] = 1;
    }
    for (uint32_t wy = 0; wy < side; ++wy)
        for (uint32_t wx = 0; wx < side; ++wx) {
            if (!hit[static_cast<size_t>(wy) * side + wx]) continue;
            const int32_t dx = static_cast<int32_t>(wx) - g.reach, dy = static_cast<int32_t>(wy) - g.reach;
            const uint32_t m = grid_walk_length(dx, dy);
            for (uint32_t k = 0; k < m; ++k) {
                int32_t ox, oy;
                grid_step(dx, dy, m, k, ox, oy);
                miss[static_cast<size_t>(oy + g.reach) * side + static_cast<size_t>(ox + g.reach)] = 1;
            }
        }
    for (uint32_t wy = 0; wy < side; ++wy)
        for (uint32_t wx = 0; wx < side; ++wx) {
            const size_t w = static_cast<size_t>(wy) * side + wx;
            size_t c;
            if (!(hit[w] | miss[w]) || !grid_inside(g, f, wx, wy, c)) continue;
            if (hit[w])
                counts[2 * c] = grid_bump(counts[2 * c]), ++stats[2];
            else
                counts[2 * c + 1] = grid_bump(counts[2 * c + 1]), ++stats[3];
        }
}
// The fill on the host, as k_grid_fill_unknown does it: dst and src are cells x 2 counters (hits, misses); a counter is written only
// where its cell changes.  counts (nullable): the seven words.
inline void fill_unknown(uint16_t *dst, const uint16_t *src, size_t cells, const GridFillParams &p, unsigned long long counts[7]) {
    unsigned long long sums[kGridFillCounts] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < cells; ++i) {
        const uint32_t d = static_cast<uint32_t>(dst[2 * i]) | static_cast<uint32_t>(dst[2 * i + 1]) << 16;
        const uint32_t s = static_cast<uint32_t>(src[2 * i]) | static_cast<uint32_t>(src[2 * i + 1]) << 16;
        uint32_t which, disagree;
        const uint32_t after = grid_fill_pair(d, s, p, which, disagree);
        if (after != d) dst[2 * i] = static_cast<uint16_t>(after & 0xFFFFu), dst[2 * i + 1] = static_cast<uint16_t>(after >> 16);
        ++sums[which];
        if (disagree) ++sums[disagree];
    }
    if (counts)
        for (uint32_t k = 0; k < kGridFillCounts; ++k) counts[k] = sums[k];
}
}  // namespace grid_host

}  // namespace kicp
