// kicp_clear_host.hpp -- the arithmetic of the grid's clearance and costmap (kicp_grid_clearance, kicp_grid_costmap; include/kicp.h
// states the semantics): the class of a readout value, one step of a column sweep, the scan of one row and the cost of one cell.  ONE
// text for the kernels (kicp_clear.hpp), for the pure-host entries (kicp_grid_*_from_occupancy, kicp_grid_cost_table_nav2) and for the
// stand-alone program that runs clear_host:: under sanitizers (tests/cpp/clear_host_test.cpp).  Everything but the cost table is
// integer: the threshold comparison in doubles is folded on the host into the smallest readout value that is a source.
//
// The transform is separable.  g(x, y), the COLUMN DISTANCE, is the vertical distance from (x, y) to the nearest source of column x,
// 255 when there is none within R; then c(x, y) = min over k of k^2 + g(x + k, y)^2, capped at R^2 + 1.  255^2 > 254^2 + 1, so the
// "none" value needs no test of its own.
#pragma once
#include <algorithm>
#include <vector>

#include "kicp_grid_host.hpp"

namespace kicp {

constexpr int32_t kClearMaxRadius = 254;  // a column distance fits a byte beside the 255 of "none"; R^2 + 1 = 64 517 fits 16 bits
constexpr uint32_t kClearNone = 255u;     // column distance: no source of this column within R
constexpr uint32_t kClearSegment = 256u;  // cells of a row that one workgroup of k_clear_rows scans

enum : uint32_t { kClearClear = 0u, kClearUnknown = 1u, kClearSource = 2u };

struct ClearParams {
    uint32_t min_observations;
    int32_t source_min;            // the smallest readout value v with (double)v > occupied_thresh * 100.0; 101 when none is
    uint32_t unknown_is_obstacle;  // 0 / 1
    uint32_t radius;               // R, 1 .. 254
};
struct ClearRect {
    uint32_t x0, y0, w, h;
};

// (double)v > occupied_thresh * 100.0 is monotone in v, so it is v >= source_min (occupied_thresh in [0, 1]: 101 passes)
inline int32_t clear_source_min(double occupied_thresh) {
    int32_t v = 0;
    while (v <= 100 && !(static_cast<double>(v) > occupied_thresh * 100.0)) ++v;
    return v;
}
KICP_HD uint32_t clear_class(int8_t v, int32_t source_min) { return v >= source_min ? kClearSource : v < 0 ? kClearUnknown : kClearClear; }
KICP_HD bool clear_is_source(uint32_t cls, uint32_t unknown_is_obstacle) { return cls == kClearSource || (unknown_is_obstacle && cls == kClearUnknown); }
// one step of a column sweep: the distance to the last source met, saturating at "none"
KICP_HD uint32_t clear_sweep(uint32_t d, bool source) { return source ? 0u : d >= kClearNone ? kClearNone : d + 1u; }
KICP_HD uint32_t clear_far(uint32_t radius) { return radius * radius + 1u; }
// The clearance of one cell from the column distances of its row: g points at the cell's own, g[-R .. R] are readable (255 for
// columns outside the grid).  Scans outwards and stops once k^2 alone reaches the best so far.
KICP_HD uint32_t clear_row_scan(const uint8_t *g, uint32_t radius) {
    const uint32_t own = g[0];
    uint32_t best = own * own < clear_far(radius) ? own * own : clear_far(radius);
    for (uint32_t k = 1; k <= radius && k * k < best; ++k) {
        const uint32_t a = g[-static_cast<int32_t>(k)], b = g[k], m = a < b ? a : b;
        const uint32_t c = k * k + m * m;
        best = c < best ? c : best;
    }
    return best;
}
// The cost of one cell: t = table[clearance]; Nav2's inflation layer (nav2_costmap_2d InflationLayer::updateCosts) over a master grid
// of 254 lethal / 255 no information / 0 free: an unknown cell takes t only when inflate_unknown ? t > 0 : t >= 253, every other cell
// max(its own cost, t).
KICP_HD uint8_t clear_cost(uint32_t cls, uint32_t unknown_is_obstacle, uint32_t t, uint32_t inflate_unknown) {
    if (clear_is_source(cls, unknown_is_obstacle)) return static_cast<uint8_t>(t > 254u ? t : 254u);
    if (cls == kClearUnknown) return static_cast<uint8_t>((inflate_unknown ? t > 0u : t >= 253u) ? t : 255u);
    return static_cast<uint8_t>(t);
}

namespace clear_host {
// the column range a rectangle's rows need: the rectangle grown by R in x, clipped to the grid
inline void column_range(uint32_t width, const ClearRect &r, uint32_t radius, uint32_t &cx0, uint32_t &cx1) {
    cx0 = r.x0 > radius ? r.x0 - radius : 0u;
    cx1 = static_cast<uint32_t>(std::min<uint64_t>(width, static_cast<uint64_t>(r.x0) + r.w + radius));
}
// Column distances of the rectangle's rows over columns cx0 .. cx1: a sweep down from R rows below the rectangle, a sweep up from R
// rows above it, the smaller of the two, "none" beyond R.  out: r.h rows of (cx1 - cx0).
inline void columns(const int8_t *occupancy, uint32_t width, uint32_t height, const ClearParams &p, const ClearRect &r, uint32_t cx0, uint32_t cx1,
                    std::vector<uint8_t> &out) {
    const size_t cw = cx1 - cx0;
    out.assign(cw * r.h, static_cast<uint8_t>(kClearNone));
    const uint32_t lo = r.y0 > p.radius ? r.y0 - p.radius : 0u;
    const uint32_t hi = static_cast<uint32_t>(std::min<uint64_t>(height, static_cast<uint64_t>(r.y0) + r.h + p.radius));
    auto source = [&](uint32_t x, uint32_t y) { return clear_is_source(clear_class(occupancy[static_cast<size_t>(y) * width + x], p.source_min), p.unknown_is_obstacle); };
    for (uint32_t x = cx0; x < cx1; ++x) {
        uint32_t d = kClearNone;
        for (uint32_t y = lo; y < r.y0 + r.h; ++y) {
            d = clear_sweep(d, source(x, y));
            if (y >= r.y0) out[(y - r.y0) * cw + (x - cx0)] = static_cast<uint8_t>(d);
        }
        d = kClearNone;
        for (uint32_t y = hi; y-- > r.y0;) {
            uint8_t &o = out[(y < r.y0 + r.h ? y - r.y0 : 0u) * cw + (x - cx0)];
            d = clear_sweep(d, y < r.y0 + r.h ? o == 0u : source(x, y));
            if (y < r.y0 + r.h) {
                const uint32_t m = std::min<uint32_t>(o, d);
                o = static_cast<uint8_t>(m > p.radius ? kClearNone : m);
            }
        }
    }
}
// one row of the rectangle: its column distances padded with "none" to R columns on both sides of the rectangle
inline void padded_row(const std::vector<uint8_t> &col, uint32_t cx0, uint32_t cx1, const ClearRect &r, uint32_t radius, uint32_t row, std::vector<uint8_t> &padded) {
    padded.assign(static_cast<size_t>(r.w) + 2u * radius, static_cast<uint8_t>(kClearNone));
    const size_t cw = cx1 - cx0;
    for (uint32_t x = cx0; x < cx1; ++x) padded[x + radius - r.x0] = col[row * cw + (x - cx0)];
}
inline void clearance(const int8_t *occupancy, uint32_t width, uint32_t height, const ClearParams &p, const ClearRect &r, uint16_t *out) {
    uint32_t cx0, cx1;
    column_range(width, r, p.radius, cx0, cx1);
    std::vector<uint8_t> col, padded;
    columns(occupancy, width, height, p, r, cx0, cx1, col);
    for (uint32_t row = 0; row < r.h; ++row) {
        padded_row(col, cx0, cx1, r, p.radius, row, padded);
        for (uint32_t i = 0; i < r.w; ++i) out[static_cast<size_t>(row) * r.w + i] = static_cast<uint16_t>(clear_row_scan(padded.data() + p.radius + i, p.radius));
    }
}
inline void costmap(const int8_t *occupancy, uint32_t width, uint32_t height, const ClearParams &p, const uint8_t *table, uint32_t inflate_unknown,
                    const ClearRect &r, uint8_t *out) {
    uint32_t cx0, cx1;
    column_range(width, r, p.radius, cx0, cx1);
    std::vector<uint8_t> col, padded;
    columns(occupancy, width, height, p, r, cx0, cx1, col);
    for (uint32_t row = 0; row < r.h; ++row) {
        padded_row(col, cx0, cx1, r, p.radius, row, padded);
        for (uint32_t i = 0; i < r.w; ++i) {
            const uint32_t cls = clear_class(occupancy[static_cast<size_t>(r.y0 + row) * width + r.x0 + i], p.source_min);
            out[static_cast<size_t>(row) * r.w + i] = clear_cost(cls, p.unknown_is_obstacle, table[clear_row_scan(padded.data() + p.radius + i, p.radius)], inflate_unknown);
        }
    }
}
// the table of Nav2's inflation layer: table[0 .. R^2 + 1]
inline void cost_table_nav2(double cell, uint32_t radius, double inscribed_radius, double cost_scaling_factor, uint8_t *table) {
    table[0] = 254u, table[clear_far(radius)] = 0u;
    for (uint32_t d2 = 1; d2 <= radius * radius; ++d2) {
        const double d = std::sqrt(static_cast<double>(d2)) * cell;
        table[d2] = d <= inscribed_radius ? static_cast<uint8_t>(253u) : static_cast<uint8_t>(252.0 * std::exp(-cost_scaling_factor * (d - inscribed_radius)));
    }
}
}  // namespace clear_host

}  // namespace kicp
