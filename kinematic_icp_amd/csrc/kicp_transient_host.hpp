// kicp_transient_host.hpp -- the arithmetic of the grid's transient obstacles (kicp_grid_transients, kicp_transients_from_counts;
// include/kicp.h states the semantics): the transient-cell test from a cell's returns and its counters, the key of a row's nearest
// cell, the empty row and what one cell adds to it, and the host entry's whole pass.  ONE text for the kernels (kicp_transient.hpp), for
// the entries (kicp_grid_transient.hip) and for the stand-alone program that runs transient_host:: under sanitizers
// (tests/cpp/transient_host_test.cpp).  The endpoint cell of a point is kicp_grid_host.hpp's (grid_endpoint, grid_inside); the labelling,
// the order and the filter of the output are kicp_front_host.hpp's (front_host::label, front_order).  Everything is integer.
//
// A ROW has ten words, all live while it is being summed: 0 the label, 1 the size, 2 the returns, 3 and 4 the sums of n x and n y,
// 5 .. 8 the box (min x, max x, min y, max y) and in word 9 the least key d2(c) * 2^32 + c of its cells.  Every update commutes.
#pragma once
#include "kicp_front_host.hpp"

namespace kicp {

constexpr uint32_t kTransientWords = 10;  // KICP_TRANSIENT_WORDS

struct TransientParams {
    uint32_t min_observations, free_max, min_points, min_size;  // >= 1; 0 .. 100; >= 1; >= 1
};

// n: the used points whose endpoint cell this is; pair: its counters (hits | misses << 16) as they stand
KICP_HD bool transient_is_cell(uint32_t n, uint32_t pair, const TransientParams &p) {
    const int32_t v = grid_readout(pair & 0xFFFFu, pair >> 16, p.min_observations);
    return n >= p.min_points && v >= 0 && v <= static_cast<int32_t>(p.free_max);
}
// the sensor's cell as integers: the window's lower corner plus the reach (the corner is kGridFarAway where no grid cell can be near)
KICP_HD int64_t transient_sensor(int32_t corner, int32_t reach) { return static_cast<int64_t>(corner) + reach; }
// d2 * 2^32 + cell; |x - sx|, |y - sy| <= 4095 on a cell a used point ends in, so d2 < 2^25
KICP_HD unsigned long long transient_key(uint32_t x, uint32_t y, int64_t sx, int64_t sy, uint32_t cell) {
    const int64_t dx = static_cast<int64_t>(x) - sx, dy = static_cast<int64_t>(y) - sy;
    return (static_cast<unsigned long long>(dx * dx + dy * dy) << 32) | cell;
}
// the row of a transient no cell has been added to yet
KICP_HD void transient_row_init(unsigned long long *row, uint32_t label) {
    row[0] = label, row[1] = row[2] = row[3] = row[4] = 0ull;
    row[5] = row[7] = ~0ull, row[6] = row[8] = 0ull;
    row[9] = ~0ull;
}
// one cell more (host; the kernel does the same with one atomic per word)
inline void transient_row_add(unsigned long long *row, uint32_t n, uint32_t x, uint32_t y, unsigned long long key) {
    row[1] += 1ull, row[2] += n, row[3] += static_cast<unsigned long long>(n) * x, row[4] += static_cast<unsigned long long>(n) * y;
    row[5] = std::min<unsigned long long>(row[5], x), row[6] = std::max<unsigned long long>(row[6], x);
    row[7] = std::min<unsigned long long>(row[7], y), row[8] = std::max<unsigned long long>(row[8], y);
    row[9] = std::min(row[9], key);
}
// The output of n summed rows (in any order): those of at least min_size cells in ascending label order; the first `cap` of them are
// stored.  Returns the number that passed the filter.
inline size_t transient_emit(const unsigned long long *rows, size_t n, uint32_t min_size, unsigned long long *out, size_t cap) {
    const std::vector<size_t> order = front_order(rows, n, min_size);
    for (size_t k = 0; k < order.size() && k < cap; ++k) std::copy(rows + order[k] * kTransientWords, rows + (order[k] + 1u) * kTransientWords, out + k * kTransientWords);
    return order.size();
}
static_assert(kTransientWords == kFrontWords, "front_order strides over the rows");

namespace transient_host {
// n(c) of one frame: a word per cell.  stats[0] the used points, stats[1] those whose endpoint cell lies inside the grid, stats[2] the
// cells with n(c) > 0
inline void count(const GridGeom &g, const GridFrame &f, const double *xyz, size_t n, std::vector<uint32_t> &returns, unsigned long long stats[4]) {
    returns.assign(static_cast<size_t>(g.width) * g.height, 0u);
    stats[0] = stats[1] = stats[2] = stats[3] = 0ull;
    for (size_t i = 0; i < n; ++i) {
        int32_t dx, dy;
        if (!grid_endpoint(g, f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], dx, dy)) continue;
        ++stats[0];
        size_t c;
        if (!grid_inside(g, f, static_cast<uint32_t>(dx + g.reach), static_cast<uint32_t>(dy + g.reach), c)) continue;
        ++stats[1];
        if (returns[c]++ == 0u) ++stats[2];
    }
}
// The whole host entry over counters in kicp_grid_counts' layout.  out_labels (width * height words), out_plane (a byte per cell) and
// stats (four words) are nullable.  Returns the number of transients that passed the filter.
inline size_t transients(const GridGeom &g, const uint16_t *counts, const double *xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                         const TransientParams &p, unsigned long long *out_rows, size_t cap_rows, uint32_t *out_labels, uint8_t *out_plane, unsigned long long *out_stats) {
    const GridFrame f = grid_frame(g, pose_qt, sensor_xyz);
    const size_t cells = static_cast<size_t>(g.width) * g.height;
    const int64_t sx = transient_sensor(f.gx0, g.reach), sy = transient_sensor(f.gy0, g.reach);
    std::vector<uint32_t> returns, labels, row_of(cells, 0u);
    std::vector<uint8_t> flags(cells, 0u);
    std::vector<unsigned long long> summed;
    unsigned long long stats[4];
    count(g, f, xyz, n, returns, stats);
    for (size_t c = 0; c < cells; ++c) {
        if (!returns[c]) continue;
        flags[c] = transient_is_cell(returns[c], static_cast<uint32_t>(counts[2 * c]) | static_cast<uint32_t>(counts[2 * c + 1]) << 16, p) ? 1u : 0u;
        stats[3] += flags[c];
    }
    front_host::label(flags, g.width, g.height, labels);
    for (size_t c = 0; c < cells; ++c) {  // ascending: a root is met before the other cells of its component
        if (!flags[c]) continue;
        const uint32_t cell = static_cast<uint32_t>(c), x = cell % g.width, y = cell / g.width;
        if (labels[c] == cell) {
            row_of[c] = static_cast<uint32_t>(summed.size() / kTransientWords);
            summed.resize(summed.size() + kTransientWords);
            transient_row_init(summed.data() + summed.size() - kTransientWords, cell);
        }
        transient_row_add(summed.data() + static_cast<size_t>(row_of[labels[c]]) * kTransientWords, returns[c], x, y, transient_key(x, y, sx, sy, cell));
    }
    if (out_plane)
        for (size_t c = 0; c < cells; ++c) out_plane[c] = flags[c] && summed[static_cast<size_t>(row_of[labels[c]]) * kTransientWords + 1u] >= p.min_size ? 1u : 0u;
    if (out_labels) std::copy(labels.begin(), labels.end(), out_labels);
    if (out_stats) std::copy(stats, stats + 4, out_stats);
    return transient_emit(summed.data(), summed.size() / kTransientWords, p.min_size, out_rows, cap_rows);
}
}  // namespace transient_host

}  // namespace kicp
