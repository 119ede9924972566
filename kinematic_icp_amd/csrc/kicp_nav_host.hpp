// kicp_nav_host.hpp -- the arithmetic of the cost-to-go field over a costmap and of the path it yields (kicp_potential_*,
// kicp_grid_potential*; include/kicp.h states the semantics): the weight of a step, the saturating add, one cell's relaxation and one
// step of the path.  ONE text for the kernels (kicp_nav.hpp), for the pure-host entries (kicp_plan_weights, kicp_potential_from_costmap,
// kicp_potential_path) and for the stand-alone program that runs nav_host:: under sanitizers (tests/cpp/nav_host_test.cpp).  Integers
// only.
//
// q(c) = weight[costmap[c]] is a byte per cell, 0 for impassable.  The potential is the fixed point of
//   pot(c) = min(pot(c), nav_add(pot(n), nav_edge(q(c), q(n)))) over the passable neighbours n,   pot(goal) = 0
// and nav_add saturates at max_potential.  A saturating add is monotone, so the fixed point is min(D, max_potential) with D the least
// sum of edge weights: the host computes D by Dijkstra in 64 bits and clamps at the end, the device relaxes the clamped recurrence.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <queue>
#include <utility>
#include <vector>

#include "kicp_common.hpp"

namespace kicp {

constexpr uint32_t kNavUnreached = 0xFFFFFFFFu;     // impassable cells and cells no path reaches
constexpr uint32_t kNavMaxPotential = 0xFFFFFFFEu;  // the largest max_potential
constexpr uint32_t kNavTile = 32u;                  // a workgroup of k_nav_relax owns kNavTile x kNavTile cells

// the neighbours in the path's order: +x, -x, +y, -y, (+x, +y), (-x, +y), (+x, -y), (-x, -y); the last four are diagonal
KICP_HD int32_t nav_dx(uint32_t k) { return k == 0u || k == 4u || k == 6u ? 1 : k == 2u || k == 3u ? 0 : -1; }
KICP_HD int32_t nav_dy(uint32_t k) { return k < 2u ? 0 : k == 2u || k == 4u || k == 5u ? 1 : -1; }
// the weight of a step between two passable cells: s = q(u) + q(v) for an orthogonal step, (181 s + 64) >> 7 for a diagonal one
// (181 / 128 = 1.4140625); symmetric, 2 .. 721
KICP_HD uint32_t nav_edge(uint32_t qu, uint32_t qv, bool diagonal) {
    const uint32_t s = qu + qv;
    return diagonal ? (181u * s + 64u) >> 7 : s;
}
// pot + edge, saturating at max_potential; pot <= max_potential
KICP_HD uint32_t nav_add(uint32_t pot, uint32_t edge, uint32_t max_potential) { return edge >= max_potential - pot ? max_potential : pot + edge; }
// One cell's relaxation: the least of `own` and what the neighbour in direction k offers.  qn == 0: impassable or outside the grid.
KICP_HD uint32_t nav_relax(uint32_t own, uint32_t q, uint32_t qn, uint32_t pn, uint32_t k, uint32_t max_potential) {
    if (qn == 0u || pn == kNavUnreached) return own;
    const uint32_t c = nav_add(pn, nav_edge(q, qn, k >= 4u), max_potential);
    return c < own ? c : own;
}
// One step of the path: is the neighbour (potential pn, weight qn) the next cell after one of potential `own` and weight q?
KICP_HD bool nav_descends(uint32_t own, uint32_t q, uint32_t qn, uint32_t pn, uint32_t k) {
    return qn != 0u && pn != kNavUnreached && pn < own && own - pn == nav_edge(q, qn, k >= 4u);
}

namespace nav_host {
// kicp_plan_weights' table (arguments checked)
inline void weights(uint32_t neutral, uint32_t factor_num, uint32_t factor_den, uint32_t lethal_from, uint32_t unknown_weight, uint8_t out[256]) {
    for (uint32_t b = 0; b < 255u; ++b)
        out[b] = b < lethal_from ? static_cast<uint8_t>(std::min<uint64_t>(255u, neutral + static_cast<uint64_t>(b) * factor_num / factor_den)) : static_cast<uint8_t>(0u);
    out[255] = static_cast<uint8_t>(unknown_weight);
}
// The potential of every cell by Dijkstra with 64-bit sums, clamped at the end.  goals: n pairs (x, y), all inside the grid.
// stats: goals used, cells below max_potential, cells equal to it, 0.
inline void potential(const uint8_t *costmap, uint32_t width, uint32_t height, const uint8_t *weight, uint32_t max_potential, const uint32_t *goals, size_t n_goals,
                      uint32_t *out, unsigned long long stats[4]) {
    const size_t cells = static_cast<size_t>(width) * height;
    constexpr uint64_t kFar = ~0ull;
    std::vector<uint64_t> dist(cells, kFar);
    using Entry = std::pair<uint64_t, size_t>;
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
    stats[0] = stats[1] = stats[2] = stats[3] = 0ull;
    for (size_t g = 0; g < n_goals; ++g) {
        const size_t c = static_cast<size_t>(goals[2 * g + 1]) * width + goals[2 * g];
        if (weight[costmap[c]] == 0u) continue;
        ++stats[0];
        if (dist[c] != 0ull) dist[c] = 0ull, heap.push(Entry(0ull, c));
    }
    while (!heap.empty()) {
        const Entry top = heap.top();
        heap.pop();
        if (top.first != dist[top.second]) continue;
        const uint32_t x = static_cast<uint32_t>(top.second % width), y = static_cast<uint32_t>(top.second / width), q = weight[costmap[top.second]];
        for (uint32_t k = 0; k < 8u; ++k) {
            const int64_t nx = static_cast<int64_t>(x) + nav_dx(k), ny = static_cast<int64_t>(y) + nav_dy(k);
            if (nx < 0 || ny < 0 || nx >= static_cast<int64_t>(width) || ny >= static_cast<int64_t>(height)) continue;
            const size_t n = static_cast<size_t>(ny) * width + static_cast<size_t>(nx);
            const uint32_t qn = weight[costmap[n]];
            if (qn == 0u) continue;
            const uint64_t d = top.first + nav_edge(q, qn, k >= 4u);
            if (d < dist[n]) dist[n] = d, heap.push(Entry(d, n));
        }
    }
    for (size_t c = 0; c < cells; ++c) {
        out[c] = dist[c] == kFar ? kNavUnreached : static_cast<uint32_t>(std::min<uint64_t>(dist[c], max_potential));
        if (dist[c] != kFar) ++stats[dist[c] < max_potential ? 1 : 2];
    }
}
// The path from (x, y) down the potential.  Returns 0 with *out_n cells (the first min(*out_n, cap) of them stored as (x, y) pairs),
// 1 when the start is unreached, 2 when the walk stops at a cell above 0 that no neighbour continues (*out_n = 0 for both).
inline int path(const uint32_t *pot, const uint8_t *costmap, uint32_t width, uint32_t height, const uint8_t *weight, uint32_t x, uint32_t y, uint32_t *out_xy, size_t cap,
                size_t *out_n) {
    *out_n = 0;
    size_t cur = static_cast<size_t>(y) * width + x, n_cells = 0;
    if (pot[cur] == kNavUnreached || weight[costmap[cur]] == 0u) return 1;
    for (;;) {
        if (n_cells < cap) out_xy[2 * n_cells] = x, out_xy[2 * n_cells + 1] = y;
        ++n_cells;
        if (pot[cur] == 0u) break;
        uint32_t k = 0;
        for (; k < 8u; ++k) {
            const int64_t nx = static_cast<int64_t>(x) + nav_dx(k), ny = static_cast<int64_t>(y) + nav_dy(k);
            if (nx < 0 || ny < 0 || nx >= static_cast<int64_t>(width) || ny >= static_cast<int64_t>(height)) continue;
            const size_t n = static_cast<size_t>(ny) * width + static_cast<size_t>(nx);
            if (!nav_descends(pot[cur], weight[costmap[cur]], weight[costmap[n]], pot[n], k)) continue;
            x = static_cast<uint32_t>(nx), y = static_cast<uint32_t>(ny), cur = n;  // the potential falls by at least 2 a step: the walk ends
            break;
        }
        if (k == 8u) return 2;
    }
    *out_n = n_cells;
    return 0;
}
}  // namespace nav_host

}  // namespace kicp
