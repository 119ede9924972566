// kicp_front_host.hpp -- the arithmetic of the grid's exploration frontiers (kicp_grid_frontiers, kicp_frontiers_from_occupancy;
// include/kicp.h states the semantics): the frontier-cell predicate from five classes, the update of one frontier's row by one of its
// cells, the order and the filter of the output, and the host entry's labelling.  ONE text for the kernels (kicp_front.hpp), for the
// entries (kicp_grid_explore.hip) and for the stand-alone program that runs front_host:: under sanitizers (tests/cpp/front_host_test.cpp).
// The class of a readout is kicp_clear_host.hpp's clear_class: the classes are the clearance's.  Everything is integer.
//
// A ROW while it is being summed has nine live words: 0 the label, 1 the size, 2 and 3 the sums of x and y, 4 .. 7 the box (min x,
// max x, min y, max y) and in word 8 the least 64-bit key pot(c) * 2^32 + c of its cells; front_emit splits the key into words 8 and 9.
// Every update commutes - adds, mins, maxes - so the order in which cells arrive does not matter.
#pragma once
#include <algorithm>
#include <vector>

#include "kicp_clear_host.hpp"

namespace kicp {

constexpr uint32_t kFrontWords = 10;          // KICP_FRONTIER_WORDS
constexpr uint32_t kFrontNone = 0xFFFFFFFFu;  // the label plane outside the frontier cells; pot(c) without a plan
constexpr uint32_t kFrontOutside = 3u;        // the "class" of a neighbour outside the grid: nothing, in particular not unknown

struct FrontParams {
    uint32_t min_observations;
    int32_t source_min;  // clear_source_min(occupied_thresh)
};

// own and the four edge neighbours' classes (kClear*, kFrontOutside)
KICP_HD bool front_is_frontier(uint32_t own, uint32_t west, uint32_t east, uint32_t south, uint32_t north) {
    return own == kClearClear && (west == kClearUnknown || east == kClearUnknown || south == kClearUnknown || north == kClearUnknown);
}
KICP_HD unsigned long long front_key(uint32_t pot, uint32_t cell) { return (static_cast<unsigned long long>(pot) << 32) | cell; }
// the row of a frontier no cell has been added to yet
KICP_HD void front_row_init(unsigned long long *row, uint32_t label) {
    row[0] = label, row[1] = row[2] = row[3] = 0ull;
    row[4] = row[6] = ~0ull, row[5] = row[7] = 0ull;
    row[8] = ~0ull, row[9] = 0ull;
}
// one cell more (host; the kernel does the same with one atomic per word)
inline void front_row_add(unsigned long long *row, uint32_t x, uint32_t y, unsigned long long key) {
    row[1] += 1ull, row[2] += x, row[3] += y;
    row[4] = std::min<unsigned long long>(row[4], x), row[5] = std::max<unsigned long long>(row[5], x);
    row[6] = std::min<unsigned long long>(row[6], y), row[7] = std::max<unsigned long long>(row[7], y);
    row[8] = std::min(row[8], key);
}
// Which of n summed rows (in any order) are output and in which order: those of at least min_size cells (word 1), by ascending label
// (word 0).  The transients' rows keep the same two words there (kicp_transient_host.hpp).
inline std::vector<size_t> front_order(const unsigned long long *rows, size_t n, uint32_t min_size) {
    std::vector<size_t> order;
    order.reserve(n);
    for (size_t i = 0; i < n; ++i)
        if (rows[i * kFrontWords + 1] >= min_size) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return rows[a * kFrontWords] < rows[b * kFrontWords]; });
    return order;
}
// The output of n summed rows: those front_order keeps, the key split into best_potential and best_cell; the first `cap` of them are
// stored.  Returns the number that passed the filter.
inline size_t front_emit(const unsigned long long *rows, size_t n, uint32_t min_size, unsigned long long *out, size_t cap) {
    const std::vector<size_t> order = front_order(rows, n, min_size);
    for (size_t k = 0; k < order.size() && k < cap; ++k) {
        const unsigned long long *row = rows + order[k] * kFrontWords;
        unsigned long long *o = out + k * kFrontWords;
        for (uint32_t w = 0; w < 8u; ++w) o[w] = row[w];
        o[8] = row[8] >> 32, o[9] = row[8] & 0xFFFFFFFFull;
    }
    return order.size();
}

namespace front_host {
inline uint32_t class_at(const int8_t *occupancy, uint32_t width, uint32_t height, int64_t x, int64_t y, int32_t source_min) {
    if (x < 0 || y < 0 || x >= static_cast<int64_t>(width) || y >= static_cast<int64_t>(height)) return kFrontOutside;
    return clear_class(occupancy[static_cast<size_t>(y) * width + static_cast<size_t>(x)], source_min);
}
// flags: a byte per cell, 1 on a frontier cell
inline void mark(const int8_t *occupancy, uint32_t width, uint32_t height, int32_t source_min, std::vector<uint8_t> &flags) {
    flags.assign(static_cast<size_t>(width) * height, 0u);
    for (int64_t y = 0; y < static_cast<int64_t>(height); ++y)
        for (int64_t x = 0; x < static_cast<int64_t>(width); ++x)
            flags[static_cast<size_t>(y) * width + static_cast<size_t>(x)] =
                front_is_frontier(class_at(occupancy, width, height, x, y, source_min), class_at(occupancy, width, height, x - 1, y, source_min),
                                  class_at(occupancy, width, height, x + 1, y, source_min), class_at(occupancy, width, height, x, y - 1, source_min),
                                  class_at(occupancy, width, height, x, y + 1, source_min))
                    ? 1u
                    : 0u;
}
inline uint32_t find(const std::vector<uint32_t> &parent, uint32_t a) {
    while (parent[a] != a) a = parent[a];
    return a;
}
// Labels by a sequential union-find: the cells in index order, each joined to its frontier neighbours W, NW, N and NE (every
// undirected pair once), the larger root under the smaller - so parent[c] <= c always and a root is its component's least index.
// A second pass in index order replaces every parent by its root: parent[c] <= c has been labelled before c.
inline void label(const std::vector<uint8_t> &flags, uint32_t width, uint32_t height, std::vector<uint32_t> &labels) {
    labels.assign(flags.size(), kFrontNone);
    static const int32_t dx[4] = {-1, -1, 0, 1}, dy[4] = {0, -1, -1, -1};
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const uint32_t c = y * width + x;
            if (!flags[c]) continue;
            labels[c] = c;
            for (int k = 0; k < 4; ++k) {
                const int64_t nx = static_cast<int64_t>(x) + dx[k], ny = static_cast<int64_t>(y) + dy[k];
                if (nx < 0 || ny < 0 || nx >= static_cast<int64_t>(width)) continue;
                const uint32_t n = static_cast<uint32_t>(ny) * width + static_cast<uint32_t>(nx);
                if (!flags[n]) continue;
                const uint32_t a = find(labels, c), b = find(labels, n);
                if (a != b) labels[std::max(a, b)] = std::min(a, b);
            }
        }
    for (size_t c = 0; c < labels.size(); ++c)
        if (flags[c]) labels[c] = labels[labels[c]];
}
// The summed rows of every frontier, in ascending label order: a root is met before the other cells of its component.
// potential: nullable (pot = 0xFFFFFFFF everywhere).  row_of is scratch of one word per cell.
inline void rows(const std::vector<uint8_t> &flags, const std::vector<uint32_t> &labels, uint32_t width, const uint32_t *potential,
                 std::vector<uint32_t> &row_of, std::vector<unsigned long long> &out) {
    out.clear();
    row_of.assign(flags.size(), 0u);
    for (size_t c = 0; c < flags.size(); ++c) {
        if (!flags[c]) continue;
        const uint32_t cell = static_cast<uint32_t>(c);
        if (labels[c] == cell) {
            row_of[c] = static_cast<uint32_t>(out.size() / kFrontWords);
            out.resize(out.size() + kFrontWords);
            front_row_init(out.data() + out.size() - kFrontWords, cell);
        }
        front_row_add(out.data() + static_cast<size_t>(row_of[labels[c]]) * kFrontWords, cell % width, cell / width, front_key(potential ? potential[c] : kFrontNone, cell));
    }
}
// the whole host entry; out_labels nullable.  Returns the number of frontiers that passed the filter.
inline size_t frontiers(const int8_t *occupancy, uint32_t width, uint32_t height, int32_t source_min, uint32_t min_size, const uint32_t *potential,
                        unsigned long long *out_rows, size_t cap_rows, uint32_t *out_labels) {
    std::vector<uint8_t> flags;
    std::vector<uint32_t> labels, row_of;
    std::vector<unsigned long long> summed;
    mark(occupancy, width, height, source_min, flags);
    label(flags, width, height, labels);
    rows(flags, labels, width, potential, row_of, summed);
    if (out_labels) std::copy(labels.begin(), labels.end(), out_labels);
    return front_emit(summed.data(), summed.size() / kFrontWords, min_size, out_rows, cap_rows);
}
}  // namespace front_host

}  // namespace kicp
