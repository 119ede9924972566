// kicp_search_host.hpp -- the host's side of the whole-map relocalisation (kicp_search_poses): the branch-and-bound traversal over the
// occupancy pyramid, templated on the scorer, so that the same code runs over the GPU's k_search_score (kicp_search.hip) and over a
// CPU scorer in a stand-alone program (tests/cpp/search_host_test.cpp).  Plain C++ without any device header.
//
// Nodes are (j, ix, iy) with index (j * ny + iy) * nx + ix.  score(level, nodes, hits) must write, for every node, a count that at
// level 0 is the node's own score and at level h > 0 is an upper bound of the level-0 score of every node (j, ix + a, iy + b),
// 0 <= a, b < 2^h (the sliding OR of the pyramid gives exactly that).  The traversal's RESULT does not depend on how tight the bounds
// are or on which blocks the dive meets: it is the first min(top_m, all) nodes by (score descending, index ascending).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kicp {

constexpr int kSearchOk = 0, kSearchCapacity = -3;  // (= KICP_OK, KICP_ERR_CAPACITY)
constexpr size_t kSearchDiveWidth = 64;             // blocks the greedy dive follows per level (at least top_m)

struct SearchCounts {
    unsigned long long nodes_scored = 0;  // nodes handed to the scorer, all levels, the dive included
    unsigned int launches = 0;            // calls of the scorer
};
struct SearchHit {
    unsigned long long node;
    unsigned int hits;
};
inline bool search_better(const SearchHit &a, const SearchHit &b) { return a.hits > b.hits || (a.hits == b.hits && a.node < b.node); }

// the four children (block size 2^(level - 1)) of every block of `parents` (block size 2^level) that lie inside the window, parent by parent
inline void search_children(const std::vector<SearchHit> &parents, int level, unsigned int nx, unsigned int ny, std::vector<unsigned long long> &out) {
    const unsigned long long s = 1ull << (level - 1);
    out.clear();
    out.reserve(parents.size() * 4);
    for (const SearchHit &p : parents) {
        const unsigned long long ix = p.node % nx, row = p.node / nx, iy = row % ny;
        for (int b = 0; b < 2; ++b)
            for (int a = 0; a < 2; ++a)
                if (ix + a * s < nx && iy + b * s < ny) out.push_back(p.node + b * s * nx + a * s);
    }
}

// Scorer: int(int level, const std::vector<unsigned long long> &nodes, std::vector<unsigned int> &hits) - resizes hits to
// nodes.size(); a non-zero return ends the search with that value.  `out`: the result, best first.  Returns kSearchOk,
// kSearchCapacity when more than max_nodes nodes would have to be scored (nothing is returned then), or the scorer's error.
template <class Scorer>
int search_top(unsigned int nx, unsigned int ny, unsigned int nyaw, int levels, size_t top_m, unsigned long long max_nodes, Scorer &&score,
               std::vector<SearchHit> &out, SearchCounts &counts) {
    out.clear();
    counts = SearchCounts{};
    const unsigned long long total = static_cast<unsigned long long>(nx) * ny * nyaw;
    const size_t m = static_cast<size_t>(std::min<unsigned long long>(top_m, total));
    if (m == 0) return kSearchOk;
    std::vector<unsigned long long> nodes;
    std::vector<unsigned int> hits;
    auto run = [&](int level, std::vector<SearchHit> &scored) -> int {
        if (counts.nodes_scored + nodes.size() > max_nodes) return kSearchCapacity;
        counts.nodes_scored += nodes.size(), ++counts.launches;
        if (int rc = score(level, nodes, hits)) return rc;
        scored.resize(nodes.size());
        for (size_t k = 0; k < nodes.size(); ++k) scored[k] = SearchHit{nodes[k], hits[k]};
        return kSearchOk;
    };
    // 1. the window tiled with blocks of 2^levels cells (a block that overhangs the window is still a valid bound)
    const unsigned long long block = 1ull << levels;
    for (unsigned int j = 0; j < nyaw; ++j)
        for (unsigned long long iy = 0; iy < ny; iy += block)
            for (unsigned long long ix = 0; ix < nx; ix += block) nodes.push_back((static_cast<unsigned long long>(j) * ny + iy) * nx + ix);
    std::vector<SearchHit> front;
    if (int rc = run(levels, front)) return rc;
    // 2. a greedy dive with the best blocks down to level 0: L = the m-th best leaf it meets (0 when it meets fewer: nothing is pruned)
    unsigned int limit = 0;
    if (levels > 0) {
        const size_t width = std::max(kSearchDiveWidth, m);
        std::vector<SearchHit> dive = front;
        for (int level = levels; level >= 1; --level) {
            if (dive.size() > width) {
                std::partial_sort(dive.begin(), dive.begin() + width, dive.end(), search_better);
                dive.resize(width);
            }
            search_children(dive, level, nx, ny, nodes);
            if (int rc = run(level - 1, dive)) return rc;
        }
        if (dive.size() >= m) {
            std::nth_element(dive.begin(), dive.begin() + (m - 1), dive.end(), search_better);
            limit = dive[m - 1].hits;
        }
    }
    // 3. level by level: the children of every block whose bound reaches L (>=: ties must survive, the index decides among them at the end)
    for (int level = levels; level >= 1; --level) {
        front.erase(std::remove_if(front.begin(), front.end(), [&](const SearchHit &h) { return h.hits < limit; }), front.end());
        search_children(front, level, nx, ny, nodes);
        if (int rc = run(level - 1, front)) return rc;
    }
    // 4. `front` holds every node whose score reaches L, at least m of them: the best m, ties to the lower index
    std::partial_sort(front.begin(), front.begin() + m, front.end(), search_better);
    front.resize(m);
    out.swap(front);
    return kSearchOk;
}

}  // namespace kicp
