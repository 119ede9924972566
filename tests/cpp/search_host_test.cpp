// The host traversal of kicp_search_poses (kicp_search_host.hpp) in a program of its own, over a CPU scorer that restates the
// pyramid in two dimensions: random bitsets, a handful of "points" with a random cell per yaw, level h = the sliding OR over
// 2^h x 2^h cells, cells beyond the grid empty.  Every result is compared with the exhaustive stable top-M.  Built with ASan + UBSan
// by tests/test_search_host.py; prints "ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <random>

#include "kicp_search_host.hpp"

using kicp::SearchCounts;
using kicp::SearchHit;

namespace {
struct Model {
    int gx = 0, gy = 0, levels = 0;
    unsigned int nx = 1, ny = 1, nyaw = 1;
    std::vector<std::vector<unsigned char>> occ;  // [level][y * gx + x]
    std::vector<int> cells;                        // [yaw][point][2]
    int points = 0;
    bool at(int level, long x, long y) const { return x >= 0 && y >= 0 && x < gx && y < gy && occ[level][static_cast<size_t>(y) * gx + x]; }
    void build_levels() {
        occ.resize(levels + 1);
        for (int h = 1; h <= levels; ++h) {
            const long s = 1l << (h - 1);
            occ[h].assign(occ[0].size(), 0);
            for (long y = 0; y < gy; ++y)
                for (long x = 0; x < gx; ++x)
                    occ[h][static_cast<size_t>(y) * gx + x] = at(h - 1, x, y) || at(h - 1, x + s, y) || at(h - 1, x, y + s) || at(h - 1, x + s, y + s);
        }
    }
    unsigned int score(int level, unsigned long long node) const {
        const long ix = static_cast<long>(node % nx), iy = static_cast<long>((node / nx) % ny);
        const size_t j = static_cast<size_t>(node / nx / ny);
        unsigned int c = 0;
        // (a block that starts less than its size below the grid still covers cells of it: it reads the first column / row, as the device does)
        const long lowest = -(1l << level);
        for (int p = 0; p < points; ++p) {
            long x = cells[(j * points + p) * 2] + ix, y = cells[(j * points + p) * 2 + 1] + iy;
            x = (x < 0 && x > lowest) ? 0 : x, y = (y < 0 && y > lowest) ? 0 : y;
            c += at(level, x, y);
        }
        return c;
    }
};

unsigned long long g_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

// fill: 0 empty, 1 full, 2 random with the given density
Model make(std::mt19937_64 &rng, unsigned int nx, unsigned int ny, unsigned int nyaw, int levels, int points, int fill, double density) {
    Model m;
    m.nx = nx, m.ny = ny, m.nyaw = nyaw, m.levels = levels, m.points = points;
    m.gx = static_cast<int>(nx) + 11, m.gy = static_cast<int>(ny) + 7;  // some cells of some nodes leave the grid on every side
    m.occ.resize(1);
    m.occ[0].resize(static_cast<size_t>(m.gx) * m.gy);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (auto &b : m.occ[0]) b = fill == 1 || (fill == 2 && u(rng) < density);
    m.build_levels();
    std::uniform_int_distribution<int> cx(-6, 12), cy(-5, 9);
    m.cells.resize(static_cast<size_t>(nyaw) * points * 2);
    for (size_t k = 0; k < m.cells.size(); k += 2) m.cells[k] = cx(rng), m.cells[k + 1] = cy(rng);
    return m;
}
std::vector<SearchHit> exhaustive(const Model &m, size_t top_m) {
    const unsigned long long total = static_cast<unsigned long long>(m.nx) * m.ny * m.nyaw;
    std::vector<SearchHit> all(total);
    for (unsigned long long k = 0; k < total; ++k) all[k] = SearchHit{k, m.score(0, k)};
    std::stable_sort(all.begin(), all.end(), [](const SearchHit &a, const SearchHit &b) { return a.hits > b.hits; });
    all.resize(std::min<unsigned long long>(top_m, total));
    return all;
}
int search(const Model &m, size_t top_m, unsigned long long max_nodes, std::vector<SearchHit> &out, SearchCounts &counts) {
    auto scorer = [&](int level, const std::vector<unsigned long long> &nodes, std::vector<unsigned int> &hits) {
        hits.resize(nodes.size());
        for (size_t k = 0; k < nodes.size(); ++k) {
            CHECK(nodes[k] < static_cast<unsigned long long>(m.nx) * m.ny * m.nyaw);
            CHECK(level >= 0 && level <= m.levels);
            const unsigned long long ix = nodes[k] % m.nx, iy = (nodes[k] / m.nx) % m.ny;
            CHECK(ix % (1ull << level) == 0 && iy % (1ull << level) == 0);  // blocks start on multiples of their size
            hits[k] = m.score(level, nodes[k]);
        }
        return 0;
    };
    return kicp::search_top(m.nx, m.ny, m.nyaw, m.levels, top_m, max_nodes, scorer, out, counts);
}
void compare(const Model &m, size_t top_m) {
    std::vector<SearchHit> got;
    SearchCounts counts;
    CHECK(search(m, top_m, ~0ull, got, counts) == kicp::kSearchOk);
    const std::vector<SearchHit> want = exhaustive(m, top_m);
    CHECK(got.size() == want.size());
    for (size_t k = 0; k < want.size(); ++k) CHECK(got[k].node == want[k].node && got[k].hits == want[k].hits);
    CHECK(counts.launches >= 1 && counts.nodes_scored >= 1);
}
}  // namespace

int main() {
    std::mt19937_64 rng(20240521);
    const size_t tops[] = {1, 8, 100, 100000};  // (the last one: above every node count here)
    // random grids: sizes that are and are not multiples of the block, several depths, sparse and dense, few points (many ties) and many
    const unsigned int shapes[][3] = {{37, 50, 3}, {1, 1, 1}, {64, 64, 2}, {5, 3, 4}, {33, 1, 2}, {1, 40, 1}, {16, 17, 5}};
    for (const auto &s : shapes)
        for (int levels : {0, 1, 3, 5})
            for (int points : {1, 2, 40})
                for (double density : {0.02, 0.3, 0.9}) {
                    const Model m = make(rng, s[0], s[1], s[2], levels, points, 2, density);
                    for (size_t top : tops) compare(m, top);
                }
    // an empty grid: every score is zero, the result is the first nodes by index
    {
        const Model m = make(rng, 37, 50, 3, 4, 10, 0, 0.0);
        compare(m, 8);
        std::vector<SearchHit> got;
        SearchCounts counts;
        CHECK(search(m, 8, ~0ull, got, counts) == kicp::kSearchOk);
        for (size_t k = 0; k < 8; ++k) CHECK(got[k].node == k && got[k].hits == 0);
    }
    // a full grid prunes nothing where the points' cells stay inside: all levels are visited, and a budget below that gives the
    // capacity error - never a result
    {
        Model m = make(rng, 32, 32, 2, 3, 6, 1, 1.0);
        for (auto &c : m.cells) c = 2;  // (every cell of every node inside the grid: all scores equal the number of points)
        compare(m, 8);
        std::vector<SearchHit> got;
        SearchCounts counts;
        CHECK(search(m, 8, ~0ull, got, counts) == kicp::kSearchOk);
        const unsigned long long total = 32ull * 32 * 2;
        CHECK(counts.nodes_scored >= total + total / 4 + total / 16 + total / 64);  // every block of every level (plus the dive)
        const unsigned long long needed = counts.nodes_scored;
        got.assign(3, SearchHit{7, 7});
        CHECK(search(m, 8, needed - 1, got, counts) == kicp::kSearchCapacity && got.empty());
        CHECK(search(m, 8, 10, got, counts) == kicp::kSearchCapacity && got.empty());
        CHECK(search(m, 8, needed, got, counts) == kicp::kSearchOk && got.size() == 8);
    }
    // a sparse grid is pruned: fewer nodes are scored than the window has
    {
        const Model m = make(rng, 64, 64, 4, 4, 60, 2, 0.003);
        std::vector<SearchHit> got;
        SearchCounts counts;
        CHECK(search(m, 8, ~0ull, got, counts) == kicp::kSearchOk);
        CHECK(counts.nodes_scored < 64ull * 64 * 4);
        compare(m, 8);
    }
    // a scorer's error ends the search with that value
    {
        const Model m = make(rng, 8, 8, 1, 2, 3, 2, 0.5);
        std::vector<SearchHit> got;
        SearchCounts counts;
        int calls = 0;
        auto failing = [&](int, const std::vector<unsigned long long> &nodes, std::vector<unsigned int> &hits) {
            hits.assign(nodes.size(), 1u);
            return ++calls == 2 ? -1 : 0;
        };
        CHECK(kicp::search_top(m.nx, m.ny, m.nyaw, m.levels, 4, ~0ull, failing, got, counts) == -1 && got.empty());
    }
    std::printf("ok %llu\n", g_checks);
    return 0;
}
