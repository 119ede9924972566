// arc_tree_host_test.cpp -- arc_tree_host::nodes, score and best (kicp_arc_tree_host.hpp), the host side of scoring a tree of arc
// segments and the very arithmetic the kernel calls, in a program of its own: tests/test_arc_tree_host.py builds it plainly and under
// ASan + UBSan and compares what it writes with the restatement (tests/arc_tree_ref.py).
// Input (argv[1]): 11 doubles - width, height, cell, origin_x, origin_y, depth, n_samples, then w_potential, w_cost, w_blocked,
// min_free_steps - then branch and steps (depth doubles each), start[4], the primitives (sum of branch x 4), the footprint
// (n_samples x 2), all doubles, then q (width * height bytes) and the potential (width * height x uint32).
// Output (argv[2]): n_nodes, n_leaves, total_steps and the levels' offsets (3 + depth x uint64), the results (n_nodes x 4 x uint32) -
// the buffer holds exactly those, and the records' exactly two levels above the leaves - then arc_tree_host::best's leaf (uint64) and
// its path (depth x uint32, 0xFFFFFFFF where none was found).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_arc_tree_host.hpp"

template <class T>
static std::vector<T> read_values(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}
template <class T>
static void write_values(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "cannot write\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!f || !out) return 1;
    const auto h = read_values<double>(f, 11);
    const uint32_t width = static_cast<uint32_t>(h[0]), height = static_cast<uint32_t>(h[1]), depth = static_cast<uint32_t>(h[5]), n_samples = static_cast<uint32_t>(h[6]);
    if (width < 1u || height < 1u || !(h[2] > 0.0) || depth < 1u || depth > kicp::kArcTreeMaxDepth || n_samples < 1u || n_samples > kicp::kArcsMaxP) return 1;
    std::vector<unsigned int> branch, steps;
    for (double v : read_values<double>(f, depth)) branch.push_back(static_cast<unsigned int>(v));
    for (double v : read_values<double>(f, depth)) steps.push_back(static_cast<unsigned int>(v));
    kicp::ArcTreeShape shape;
    if (kicp::arc_tree_host::nodes(depth, branch.data(), steps.data(), shape) != kicp::arc_tree_host::kShapeOk) return 1;
    const auto start = read_values<double>(f, 4), primitives = read_values<double>(f, 4 * shape.n_primitives), footprint = read_values<double>(f, 2 * static_cast<size_t>(n_samples));
    const auto q = read_values<uint8_t>(f, static_cast<size_t>(width) * height);
    const auto potential = read_values<uint32_t>(f, static_cast<size_t>(width) * height);

    std::vector<unsigned long long> counts{shape.n_nodes, shape.n_leaves, shape.total_steps};
    for (uint32_t e = 0; e < depth; ++e) counts.push_back(shape.offset[e]);
    write_values(out, counts);
    const size_t half = depth > 1u ? shape.count[depth - 2u] : 0u;
    std::vector<kicp::ArcTreeNode> above(half), below(half);  // two allocations: a record written past either is seen
    std::vector<uint32_t> results(4 * shape.n_nodes);
    kicp::arc_tree_host::score(kicp::ArcGeom{h[2], h[3], h[4], width, height}, q.data(), potential.data(), start.data(), shape, branch.data(), steps.data(), primitives.data(),
                               footprint.data(), n_samples, above.data(), below.data(), results.data());
    write_values(out, results);
    std::vector<unsigned int> path(depth, 0xFFFFFFFFu);
    const size_t leaf = kicp::arc_tree_host::best(results.data(), shape, branch.data(), static_cast<uint32_t>(h[7]), static_cast<uint32_t>(h[8]), static_cast<uint32_t>(h[9]),
                                                  static_cast<uint32_t>(h[10]), path.data());
    write_values(out, std::vector<unsigned long long>{leaf});
    write_values(out, path);
    fclose(f);
    return fclose(out) == 0 ? 0 : 1;
}
