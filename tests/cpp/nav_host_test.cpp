// nav_host_test.cpp -- nav_host::weights, nav_host::potential and nav_host::path (kicp_nav_host.hpp), the host side of the cost-to-go
// field and the very arithmetic the kernels call, in a program of its own: tests/test_potential_host.py builds it plainly and under
// ASan + UBSan and compares what it writes with the restatement (tests/potential_ref.py).
// Input (argv[1]): 11 x uint32 - width, height, max_potential, n_goals, start_x, start_y, then kicp_plan_weights' neutral, factor_num,
// factor_den, lethal_from, unknown_weight - then weight[256], width * height bytes of costmap and n_goals (x, y) pairs of uint32.
// Output (argv[2]): the potential (width * height x uint32), the four statistics (uint64), the path's return value and length (uint32
// each; the buffer holds exactly the cells the restatement's path has, so nothing may be written past it) and its cells, then the
// weights table (256 bytes).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_nav_host.hpp"

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
    if (argc < 4) return 1;
    FILE *f = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!f || !out) return 1;
    const size_t path_cap = static_cast<size_t>(atol(argv[3]));
    const auto h = read_values<uint32_t>(f, 11);
    const uint32_t width = h[0], height = h[1];
    if (width < 1u || height < 1u || h[2] < 1u || h[2] > kicp::kNavMaxPotential || h[4] >= width || h[5] >= height) return 1;
    const auto weight = read_values<uint8_t>(f, 256);
    const auto costmap = read_values<uint8_t>(f, static_cast<size_t>(width) * height);
    const auto goals = read_values<uint32_t>(f, 2 * static_cast<size_t>(h[3]));
    for (size_t g = 0; g < h[3]; ++g)
        if (goals[2 * g] >= width || goals[2 * g + 1] >= height) return 1;
    std::vector<uint32_t> potential(costmap.size());
    std::vector<unsigned long long> stats(4);
    kicp::nav_host::potential(costmap.data(), width, height, weight.data(), h[2], goals.data(), h[3], potential.data(), stats.data());
    write_values(out, potential), write_values(out, stats);
    std::vector<uint32_t> cells(2 * path_cap);
    size_t n = 0;
    const int rc = kicp::nav_host::path(potential.data(), costmap.data(), width, height, weight.data(), h[4], h[5], cells.data(), path_cap, &n);
    write_values(out, std::vector<uint32_t>{static_cast<uint32_t>(rc), static_cast<uint32_t>(n)});
    cells.resize(2 * (n < path_cap ? n : path_cap));
    write_values(out, cells);
    if (h[6] < 1u || h[6] > 255u || h[8] < 1u || h[9] > 255u || h[10] > 255u) return 1;
    std::vector<uint8_t> table(256);
    kicp::nav_host::weights(h[6], h[7], h[8], h[9], h[10], table.data());
    write_values(out, table);
    fclose(f);
    return fclose(out) == 0 ? 0 : 1;
}
