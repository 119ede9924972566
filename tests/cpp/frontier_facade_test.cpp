// frontier_facade_test.cpp -- the exploration frontiers through the drop-in C++ headers: KinematicICP::GridFrontiers on a grid whose
// counters the test sets, against the C entry it wraps, and the exceptions without a grid and without a plan.
// Input: a file with the grid's width and height (2 x uint32) and its counters (width * height x 2 x uint16), and a prefix for what
// it writes:
//   <prefix>_rows.bin     GridFrontiers with min_size 2 and the plan of a potential from the grid's middle cell: per frontier the ten
//                         words of kicp_grid_frontiers, taken back out of the named fields (uint64)
//   <prefix>_labels.bin   its label plane (uint32)
//   <prefix>_potential.bin the potential of that plan (uint32)
// It prints same_as_the_c_entry 1 when the rows and the labels equal what kicp_grid_frontiers itself returns for the same arguments.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "kinematic_icp/pipeline/KinematicICP.hpp"

using kinematic_icp::pipeline::KinematicICP;

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
static void write_file(const std::string &path, const std::vector<T> &v) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
}
template <class F>
static bool refused(F &&call, const char *needle) {
    try {
        call();
    } catch (const std::runtime_error &e) {
        return std::string(e.what()).find(needle) != std::string::npos;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    const std::string prefix = argv[2];
    try {
        const auto wh = read_values<uint32_t>(f, 2);
        const unsigned int W = wh[0], H = wh[1];
        const auto counts = read_values<unsigned short>(f, 2 * static_cast<size_t>(W) * H);
        const kicp_bridge::FrontierConfig config{1u, 0.65, 2u};
        KinematicICP icp{kinematic_icp::pipeline::Config{}};
        std::vector<kicp_bridge::Frontier> frontiers;
        std::vector<uint32_t> labels;
        printf("refused_without_grid %d\n", refused([&] { icp.GridFrontiers(frontiers, config); }, "EnableGrid") ? 1 : 0);
        icp.EnableGrid(kicp_bridge::GridConfig{0.05, 0.0, 0.0, W, H, 0.0, 1.0, 1.0});
        kicp_bridge::check(kicp_grid_set_counts(icp.Grid().get(), counts.data(), counts.size() / 2), "kicp_grid_set_counts");
        printf("refused_without_plan %d\n", refused([&] { icp.GridFrontiers(frontiers, config, true); }, "call GridPotential first") ? 1 : 0);
        icp.GridFrontiers(frontiers, config);  // without a plan it needs none
        printf("without_plan %zu %d\n", frontiers.size(), !frontiers.empty() && frontiers.front().best_potential == 0xFFFFFFFFu && frontiers.front().best_cell == frontiers.front().label ? 1 : 0);

        std::vector<uint8_t> table(2 * 2 + 2);
        kicp_bridge::check(kicp_grid_cost_table_nav2(0.05, 2, 0.0, 3.0, table.data(), table.size()), "kicp_grid_cost_table_nav2");
        std::vector<uint32_t> potential;
        icp.GridPotential(potential, kicp_bridge::GridClearanceConfig{1u, 0.65, 0, 2}, table, false, kicp_bridge::plan_weights(), {{W / 2u, H / 2u}});
        icp.GridFrontiers(frontiers, config, true, &labels);
        std::vector<unsigned long long> rows;
        double cx = 0.0, cy = 0.0;
        for (const auto &fr : frontiers) {
            for (unsigned long long v : {static_cast<unsigned long long>(fr.label), static_cast<unsigned long long>(fr.size), static_cast<unsigned long long>(fr.sum_x),
                                         static_cast<unsigned long long>(fr.sum_y), static_cast<unsigned long long>(fr.min_x), static_cast<unsigned long long>(fr.max_x),
                                         static_cast<unsigned long long>(fr.min_y), static_cast<unsigned long long>(fr.max_y), static_cast<unsigned long long>(fr.best_potential),
                                         static_cast<unsigned long long>(fr.best_cell)})
                rows.push_back(v);
            cx = fr.centroid_x(), cy = fr.centroid_y();
            if (!(cx >= fr.min_x && cx <= fr.max_x && cy >= fr.min_y && cy <= fr.max_y)) return 4;
        }
        std::vector<unsigned long long> c_rows(rows.size() + KICP_FRONTIER_WORDS);
        std::vector<unsigned int> c_labels(labels.size());
        size_t n = 0;
        kicp_bridge::check(kicp_grid_frontiers(icp.Grid().get(), &config, 1, c_rows.data(), c_rows.size() / KICP_FRONTIER_WORDS, &n, c_labels.data(), c_labels.size()),
                           "kicp_grid_frontiers");
        c_rows.resize(n * KICP_FRONTIER_WORDS);
        printf("same_as_the_c_entry %d\n", c_rows == rows && std::vector<uint32_t>(c_labels.begin(), c_labels.end()) == labels ? 1 : 0);
        write_file(prefix + "_rows.bin", rows), write_file(prefix + "_labels.bin", labels), write_file(prefix + "_potential.bin", potential);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f);
    return 0;
}
