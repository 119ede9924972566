// arc_tree_facade_test.cpp -- a tree of arc segments scored through the drop-in C++ headers: KinematicICP::ScoreArcTree and
// BestArcTreeLeaf after a short drive with a grid enabled, the way a node picks its next command: GridPotential towards a goal cell,
// then the tree from the pose the robot stands at.
// Input: the drive file tests/test_arc_tree_facade.py writes (the format of tests/test_grid_facade.py's), a file with the eight doubles
// of the grid's configuration followed by radius_cells, inscribed_radius, cost_scaling_factor, the goal's x and y, dt, the footprint's
// box x_min, x_max, y_min, y_max, spacing, the depth, branch and steps (depth doubles each) and the commands of the primitives as
// v, omega pairs (sum of branch of them), and a prefix for what it writes:
//   <prefix>_pose.bin        the pose after the drive (7 doubles)
//   <prefix>_costmap.bin     the full grid's GridCostmap (uint8), <prefix>_potential.bin GridPotential of the same arguments (uint32)
//   <prefix>_start.bin       the start ScoreArcTree made of the pose (4 doubles)
//   <prefix>_primitives.bin  ArcSteps of the commands, <prefix>_footprint.bin FootprintBox of the box (doubles)
//   <prefix>_results.bin     ScoreArcTree from the pose (uint32 x 4 per node), <prefix>_results_start.bin the same from the start,
//   <prefix>_results_c.bin   kicp_grid_score_arc_tree itself on Grid()
//   <prefix>_best.bin        BestArcTreeLeaf with (1, 0, 0, 1), (1, 2, 300, 0) and (0, 1, 0, T + 1): per ranking found, leaf and the
//                            path's depth entries (0xFFFFFFFF each when no leaf was found), all uint64
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kinematic_icp/pipeline/KinematicICP.hpp"

using kinematic_icp::pipeline::KinematicICP;

static std::vector<double> read_doubles(FILE *f, size_t n) {
    std::vector<double> v(n);
    if (n && fread(v.data(), sizeof(double), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}
static std::vector<Eigen::Vector3d> to_points(const std::vector<double> &v) {
    std::vector<Eigen::Vector3d> p(v.size() / 3);
    if (!p.empty()) std::memcpy(p.front().data(), v.data(), v.size() * sizeof(double));
    return p;
}
template <class T>
static void write_file(const std::string &path, const std::vector<T> &v) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
}
// "" when the call went through, else what it threw
template <class F>
static std::string refusal(F &&call) {
    try {
        call();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return "";
}

int main(int argc, char **argv) {
    if (argc < 4) return 1;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "rb");
    if (!f || !g) return 1;
    const std::string prefix = argv[3];
    try {
        const auto h = read_doubles(f, 4);  // n_frames, voxel, max_range, deskew
        kinematic_icp::pipeline::Config cfg;
        cfg.voxel_size = h[1], cfg.max_range = h[2], cfg.deskew = h[3] != 0.0;
        const Sophus::SE3d ext = kicp_bridge::from_params(read_doubles(f, 7).data());
        const auto gc = read_doubles(g, 20);
        const kicp_bridge::GridConfig grid_config{gc[0], gc[1], gc[2], static_cast<unsigned int>(gc[3]), static_cast<unsigned int>(gc[4]), gc[5], gc[6], gc[7]};
        const int radius = static_cast<int>(gc[8]);
        const kicp_bridge::GridClearanceConfig clearance_config{1u, 0.65, 0, radius};
        std::vector<uint8_t> table(static_cast<size_t>(radius) * radius + 2);
        kicp_bridge::check(kicp_grid_cost_table_nav2(grid_config.cell, radius, gc[9], gc[10], table.data(), table.size()), "kicp_grid_cost_table_nav2");
        const std::vector<KinematicICP::GridCell> goals{{static_cast<unsigned int>(gc[11]), static_cast<unsigned int>(gc[12])}};
        const size_t depth = static_cast<size_t>(gc[19]);
        kicp_bridge::ArcTree tree;
        size_t rows = 0;
        for (double b : read_doubles(g, depth)) tree.branch.push_back(static_cast<unsigned int>(b)), rows += static_cast<size_t>(b);
        for (double s : read_doubles(g, depth)) tree.steps.push_back(static_cast<unsigned int>(s));
        std::vector<double> v, omega;
        const auto commands = read_doubles(g, 2 * rows);
        for (size_t k = 0; k < rows; ++k) v.push_back(commands[2 * k]), omega.push_back(commands[2 * k + 1]);
        const std::array<uint8_t, 256> weight = kicp_bridge::plan_weights(50, 4, 5, 253, 120);  // NavFn's, and unknown space passable at a price

        KinematicICP icp(cfg);
        tree.primitives = icp.ArcSteps(v, omega, gc[13]);
        const auto footprint = icp.FootprintBox(gc[14], gc[15], gc[16], gc[17], gc[18]);
        const kicp_bridge::ArcTreeCounts counts = kicp_bridge::arc_tree_nodes(tree);
        std::vector<kicp_bridge::ArcResult> results, from_start, by_c(counts.n_nodes);
        printf("refused_without_grid %d\n", refusal([&] { icp.ScoreArcTree(results, icp.pose(), tree, footprint); }).find("EnableGrid") != std::string::npos ? 1 : 0);
        icp.EnableGrid(grid_config);
        printf("refused_without_plan %d\n",
               refusal([&] { icp.ScoreArcTree(results, icp.pose(), tree, footprint); }).find("ScoreArcTree: call GridPotential first") != std::string::npos ? 1 : 0);
        for (size_t k = 0; k < static_cast<size_t>(h[0]); ++k) {
            const auto n = read_doubles(f, 1);
            const auto points = to_points(read_doubles(f, static_cast<size_t>(n[0]) * 3));
            const auto stamps = read_doubles(f, static_cast<size_t>(n[0]));
            const Sophus::SE3d delta = kicp_bridge::from_params(read_doubles(f, 7).data());
            icp.RegisterFrame(points, stamps, ext, delta);
        }
        std::vector<double> pose(7);
        kicp_bridge::to_params(icp.pose(), pose.data());
        write_file(prefix + "_pose.bin", pose);
        std::vector<uint32_t> potential;
        std::vector<uint8_t> costmap;
        icp.GridPotential(potential, clearance_config, table, true, weight, goals);
        icp.ScoreArcTree(results, icp.pose(), tree, footprint);
        const kicp_bridge::ArcStart start = kicp_bridge::arc_start(icp.pose());
        icp.ScoreArcTree(from_start, start, tree, footprint);
        icp.GridCostmap(costmap, clearance_config, table, true);  // writes no buffer of the plan
        kicp_bridge::check(kicp_grid_score_arc_tree(icp.Grid().get(), start.data(), static_cast<unsigned int>(depth), tree.branch.data(), tree.steps.data(),
                                                    tree.primitives.front().data(), footprint.front().data(), footprint.size(), by_c.front().data(), 4 * by_c.size()),
                           "kicp_grid_score_arc_tree");
        write_file(prefix + "_costmap.bin", costmap), write_file(prefix + "_potential.bin", potential);
        write_file(prefix + "_start.bin", std::vector<double>(start.begin(), start.end()));
        write_file(prefix + "_primitives.bin", tree.primitives), write_file(prefix + "_footprint.bin", footprint);
        write_file(prefix + "_results.bin", results), write_file(prefix + "_results_start.bin", from_start), write_file(prefix + "_results_c.bin", by_c);
        printf("counts %zu %zu %u\n", counts.n_nodes, counts.n_leaves, counts.total_steps);
        std::vector<unsigned long long> best;
        for (const auto &leaf : {icp.BestArcTreeLeaf(results, tree), icp.BestArcTreeLeaf(results, tree, 1, 2, 300, 0), icp.BestArcTreeLeaf(results, tree, 0, 1, 0, counts.total_steps + 1)}) {
            best.push_back(leaf.found ? 1u : 0u), best.push_back(leaf.leaf);
            for (size_t e = 0; e < depth; ++e) best.push_back(leaf.found ? leaf.path[e] : 0xFFFFFFFFu);
        }
        write_file(prefix + "_best.bin", best);
        // a potential call that fails leaves no plan
        const std::vector<KinematicICP::GridCell> outside{{grid_config.width, 0u}};
        const bool failed = !refusal([&] { icp.GridPotential(potential, clearance_config, table, true, weight, outside); }).empty();
        printf("refused_after_a_failed_potential %d\n",
               failed && refusal([&] { icp.ScoreArcTree(from_start, start, tree, footprint); }).find("call GridPotential first") != std::string::npos ? 1 : 0);
        kicp_bridge::ArcTree short_of_a_row = tree;
        short_of_a_row.primitives.pop_back();
        printf("refused_a_tree_short_of_a_row %d\n", refusal([&] { kicp_bridge::arc_tree_nodes(short_of_a_row); }).empty() ? 0 : 1);
        kicp_bridge::ArcTree too_deep;
        too_deep.branch.assign(9, 1u), too_deep.steps.assign(9, 1u), too_deep.primitives.assign(9, kicp_bridge::ArcStep{0.1, 0.0, 1.0, 0.0});
        printf("refused_depth_9 %d\n", refusal([&] { kicp_bridge::arc_tree_nodes(too_deep); }).find("limit 8") != std::string::npos ? 1 : 0);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
