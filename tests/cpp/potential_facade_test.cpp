// potential_facade_test.cpp -- the cost-to-go field and its path through the drop-in C++ headers: KinematicICP::GridPotential,
// GridPotentialOfCostmap and PotentialPath after a short drive with a grid enabled, the way a node re-plans: the goal is a cell, the
// start is the cell the robot stands in after the last frame.
// Input: the drive file tests/test_potential_facade.py writes (the format of tests/test_grid_facade.py's), a file with the eight doubles
// of the grid's configuration followed by radius_cells, inscribed_radius, cost_scaling_factor, max_potential, the number of goals and
// the goals as x, y pairs, and a prefix for what it writes:
//   <prefix>_pose.bin        the pose after the drive (7 doubles)
//   <prefix>_counts.bin      the counters after the drive
//   <prefix>_costmap.bin     the full grid's GridCostmap (uint8)
//   <prefix>_potential.bin   GridPotential of the same arguments (uint32), <prefix>_of_costmap.bin GridPotentialOfCostmap over those bytes
//   <prefix>_clamped.bin     GridPotential with max_potential
//   <prefix>_stats.bin       the three calls' statistics (3 x 4 x uint64)
//   <prefix>_path.bin        PotentialPath from the robot's cell (uint32 pairs)
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
template <class F>
static bool refused(F &&call) {
    try {
        call();
    } catch (const std::runtime_error &) {
        return true;
    }
    return false;
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
        const auto gc = read_doubles(g, 13);
        const kicp_bridge::GridConfig grid_config{gc[0], gc[1], gc[2], static_cast<unsigned int>(gc[3]), static_cast<unsigned int>(gc[4]), gc[5], gc[6], gc[7]};
        const int radius = static_cast<int>(gc[8]);
        const kicp_bridge::GridClearanceConfig clearance_config{1u, 0.65, 0, radius};
        std::vector<uint8_t> table(static_cast<size_t>(radius) * radius + 2);
        kicp_bridge::check(kicp_grid_cost_table_nav2(grid_config.cell, radius, gc[9], gc[10], table.data(), table.size()), "kicp_grid_cost_table_nav2");
        const kicp_bridge::PlanConfig clamp{static_cast<unsigned int>(gc[11])};
        std::vector<KinematicICP::GridCell> goals;
        for (const auto &xy = read_doubles(g, 2 * static_cast<size_t>(gc[12])); goals.size() < xy.size() / 2;)
            goals.push_back({static_cast<unsigned int>(xy[2 * goals.size()]), static_cast<unsigned int>(xy[2 * goals.size() + 1])});
        const std::array<uint8_t, 256> weight = kicp_bridge::plan_weights(50, 4, 5, 253, 120);  // NavFn's, and unknown space passable at a price

        KinematicICP icp(cfg);
        std::vector<uint32_t> potential, of_costmap, clamped;
        std::vector<uint8_t> costmap;
        const bool r1 = refused([&] { icp.GridPotential(potential, clearance_config, table, true, weight, goals); });
        const bool r2 = refused([&] { icp.GridPotentialOfCostmap(potential, costmap, weight, goals); });
        const bool r3 = refused([&] { icp.PotentialPath(potential, costmap, weight, {0u, 0u}); });
        printf("refused_without_grid %d %d %d\n", r1 ? 1 : 0, r2 ? 1 : 0, r3 ? 1 : 0);
        icp.EnableGrid(grid_config);
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
        const unsigned int W = grid_config.width, H = grid_config.height;
        std::vector<unsigned long long> stats;
        icp.GridCostmap(costmap, clearance_config, table, true);
        for (unsigned long long v : icp.GridPotential(potential, clearance_config, table, true, weight, goals)) stats.push_back(v);
        for (unsigned long long v : icp.GridPotentialOfCostmap(of_costmap, costmap, weight, goals)) stats.push_back(v);
        for (unsigned long long v : icp.GridPotential(clamped, clearance_config, table, true, weight, goals, clamp)) stats.push_back(v);
        write_file(prefix + "_costmap.bin", costmap), write_file(prefix + "_potential.bin", potential), write_file(prefix + "_of_costmap.bin", of_costmap);
        write_file(prefix + "_clamped.bin", clamped), write_file(prefix + "_stats.bin", stats);
        const KinematicICP::GridCell start{static_cast<unsigned int>(std::floor((pose[4] - grid_config.origin_x) / grid_config.cell)),
                                           static_cast<unsigned int>(std::floor((pose[5] - grid_config.origin_y) / grid_config.cell))};
        const auto path = icp.PotentialPath(potential, costmap, weight, start);
        std::vector<unsigned int> flat;
        for (const auto &c : path) flat.push_back(c[0]), flat.push_back(c[1]);
        write_file(prefix + "_path.bin", flat);
        std::vector<unsigned short> counts(2 * static_cast<size_t>(W) * H);
        kicp_bridge::check(kicp_grid_counts(icp.Grid().get(), counts.data(), counts.size() / 2), "kicp_grid_counts");
        write_file(prefix + "_counts.bin", counts);
        const std::vector<KinematicICP::GridCell> outside{{W, 0u}};
        printf("refused_goal_outside_the_grid %d\n", refused([&] { icp.GridPotential(potential, clearance_config, table, true, weight, outside); }) ? 1 : 0);
        size_t lethal = 0;  // a cell the field does not enter: lethal or inscribed
        while (lethal < potential.size() && potential[lethal] != 0xFFFFFFFFu) ++lethal;
        const KinematicICP::GridCell unreachable{static_cast<unsigned int>(lethal % W), static_cast<unsigned int>(lethal / W)};
        printf("refused_unreachable_start %d\n", lethal < potential.size() && refused([&] { icp.PotentialPath(potential, costmap, weight, unreachable); }) ? 1 : 0);
        printf("refused_costmap_of_another_size %d\n", refused([&] { icp.GridPotentialOfCostmap(of_costmap, table, weight, goals); }) ? 1 : 0);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
