// clearance_facade_test.cpp -- the grid's clearance and costmap through the drop-in C++ headers: KinematicICP::GridClearance, GridCostmap
// and GridLastWindow, used the way a node keeps a costmap current - after every RegisterFrame only the last window grown by the radius
// is refreshed.
// Input: the drive file tests/test_clearance_facade.py writes (the format of tests/test_grid_facade.py's), a file with the eight doubles
// of the grid's configuration followed by radius_cells, inscribed_radius and cost_scaling_factor, and a prefix for what it writes:
//   <prefix>_poses.bin     per frame the pose (7 doubles)
//   <prefix>_windows.bin   per frame GridLastWindow() as 4 x uint32
//   <prefix>_counts.bin    the counters after the drive
//   <prefix>_table.bin     kicp_grid_cost_table_nav2's table
//   <prefix>_kept.bin      the costmap a node would hold: the full one before the drive, refreshed per frame in the grown window only
//   <prefix>_costmap.bin, <prefix>_clearance.bin   the full grid's GridCostmap (uint8) and GridClearance (uint16) after the drive
//   <prefix>_patch.bin     GridClearance of the last frame's grown window
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
        const auto gc = read_doubles(g, 11);
        const kicp_bridge::GridConfig grid_config{gc[0], gc[1], gc[2], static_cast<unsigned int>(gc[3]), static_cast<unsigned int>(gc[4]), gc[5], gc[6], gc[7]};
        const int radius = static_cast<int>(gc[8]);
        const kicp_bridge::GridClearanceConfig clearance_config{1u, 0.65, 0, radius};
        std::vector<uint8_t> table(static_cast<size_t>(radius) * radius + 2);
        kicp_bridge::check(kicp_grid_cost_table_nav2(grid_config.cell, radius, gc[9], gc[10], table.data(), table.size()), "kicp_grid_cost_table_nav2");
        write_file(prefix + "_table.bin", table);

        KinematicICP icp(cfg);
        std::vector<uint16_t> clearance;
        std::vector<uint8_t> kept, patch;
        const bool r1 = refused([&] { icp.GridClearance(clearance, clearance_config); }), r2 = refused([&] { icp.GridCostmap(kept, clearance_config, table); });
        const bool r3 = refused([&] { icp.GridLastWindow(); });
        printf("refused_without_grid %d %d %d\n", r1 ? 1 : 0, r2 ? 1 : 0, r3 ? 1 : 0);
        icp.EnableGrid(grid_config);
        printf("window_before_any_frame_is_empty %d\n", icp.GridLastWindow().empty() ? 1 : 0);
        icp.GridCostmap(kept, clearance_config, table, true);
        const unsigned int W = grid_config.width, H = grid_config.height;
        std::vector<double> poses;
        std::vector<uint32_t> windows;
        kicp_bridge::GridRect grown;
        for (size_t k = 0; k < static_cast<size_t>(h[0]); ++k) {
            const auto n = read_doubles(f, 1);
            const auto points = to_points(read_doubles(f, static_cast<size_t>(n[0]) * 3));
            const auto stamps = read_doubles(f, static_cast<size_t>(n[0]));
            const Sophus::SE3d delta = kicp_bridge::from_params(read_doubles(f, 7).data());
            icp.RegisterFrame(points, stamps, ext, delta);
            double p[7];
            kicp_bridge::to_params(icp.pose(), p);
            poses.insert(poses.end(), p, p + 7);
            const kicp_bridge::GridRect window = icp.GridLastWindow();
            for (unsigned int v : {window.x0, window.y0, window.w, window.h}) windows.push_back(v);
            if (window.empty()) continue;
            grown = window.grown(static_cast<unsigned int>(radius), W, H);
            icp.GridCostmap(patch, clearance_config, table, true, &grown);
            for (unsigned int y = 0; y < grown.h; ++y)
                std::memcpy(&kept[static_cast<size_t>(grown.y0 + y) * W + grown.x0], &patch[static_cast<size_t>(y) * grown.w], grown.w);
        }
        write_file(prefix + "_poses.bin", poses), write_file(prefix + "_windows.bin", windows), write_file(prefix + "_kept.bin", kept);
        std::vector<uint8_t> full;
        icp.GridCostmap(full, clearance_config, table, true);
        icp.GridClearance(clearance, clearance_config);
        write_file(prefix + "_costmap.bin", full), write_file(prefix + "_clearance.bin", clearance);
        icp.GridClearance(clearance, clearance_config, &grown);
        write_file(prefix + "_patch.bin", clearance);
        std::vector<unsigned short> counts(2 * static_cast<size_t>(W) * H);
        kicp_bridge::check(kicp_grid_counts(icp.Grid().get(), counts.data(), counts.size() / 2), "kicp_grid_counts");
        write_file(prefix + "_counts.bin", counts);
        kicp_bridge::GridRect outside;
        outside.x0 = W - 1, outside.y0 = 0, outside.w = 2, outside.h = 1;
        printf("refused_outside_the_grid %d\n", refused([&] { icp.GridClearance(clearance, clearance_config, &outside); }) ? 1 : 0);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
