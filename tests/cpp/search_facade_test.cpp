// search_facade_test.cpp -- the whole-map relocalisation through the drop-in C++ headers: KinematicICP::BuildOccupancy and
// KinematicICP::RelocalizeSearch on a loaded map (Config::update_map = false), and KinematicRegistration::RelocalizeSearch on a pyramid
// built through kicp_bridge::build_occupancy.
// Input: a map file (PCD with the `# kicp_map` line), and a file of doubles tests/test_search_facade.py writes: cell, dilate, levels,
// top_m, max_iterations, convergence, centre x, centre y, half x, half y, z, yaw step, n, the n keypoints.  Output: text on stdout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kinematic_icp/pipeline/KinematicICP.hpp"

static std::vector<double> read_doubles(FILE *f, size_t n) {
    std::vector<double> v(n);
    if (n && fread(v.data(), sizeof(double), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}
static void print_pose(const char *tag, const Sophus::SE3d &T) {
    double p[7];
    kicp_bridge::to_params(T, p);
    printf("%s %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", tag, p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 1;
    try {
        const auto h = read_doubles(f, 13);
        const double cell = h[0], convergence = h[5];
        const int dilate = static_cast<int>(h[1]), levels = static_cast<int>(h[2]), max_iterations = static_cast<int>(h[4]);
        const size_t top_m = static_cast<size_t>(h[3]), n = static_cast<size_t>(h[12]);
        const auto xyz = read_doubles(f, 3 * n);
        std::vector<Eigen::Vector3d> keypoints(n);
        if (n) std::memcpy(keypoints.front().data(), xyz.data(), xyz.size() * sizeof(double));
        kinematic_icp::pipeline::Config cfg;
        cfg.update_map = false;
        kinematic_icp::pipeline::KinematicICP localizer(cfg);
        localizer.LoadMap(argv[1]);
        bool refused = false;
        try {
            localizer.RelocalizeSearch(keypoints, kicp_search_window{});
        } catch (const std::runtime_error &) {
            refused = true;  // no pyramid yet
        }
        printf("refused_without_pyramid %d\n", refused ? 1 : 0);
        localizer.BuildOccupancy(cell, dilate, levels);
        int dims[3];
        unsigned long long set_cells = 0;
        kicp_bridge::check(kicp_occ_info(localizer.Occupancy(), nullptr, dims, nullptr, nullptr, nullptr, &set_cells), "kicp_occ_info");
        printf("occupancy %d %d %d %llu\n", dims[0], dims[1], dims[2], set_cells);
        const kicp_search_window window = kicp_bridge::search_window_around(localizer.Occupancy(), Eigen::Vector2d(h[6], h[7]), h[8], h[9], h[10], h[11]);
        printf("window %.17g %.17g %.17g %u %u %.17g %.17g %u\n", window.x0, window.y0, window.z, window.nx, window.ny, window.yaw0, window.yaw_step, window.nyaw);
        const auto found = localizer.RelocalizeSearch(keypoints, window, top_m, max_iterations, convergence);
        print_pose("relocalized_pose", found.pose);
        printf("relocalized %zu %.17g %.17g %d\n", found.candidate, found.cost_before, found.cost_after, found.refined ? 1 : 0);
        print_pose("pose_after_relocalize", localizer.pose());
        // the registration's entry point on a pyramid of its own, at the threshold the pipeline used
        kinematic_icp::KinematicRegistration registration(cfg.max_num_iterations, cfg.convergence_criterion, cfg.max_num_threads, true, 0.0);
        const auto occ = kicp_bridge::build_occupancy(localizer.VoxelMap().handle(), cell, dilate, levels);
        const auto again = registration.RelocalizeSearch(keypoints, localizer.VoxelMap(), occ.get(), window, 3.0 * cfg.map_resolution(), top_m, max_iterations,
                                                         convergence);
        print_pose("registration_pose", again.pose);
        printf("registration %zu %.17g %.17g %d\n", again.candidate, again.cost_before, again.cost_after, again.refined ? 1 : 0);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f);
    return 0;
}
