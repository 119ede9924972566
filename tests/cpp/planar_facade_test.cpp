// planar_facade_test.cpp -- the planar refinement through the drop-in C++ headers: KinematicICP::RelocalizePlanar on a loaded map
// (Config::update_map = false) and KinematicRegistration::RefinePosesPlanar on the same inputs.
// Input: a map file (PCD with the `# kicp_map` line), and a file of doubles tests/test_planar_facade.py writes: top_m, max_iterations,
// convergence, n, count, the n keypoints, the count candidate poses.  Output: poses and figures as text on stdout.
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
        const auto h = read_doubles(f, 5);  // top_m, max_iterations, convergence, n, count
        const size_t top_m = static_cast<size_t>(h[0]), n = static_cast<size_t>(h[3]), count = static_cast<size_t>(h[4]);
        const int max_iterations = static_cast<int>(h[1]);
        const double convergence = h[2];
        const auto xyz = read_doubles(f, 3 * n);
        std::vector<Eigen::Vector3d> keypoints(n);
        if (n) std::memcpy(keypoints.front().data(), xyz.data(), xyz.size() * sizeof(double));
        const auto flat = read_doubles(f, 7 * count);
        std::vector<Sophus::SE3d> candidates(count);
        for (size_t k = 0; k < count; ++k) candidates[k] = kicp_bridge::from_params(&flat[7 * k]);
        kinematic_icp::pipeline::Config cfg;
        cfg.update_map = false;
        kinematic_icp::pipeline::KinematicICP localizer(cfg);
        localizer.LoadMap(argv[1]);
        printf("map_points %zu\n", localizer.LocalMap().size());
        const auto found = localizer.RelocalizePlanar(keypoints, candidates, top_m, max_iterations, convergence);
        print_pose("relocalized_pose", found.pose);
        printf("relocalized %zu %.17g %.17g %d\n", found.candidate, found.cost_before, found.cost_after, found.refined ? 1 : 0);
        print_pose("pose_after_relocalize", localizer.pose());
        printf("map_points_after %zu\n", localizer.LocalMap().size());
        // the refinement on its own, through the registration's entry point, at the threshold RelocalizePlanar used
        kinematic_icp::KinematicRegistration registration(cfg.max_num_iterations, cfg.convergence_criterion, cfg.max_num_threads, true, 0.0);
        const std::vector<Sophus::SE3d> some(candidates.begin(), candidates.begin() + std::min<size_t>(count, 5));
        const auto refined = registration.RefinePosesPlanar(keypoints, localizer.VoxelMap(), some, 3.0 * cfg.map_resolution(), max_iterations, convergence);
        for (const auto &r : refined) {
            print_pose("refined_pose", r.pose);
            printf("refined %d %d\n", r.iterations, r.status);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f);
    return 0;
}
