// localization_facade_test.cpp -- localising in a saved map through the drop-in C++ headers: SaveMap / LoadMap, Config::update_map =
// false (the map is a prior: RegisterFrame does everything but the map update), Relocalize from a planar grid of candidates.
// Input: the drive file tests/test_localization_facade.py writes (the format of tests/test_facade.py's pipeline mode) and three
// paths to write: the map, the keypoints of the fourth frame, the candidates.  Output: poses and map fingerprints as text on stdout.
#include <cstdint>
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
static std::vector<Eigen::Vector3d> to_points(const std::vector<double> &v) {
    std::vector<Eigen::Vector3d> p(v.size() / 3);
    if (!p.empty()) std::memcpy(p.front().data(), v.data(), v.size() * sizeof(double));
    return p;
}
static void print_pose(const char *tag, const Sophus::SE3d &T) {
    double p[7];
    kicp_bridge::to_params(T, p);
    printf("%s %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", tag, p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
}
static void write_doubles(const std::string &path, const double *v, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(v, sizeof(double), n, f) != n) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
    fclose(f);
}
// the map as the node would publish it: number of points and an FNV-1a hash of the PointCloud2 bytes
static void print_map(const char *tag, kinematic_icp::pipeline::KinematicICP &icp) {
    std::vector<uint8_t> data;
    icp.LocalMapF32(data);
    uint64_t h = 1469598103934665603ull;
    for (uint8_t b : data) h = (h ^ b) * 1099511628211ull;
    printf("%s %zu %016llx\n", tag, data.size() / kicp_bridge::PointCloud2Xyz32::point_step, static_cast<unsigned long long>(h));
}
struct Frame {
    std::vector<Eigen::Vector3d> points;
    std::vector<double> stamps;
    Sophus::SE3d delta;
};

int main(int argc, char **argv) {
    if (argc < 5) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    const std::string map_path = argv[2], keypoints_path = argv[3], candidates_path = argv[4];
    try {
        const auto h = read_doubles(f, 4);  // n_frames, voxel, max_range, deskew
        kinematic_icp::pipeline::Config cfg;
        cfg.voxel_size = h[1], cfg.max_range = h[2], cfg.deskew = h[3] != 0.0;
        const Sophus::SE3d ext = kicp_bridge::from_params(read_doubles(f, 7).data());
        std::vector<Frame> frames(static_cast<size_t>(h[0]));
        for (Frame &fr : frames) {
            const auto n = read_doubles(f, 1);
            fr.points = to_points(read_doubles(f, static_cast<size_t>(n[0]) * 3));
            fr.stamps = read_doubles(f, static_cast<size_t>(n[0]));
            fr.delta = kicp_bridge::from_params(read_doubles(f, 7).data());
        }
        // mapping: the first three frames with the map update, then the map goes to a file ... and the drive goes on (the default
        // Config behaves as it always did)
        kinematic_icp::pipeline::KinematicICP mapper(cfg);
        for (size_t k = 0; k < 3; ++k) {
            mapper.RegisterFrame(frames[k].points, frames[k].stamps, ext, frames[k].delta);
            print_pose("mapping_pose", mapper.pose());
        }
        mapper.SaveMap(map_path);
        print_map("saved_map", mapper);
        const Sophus::SE3d pose3 = mapper.pose();
        for (size_t k = 3; k < frames.size(); ++k) {
            mapper.RegisterFrame(frames[k].points, frames[k].stamps, ext, frames[k].delta);
            print_pose("mapping_pose", mapper.pose());
        }
        printf("mapping_map_points %zu\n", mapper.LocalMap().size());
        // localisation: a fresh pipeline that never updates its map
        cfg.update_map = false;
        kinematic_icp::pipeline::KinematicICP localizer(cfg);
        localizer.LoadMap(map_path);
        localizer.SetPose(pose3);  // (moves the robot, not the map)
        print_map("loaded_map", localizer);
        std::vector<Eigen::Vector3d> keypoints;
        Sophus::SE3d pose4;
        for (size_t k = 3; k < frames.size(); ++k) {
            const auto [deskewed, source] = localizer.RegisterFrame(frames[k].points, frames[k].stamps, ext, frames[k].delta);
            print_pose("frozen_pose", localizer.pose());
            print_map("frozen_map", localizer);
            if (k == 3) keypoints = source, pose4 = localizer.pose();
        }
        // Relocalize: the fourth frame's keypoints (base frame) against a 5 x 5 x 5 grid around that frame's pose, off its centre
        const double s = 0.5 * cfg.voxel_size, a = 0.05;
        const Sophus::SE3d center = pose4 * Sophus::SE3d(Eigen::Quaterniond(std::cos(0.03), 0.0, 0.0, std::sin(0.03)), Eigen::Vector3d(0.3 * s, -0.4 * s, 0.0));
        const std::vector<Sophus::SE3d> grid = kicp_bridge::planar_grid(center, 2.0 * s, 2.0 * s, 2.0 * a, s, s, a);
        const std::vector<double> flat = kicp_bridge::to_params(grid);
        write_doubles(keypoints_path, keypoints.front().data(), keypoints.size() * 3);
        write_doubles(candidates_path, flat.data(), flat.size());
        print_pose("grid_center", center);
        const auto found = localizer.Relocalize(keypoints, grid, 4);
        print_pose("relocalized_pose", found.pose);
        printf("relocalized %zu %.17g %.17g %d %zu\n", found.candidate, found.cost_before, found.cost_after, found.refined ? 1 : 0, grid.size());
        print_pose("pose_after_relocalize", localizer.pose());
        print_map("map_after_relocalize", localizer);
        // the scores behind it, through the registration's own entry point
        const auto scores = kinematic_icp::KinematicRegistration(cfg.max_num_iterations, cfg.convergence_criterion, cfg.max_num_threads, true, 0.0)
                                .ScorePoses(keypoints, localizer.VoxelMap(), grid, 3.0 * cfg.map_resolution());
        printf("score_of_winner %.17g %.17g\n", scores[found.candidate].first, scores[found.candidate].second);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f);
    return 0;
}
