// laserscan_facade_test.cpp -- the 2-D LiDAR mode of the node (ros/src/kinematic_icp_ros/nodes/online_node.cpp:44-58) through the
// drop-in headers: KinematicICP::IngestScan + RegisterIngestedFrame on the raw LaserScan ranges.
// Input: a little binary file written by tests/test_laserscan.py or tools/bench_laserscan.py; output: text on stdout.
//   scan_pipeline FILE  one pipeline, every frame: pose, sizes, the stamps IngestScan returned
//   scan_timed FILE     two pipelines on the same frames, alternating, a clock around each whole frame:
//                       (a) IngestScan + RegisterIngestedFrame;
//                       (b) the projection on the host by the same rules into 16-byte PointCloud2 records (what a node does today
//                           with laser_geometry), then IngestCloud + RegisterIngestedFrame
// File: n_frames, voxel, max_range, min_range, deskew, range_cutoff, lidar_to_base[7], angle_min, angle_max, angle_increment,
// range_min, range_max (doubles); per frame: n (double), time_increment (double), n float32 ranges, relative odometry[7].
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kinematic_icp/pipeline/KinematicICP.hpp"

template <typename T>
static std::vector<T> read_n(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
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

// laser_geometry's projector on the host, by the rules kicp_pre_ingest.hpp (laser_rules) states [RECALLED]: the cosine table cached while
// n, angle_min and angle_max stay the same; the kept beams as x y z stamps FLOAT32 records
struct HostProjector {
    std::vector<double> table;
    size_t n = 0;
    float angle_min = 0.0f, angle_max = 0.0f;
    bool valid = false;
    std::vector<float> records;
    size_t project(const float *ranges, size_t count, const kicp_laser_scan &s, double range_cutoff) {
        if (!valid || count != n || s.angle_min != angle_min || s.angle_max != angle_max) {
            table.resize(2 * count);
            for (size_t i = 0; i < count; ++i) {
                const float step = static_cast<float>(i) * s.angle_increment;
                const float a = s.angle_min + step;
                table[2 * i] = std::cos(static_cast<double>(a)), table[2 * i + 1] = std::sin(static_cast<double>(a));
            }
            valid = true, n = count, angle_min = s.angle_min, angle_max = s.angle_max;
        }
        const double cutoff = range_cutoff < 0.0 ? static_cast<double>(s.range_max) : range_cutoff;
        records.resize(4 * count);
        size_t k = 0;
        for (size_t i = 0; i < count; ++i) {
            const float r = ranges[i];
            if (!(r < cutoff && r >= s.range_min)) continue;
            records[4 * k] = static_cast<float>(static_cast<double>(r) * table[2 * i]);
            records[4 * k + 1] = static_cast<float>(static_cast<double>(r) * table[2 * i + 1]);
            records[4 * k + 2] = 0.0f;
            records[4 * k + 3] = static_cast<float>(i) * s.time_increment;
            ++k;
        }
        return k;
    }
};

struct Frame {
    std::vector<float> ranges;
    float time_increment;
    std::vector<double> delta;
};

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    const std::string mode = argv[1];
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 1;
    try {
        const auto h = read_n<double>(f, 6);  // n_frames, voxel, max_range, min_range, deskew, range_cutoff
        const auto ext = read_n<double>(f, 7);
        const auto sp = read_n<double>(f, 5);
        kicp_laser_scan scan{static_cast<float>(sp[0]), static_cast<float>(sp[1]), static_cast<float>(sp[2]), 0.0f, static_cast<float>(sp[3]),
                             static_cast<float>(sp[4])};
        const double range_cutoff = h[5];
        std::vector<Frame> frames(static_cast<size_t>(h[0]));
        for (auto &fr : frames) {
            const auto head = read_n<double>(f, 2);
            fr.time_increment = static_cast<float>(head[1]);
            fr.ranges = read_n<float>(f, static_cast<size_t>(head[0]));
            fr.delta = read_n<double>(f, 7);
        }
        kinematic_icp::pipeline::Config cfg;
        cfg.voxel_size = h[1], cfg.max_range = h[2], cfg.min_range = h[3], cfg.deskew = h[4] != 0.0;
        const Sophus::SE3d lidar_to_base = kicp_bridge::from_params(ext.data());
        if (mode == "scan_pipeline") {
            kinematic_icp::pipeline::KinematicICP icp(cfg);
            for (const auto &fr : frames) {
                scan.time_increment = fr.time_increment;
                const auto [has_stamps, lo, hi] = icp.IngestScan(fr.ranges.data(), fr.ranges.size(), scan, range_cutoff);
                const auto [deskewed, source] = icp.RegisterIngestedFrame(lidar_to_base, kicp_bridge::from_params(fr.delta.data()));
                print_pose("pose", icp.pose());
                printf("sizes %zu %zu %zu\n", deskewed.size(), source.size(), icp.LocalMap().size());
                printf("stamps %d %.17g %.17g\n", has_stamps ? 1 : 0, lo, hi);
            }
        } else if (mode == "scan_timed") {
            kinematic_icp::pipeline::KinematicICP icp_a(cfg), icp_b(cfg);
            HostProjector projector;
            const kicp_cloud_layout layout{16, 0, 4, 8, KICP_FIELD_FLOAT32, 12};
            std::vector<double> ms_a, ms_b;
            std::vector<Sophus::SE3d> pose_a, pose_b;
            auto run_a = [&](const Frame &fr) {
                const auto t0 = std::chrono::steady_clock::now();
                {
                    (void)icp_a.IngestScan(fr.ranges.data(), fr.ranges.size(), scan, range_cutoff);
                    (void)icp_a.RegisterIngestedFrame(lidar_to_base, kicp_bridge::from_params(fr.delta.data()));
                }
                ms_a.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                pose_a.push_back(icp_a.pose());
            };
            auto run_b = [&](const Frame &fr) {
                const auto t0 = std::chrono::steady_clock::now();
                {
                    const size_t kept = projector.project(fr.ranges.data(), fr.ranges.size(), scan, range_cutoff);
                    (void)icp_b.IngestCloud(projector.records.data(), kept, layout);
                    (void)icp_b.RegisterIngestedFrame(lidar_to_base, kicp_bridge::from_params(fr.delta.data()));
                }
                ms_b.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                pose_b.push_back(icp_b.pose());
            };
            for (size_t k = 0; k < frames.size(); ++k) {  // (which of the two goes first alternates from frame to frame)
                scan.time_increment = frames[k].time_increment;
                if (k % 2 == 0) run_a(frames[k]), run_b(frames[k]);
                else run_b(frames[k]), run_a(frames[k]);
            }
            const size_t map_a = icp_a.LocalMap().size(), map_b = icp_b.LocalMap().size();
            for (size_t k = 0; k < frames.size(); ++k) {
                printf("frame %zu a_ms %.4f b_ms %.4f\n", k, ms_a[k], ms_b[k]);
                print_pose("pose_a", pose_a[k]);
                print_pose("pose_b", pose_b[k]);
            }
            printf("map %zu %zu\n", map_a, map_b);
        } else {
            fprintf(stderr, "unknown mode %s\n", mode.c_str());
            return 1;
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f);
    return 0;
}
