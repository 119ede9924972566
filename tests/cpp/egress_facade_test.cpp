// egress_facade_test.cpp -- the published clouds as PointCloud2 `data` (ros/.../LidarOdometryServer.cpp:240-263 PublishClouds,
// utils/RosUtils.cpp:40-63 EigenToPointCloud2) through the drop-in headers: KinematicICP::RegisterFrameF32 /
// RegisterIngestedFrameF32 / LocalMapF32 beside the fp64 RegisterFrame / RegisterIngestedFrame / LocalMap.
// Input: a little binary file written by tests/test_gpu_egress.py or tools/bench_egress.py; output: text on stdout.
//   drive FILE FEED [DUMP]  four pipelines on the same frames: (a) fp64, (b) FLOAT32 with both outputs, (c) FLOAT32 with both
//                           outputs null, (d) fp64 and FLOAT32 frames alternating.  FEED: host (RegisterFrame[F32] on the decoded
//                           cloud), raw (IngestCloud), ahead (IngestCloud with the next message announced), scan (IngestScan).
//                           Per frame one line: "frame k n_frame n_source n_map" and every mismatch found, bit for bit, against
//                           static_cast<float> of (a)'s clouds (the map: of (b)'s own LocalMap(), and as sorted records of (a)'s).  DUMP: (b)'s LocalMapF32 bytes per frame (n as uint64, then the bytes).
//   timed FILE FEED         the drive through (a) with the node's three conversions (EigenToPointCloud2's loop), (b) and (c), one
//                           after the other on each frame, a clock around each whole frame; then "map" timings: LocalMap() + the
//                           conversion against LocalMapF32 on the final map, `reps` times each.
//   bigmap N REPS           a map of about N points (kiss_icp::VoxelHashMap, 1 m voxels, 20 points each, filled by bulk AddPoints
//                           on the GPU): Pointcloud() + the conversion against PointcloudF32, REPS times each, and whether they agree.
// File: kind (0 cloud, 1 scan), n_frames, voxel, max_range, min_range, deskew, lidar_to_base[7] (doubles); kind 1 also angle_min,
// angle_max, angle_increment, range_min, range_max.  Per frame: n (double); kind 0: n records x y z t (FLOAT32, 16 B); kind 1:
// time_increment (double) and n float32 ranges; then the relative odometry[7].
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kinematic_icp/pipeline/KinematicICP.hpp"

using kinematic_icp::pipeline::KinematicICP;
using Clock = std::chrono::steady_clock;

template <typename T>
static std::vector<T> read_n(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}
struct Frame {
    std::vector<float> data;  // kind 0: x y z t records; kind 1: ranges
    double time_increment = 0.0;
    std::vector<double> delta;
    std::vector<Eigen::Vector3d> xyz;  // kind 0: the decoded cloud (PointCloud2ToEigen)
    std::vector<double> stamps;        // ... and its stamps normalised to [0, 1] (TimeStampHandler)
};
// what EigenToPointCloud2 writes into msg->data (RosUtils.cpp:40-63): the doubles through static_cast<float>, 12 bytes per point
static void eigen_to_data(const std::vector<Eigen::Vector3d> &points, std::vector<uint8_t> &data) {
    data.resize(points.size() * 12);
    float *out = reinterpret_cast<float *>(data.data());
    for (size_t i = 0; i < points.size(); ++i)
        out[3 * i] = static_cast<float>(points[i].x()), out[3 * i + 1] = static_cast<float>(points[i].y()), out[3 * i + 2] = static_cast<float>(points[i].z());
}
// the records as a sorted list: two maps with the same points may list them in different orders (the device update claims table
// slots with atomics, so where a voxel lands in its probe sequence can differ from run to run)
static std::vector<std::array<uint32_t, 3>> sorted_records(const std::vector<uint8_t> &data) {
    std::vector<std::array<uint32_t, 3>> r(data.size() / 12);
    if (!r.empty()) std::memcpy(r.data(), data.data(), data.size());
    std::sort(r.begin(), r.end());
    return r;
}
static bool same_pose(const Sophus::SE3d &a, const Sophus::SE3d &b) {
    double p[7], q[7];
    kicp_bridge::to_params(a, p), kicp_bridge::to_params(b, q);
    return std::memcmp(p, q, sizeof p) == 0;
}

struct Drive {
    int kind = 0;
    kinematic_icp::pipeline::Config cfg;
    Sophus::SE3d lidar_to_base;
    kicp_laser_scan scan{};
    std::vector<Frame> frames;
    const kicp_cloud_layout layout{16, 0, 4, 8, KICP_FIELD_FLOAT32, 12};
    std::string feed;

    void load(const char *path) {
        FILE *f = fopen(path, "rb");
        if (!f) exit(1);
        const auto h = read_n<double>(f, 6);
        kind = static_cast<int>(h[0]);
        cfg.voxel_size = h[2], cfg.max_range = h[3], cfg.min_range = h[4], cfg.deskew = h[5] != 0.0;
        lidar_to_base = kicp_bridge::from_params(read_n<double>(f, 7).data());
        if (kind == 1) {
            const auto sp = read_n<double>(f, 5);
            scan = kicp_laser_scan{static_cast<float>(sp[0]), static_cast<float>(sp[1]), static_cast<float>(sp[2]), 0.0f, static_cast<float>(sp[3]),
                                   static_cast<float>(sp[4])};
        }
        frames.resize(static_cast<size_t>(h[1]));
        for (auto &fr : frames) {
            const size_t n = static_cast<size_t>(read_n<double>(f, 1)[0]);
            if (kind == 1) fr.time_increment = read_n<double>(f, 1)[0];
            fr.data = read_n<float>(f, kind == 1 ? n : 4 * n);
            fr.delta = read_n<double>(f, 7);
            if (kind == 0) {  // the host feed: PointCloud2ToEigen + the stamps normalised as TimeStampHandler does
                fr.xyz.resize(n), fr.stamps.resize(n);
                double lo = 0.0, hi = 0.0;
                for (size_t i = 0; i < n; ++i) {
                    fr.xyz[i] = Eigen::Vector3d(fr.data[4 * i], fr.data[4 * i + 1], fr.data[4 * i + 2]);
                    const double t = fr.data[4 * i + 3];
                    lo = i == 0 ? t : std::min(lo, t), hi = i == 0 ? t : std::max(hi, t);
                }
                for (size_t i = 0; i < n; ++i) fr.stamps[i] = (static_cast<double>(fr.data[4 * i + 3]) - lo) / (hi - lo);
            }
        }
        fclose(f);
    }
    // the message of frame k into the pipeline (feeds raw / ahead / scan); host: nothing to do
    void ingest(KinematicICP &icp, size_t k) {
        const Frame &fr = frames[k];
        if (feed == "scan") {
            kicp_laser_scan s = scan;
            s.time_increment = static_cast<float>(fr.time_increment);
            (void)icp.IngestScan(fr.data.data(), fr.data.size(), s);
        } else if (feed == "raw" || feed == "ahead") {
            (void)icp.IngestCloud(fr.data.data(), fr.data.size() / 4, layout);
            if (feed == "ahead" && k + 1 < frames.size()) icp.AnnounceNextCloud(frames[k + 1].data.data(), frames[k + 1].data.size() / 4, layout);
        }
    }
    KinematicICP::Vector3dVectorTuple fp64(KinematicICP &icp, size_t k) {
        const Frame &fr = frames[k];
        const Sophus::SE3d delta = kicp_bridge::from_params(fr.delta.data());
        if (feed == "host") return icp.RegisterFrame(fr.xyz, cfg.deskew ? fr.stamps : std::vector<double>(), lidar_to_base, delta);
        ingest(icp, k);
        return icp.RegisterIngestedFrame(lidar_to_base, delta);
    }
    void f32(KinematicICP &icp, size_t k, std::vector<uint8_t> *frame_data, std::vector<uint8_t> *keypoints_data) {
        const Frame &fr = frames[k];
        const Sophus::SE3d delta = kicp_bridge::from_params(fr.delta.data());
        if (feed == "host") return icp.RegisterFrameF32(fr.xyz, cfg.deskew ? fr.stamps : std::vector<double>(), lidar_to_base, delta, frame_data, keypoints_data);
        ingest(icp, k);
        icp.RegisterIngestedFrameF32(lidar_to_base, delta, frame_data, keypoints_data);
    }
};

static double median(std::vector<double> v, double q) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[std::min(v.size() - 1, static_cast<size_t>(q * static_cast<double>(v.size() - 1) + 0.5))];
}
static void report(const char *what, const std::vector<double> &ms) {
    printf("%s median %.4f p10 %.4f p90 %.4f n %zu\n", what, median(ms, 0.5), median(ms, 0.1), median(ms, 0.9), ms.size());
}

static int bigmap(size_t n, int reps) {
    kiss_icp::VoxelHashMap map(1.0, 1e6, 20);
    std::vector<Eigen::Vector3d> pts(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto uniform = [&s] { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<double>(s >> 11) * 0x1.0p-53; };
    const double side = std::cbrt(static_cast<double>(n) / 12.0 / 4.0);  // a slab 4 x side x side voxels tall, ~12 points per voxel kept
    for (auto &p : pts) p = Eigen::Vector3d(uniform() * side * 4.0, uniform() * side, uniform() * side * 0.25 * 4.0);
    for (size_t lo = 0; lo < n; lo += 262144) map.AddPoints(std::vector<Eigen::Vector3d>(pts.begin() + lo, pts.begin() + std::min(n, lo + 262144)));
    std::vector<double> ms_a, ms_b;
    std::vector<uint8_t> last_a, last_b;
    for (int r = 0; r < reps; ++r) {
        auto t0 = Clock::now();
        {
            std::vector<uint8_t> m;
            eigen_to_data(map.Pointcloud(), m);
            if (r == reps - 1) last_a.swap(m);
        }
        ms_a.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
        t0 = Clock::now();
        {
            std::vector<uint8_t> m;
            map.PointcloudF32(m);
            if (r == reps - 1) last_b.swap(m);
        }
        ms_b.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
    }
    report("map_fp64_plus_conversion", ms_a);
    report("map_f32", ms_b);
    printf("map_points %zu on_device %d equal %d\n", last_a.size() / 12, kicp_map_last_update_on_device(map.handle()), last_a == last_b ? 1 : 0);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) return 1;
    const std::string mode = argv[1];
    if (mode == "bigmap") {
        try {
            return bigmap(static_cast<size_t>(std::atof(argv[2])), std::atoi(argv[3]));
        } catch (const std::exception &e) {
            fprintf(stderr, "exception: %s\n", e.what());
            return 3;
        }
    }
    Drive d;
    d.load(argv[2]);
    d.feed = argv[3];
    try {
        if (mode == "drive") {
            FILE *dump = argc > 4 ? fopen(argv[4], "wb") : nullptr;
            KinematicICP a(d.cfg), b(d.cfg), c(d.cfg), alt(d.cfg);
            std::vector<uint8_t> fa, sa, fb, sb, ma, mb, mbb, falt, salt;
            for (size_t k = 0; k < d.frames.size(); ++k) {
                std::string bad;
                const auto [frame_a, source_a] = d.fp64(a, k);
                d.f32(b, k, &fb, &sb);
                d.f32(c, k, nullptr, nullptr);
                eigen_to_data(frame_a, fa), eigen_to_data(source_a, sa);
                if (fb != fa) bad += " frame_bytes";
                if (sb != sa) bad += " keypoint_bytes";
                if (k % 2 == 0) {
                    const auto [frame_d, source_d] = d.fp64(alt, k);
                    eigen_to_data(frame_d, falt), eigen_to_data(source_d, salt);
                } else {
                    d.f32(alt, k, &falt, &salt);
                }
                if (falt != fa || salt != sa) bad += " alternating_clouds";
                if (!same_pose(a.pose(), b.pose())) bad += " pose_f32";
                if (!same_pose(a.pose(), c.pose())) bad += " pose_null";
                if (!same_pose(a.pose(), alt.pose())) bad += " pose_alternating";
                const auto map_a = a.LocalMap();
                eigen_to_data(map_a, ma);
                b.LocalMapF32(mb);
                eigen_to_data(b.LocalMap(), mbb);
                if (mb != mbb) bad += " map_bytes";                              // the same map, bit for bit and in order
                if (sorted_records(mb) != sorted_records(ma)) bad += " map_points";  // the fp64 pipeline's map: the same points
                if (c.LocalMap().size() != map_a.size() || alt.LocalMap().size() != map_a.size()) bad += " map_size";
                printf("frame %zu %zu %zu %zu%s\n", k, frame_a.size(), source_a.size(), map_a.size(), bad.c_str());
                if (dump) {
                    const uint64_t n = mb.size() / 12;
                    fwrite(&n, 8, 1, dump), fwrite(mb.data(), 1, mb.size(), dump);
                }
            }
            if (dump) fclose(dump);
        } else if (mode == "timed") {
            const int reps = argc > 4 ? std::atoi(argv[4]) : 50;
            KinematicICP a(d.cfg), b(d.cfg), c(d.cfg);
            std::vector<uint8_t> msg_frame, msg_kp, msg_map;  // (the node builds fresh messages: fresh vectors each frame)
            std::vector<double> ms_a, ms_b, ms_c;
            size_t mismatches = 0, map_mismatches = 0;
            for (size_t k = 0; k < d.frames.size(); ++k) {
                auto t0 = Clock::now();
                {
                    const auto [frame, source] = d.fp64(a, k);
                    std::vector<uint8_t> m0, m1, m2;
                    eigen_to_data(frame, m0), eigen_to_data(source, m1), eigen_to_data(a.LocalMap(), m2);
                    msg_frame.swap(m0), msg_kp.swap(m1), msg_map.swap(m2);
                }
                ms_a.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                std::vector<uint8_t> m0, m1, m2;
                t0 = Clock::now();
                d.f32(b, k, &m0, &m1);
                b.LocalMapF32(m2);
                ms_b.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                mismatches += (m0 != msg_frame) + (m1 != msg_kp);  // (outside the clock)
                map_mismatches += sorted_records(m2) != sorted_records(msg_map);  // (another pipeline's map: its order may differ)
                t0 = Clock::now();
                d.f32(c, k, nullptr, nullptr);
                ms_c.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
            }
            report("drive_fp64_three_conversions", ms_a);
            report("drive_f32_all_outputs", ms_b);
            report("drive_f32_null_outputs", ms_c);
            std::vector<double> map_a, map_b;
            size_t n_map = 0;
            for (int r = 0; r < reps; ++r) {
                auto t0 = Clock::now();
                {
                    std::vector<uint8_t> m;
                    eigen_to_data(a.LocalMap(), m);
                    n_map = m.size() / 12;
                }
                map_a.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                t0 = Clock::now();
                {
                    std::vector<uint8_t> m;
                    b.LocalMapF32(m);
                }
                map_b.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
            }
            report("map_fp64_plus_conversion", map_a);
            report("map_f32", map_b);
            printf("map_points %zu cloud_mismatches %zu map_mismatches %zu poses_equal %d\n", n_map, mismatches, map_mismatches,
                   same_pose(a.pose(), b.pose()) && same_pose(a.pose(), c.pose()) ? 1 : 0);
        } else {
            fprintf(stderr, "unknown mode %s\n", mode.c_str());
            return 1;
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
