// view_facade_test.cpp -- see-through removal through the drop-in C++ headers: KinematicICP::EnableSeeThroughRemoval,
// DisableSeeThroughRemoval, LastRemoval, View and the copy of the view with the object.
// Input: the drive file tests/test_view_facade.py writes (the format of tests/test_facade.py's pipeline mode), a file with the six
// doubles of the view's configuration, and a prefix for what it writes - per run <prefix>_<run>.bin (per frame the pose and the two
// returned clouds: count, then points) and <prefix>_<run>_map.bin (the local map after the last frame):
//   plain    the feature disabled
//   tiny     enabled with max_ray 1e-3: nothing is in range
//   on       enabled with the given configuration; a copy of the object made after frame 3 goes on beside it (copy_map)
//   manual   the same sequence issued frame by frame through the C-ABI: pre-steps, register, render, sweep, update
//   prior    Config::update_map = false over the map `plain` saved: frames 4 .. 7, the removal is skipped
// and on stdout "<run> <k> <in range> <removed> <voxels touched> <voxels erased>" per frame of the runs with a view.
// Second mode, for tools/bench_view.py: `view_facade_test timed <drive> <view config> <on|off>` runs the drive once and prints the wall
// time of every RegisterFrame call ("frame <k> ms <t>"; the clock around the call alone).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kinematic_icp/pipeline/KinematicICP.hpp"

using kinematic_icp::pipeline::KinematicICP;
using Cloud = std::vector<Eigen::Vector3d>;

static std::vector<double> read_doubles(FILE *f, size_t n) {
    std::vector<double> v(n);
    if (n && fread(v.data(), sizeof(double), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}
static Cloud to_points(const std::vector<double> &v) {
    Cloud p(v.size() / 3);
    if (!p.empty()) std::memcpy(p.front().data(), v.data(), v.size() * sizeof(double));
    return p;
}
static void write_bytes(FILE *f, const void *v, size_t bytes) {
    if (bytes && fwrite(v, 1, bytes, f) != bytes) {
        fprintf(stderr, "cannot write\n");
        exit(2);
    }
}
static FILE *open_out(const std::string &path) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
    return f;
}
static void write_cloud(FILE *f, const Cloud &cloud) {
    const double n = static_cast<double>(cloud.size());
    write_bytes(f, &n, sizeof n);
    if (!cloud.empty()) write_bytes(f, cloud.front().data(), cloud.size() * 3 * sizeof(double));
}
static void write_map(const std::string &path, const KinematicICP &icp) {
    FILE *f = open_out(path);
    write_cloud(f, icp.LocalMap());
    fclose(f);
}
struct Frame {
    Cloud points;
    std::vector<double> stamps;
    Sophus::SE3d delta;
};
static void record(FILE *out, const KinematicICP &icp, const Cloud &frame, const Cloud &source) {
    double p[7];
    kicp_bridge::to_params(icp.pose(), p);
    write_bytes(out, p, sizeof p);
    write_cloud(out, frame), write_cloud(out, source);
}
static void step(KinematicICP &icp, const Frame &fr, const Sophus::SE3d &ext, FILE *out, const char *run, size_t k) {
    const auto [frame, source] = icp.RegisterFrame(fr.points, fr.stamps, ext, fr.delta);
    if (out) record(out, icp, frame, source);
    const auto &s = icp.LastRemoval();
    if (run) printf("%s %zu %llu %llu %llu %llu\n", run, k, s[0], s[1], s[2], s[3]);
}

// RegisterFrame's sequence spelled out through the C-ABI, the removal between the registration and the map update
class Manual : public KinematicICP {
public:
    using KinematicICP::KinematicICP;
    void Step(const Frame &fr, const Sophus::SE3d &ext, kicp_view *view, FILE *out, size_t k) {
        const Sophus::SE3d rel_lidar_se3 = ext.inverse() * fr.delta * ext;
        double rel_lidar[7], ext_qt[7], pose[7];
        kicp_bridge::to_params(rel_lidar_se3, rel_lidar);
        kicp_bridge::to_params(ext, ext_qt);
        Cloud frame(fr.points.size()), source;
        size_t counts[3] = {0, 0, 0};
        kicp_bridge::check(kicp_pre_frame(pre_, kicp_bridge::xyz(fr.points), fr.points.size(), fr.stamps.data(), fr.stamps.size(), rel_lidar, ext_qt, config_.max_range,
                                          config_.min_range, config_.deskew ? 1 : 0, config_.voxel_size * 0.5, config_.voxel_size * 1.5,
                                          frame.empty() ? nullptr : frame.front().data(), frame.size(), counts),
                           "kicp_pre_frame");
        const double tau = correspondence_threshold_.ComputeThreshold();
        const auto new_pose = registration_.ComputeRobotMotionDevice(kicp_pre_device_ptr(pre_, 2, nullptr), counts[2], local_map_, last_pose_, fr.delta, tau);
        correspondence_threshold_.UpdateOdometryError((last_pose_ * fr.delta).inverse() * new_pose);
        kicp_bridge::to_params(new_pose, pose);
        const Eigen::Vector3d sensor = ext.translation();
        unsigned long long s[4] = {0, 0, 0, 0};
        kicp_bridge::check(kicp_view_render_device(view, kicp_pre_device_ptr(pre_, 0, nullptr), counts[0], pose, sensor.data(), nullptr), "kicp_view_render_device");
        kicp_bridge::check(kicp_map_remove_seen_through(local_map_.handle(), view, s), "kicp_map_remove_seen_through");
        kicp_bridge::check(kicp_map_update_pose_device(local_map_.handle(), local_map_.device_, kicp_pre_device_ptr(pre_, 1, nullptr), counts[1], pose),
                           "kicp_map_update_pose_device");
        last_pose_ = new_pose;
        source.resize(counts[2]);
        kicp_bridge::check(kicp_pre_download(pre_, 2, source.empty() ? nullptr : source.front().data(), source.size(), nullptr), "download");
        kicp_bridge::check(kicp_pre_download_finish(pre_, 0, frame.empty() ? nullptr : frame.front().data(), frame.size(), nullptr), "download");
        frame.resize(counts[0]);
        record(out, *this, frame, source);
        printf("manual %zu %llu %llu %llu %llu\n", k, s[0], s[1], s[2], s[3]);
    }
};

int main(int argc, char **argv) {
    const bool timed = argc >= 5 && std::string(argv[1]) == "timed";
    if (argc < 4) return 1;
    FILE *f = fopen(argv[timed ? 2 : 1], "rb"), *g = fopen(argv[timed ? 3 : 2], "rb");
    if (!f || !g) return 1;
    const std::string prefix = argv[timed ? 4 : 3];
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
        const auto vc = read_doubles(g, 6);
        const kicp_bridge::ViewConfig view_config{static_cast<unsigned int>(vc[0]), static_cast<int>(vc[1]), static_cast<unsigned int>(vc[2]), vc[3], vc[4], vc[5]};
        if (timed) {
            KinematicICP icp(cfg);
            if (prefix == "on") icp.EnableSeeThroughRemoval(view_config);
            unsigned long long removed = 0;
            for (size_t k = 0; k < frames.size(); ++k) {
                const auto t0 = std::chrono::steady_clock::now();
                const auto result = icp.RegisterFrame(frames[k].points, frames[k].stamps, ext, frames[k].delta);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                printf("frame %zu ms %.4f in %zu\n", k, ms, std::get<0>(result).size());
                removed += icp.LastRemoval()[1];
            }
            printf("points_removed %llu\n", removed);
            return 0;
        }
        {
            KinematicICP plain(cfg);
            FILE *out = open_out(prefix + "_plain.bin");
            for (size_t k = 0; k < frames.size(); ++k) step(plain, frames[k], ext, out, nullptr, k);
            fclose(out);
            write_map(prefix + "_plain_map.bin", plain);
            plain.SaveMap(prefix + "_plain_map.pcd");
            printf("plain_has_no_view %d\n", plain.View() ? 0 : 1);
        }
        {
            KinematicICP tiny(cfg);
            kicp_bridge::ViewConfig c = view_config;
            c.max_ray = 1e-3;
            tiny.EnableSeeThroughRemoval(c);
            FILE *out = open_out(prefix + "_tiny.bin");
            for (size_t k = 0; k < frames.size(); ++k) step(tiny, frames[k], ext, out, "tiny", k);
            fclose(out);
            write_map(prefix + "_tiny_map.bin", tiny);
        }
        {
            KinematicICP mapper(cfg);
            mapper.EnableSeeThroughRemoval(view_config);
            FILE *out = open_out(prefix + "_on.bin");
            for (size_t k = 0; k < 4; ++k) step(mapper, frames[k], ext, out, "on", k);
            KinematicICP copy(mapper);  // a deep copy: the map, and a view of its own
            printf("copy_has_its_own_view %d\n", copy.View() && copy.View() != mapper.View() ? 1 : 0);
            for (size_t k = 4; k < frames.size(); ++k) step(mapper, frames[k], ext, out, "on", k), step(copy, frames[k], ext, nullptr, "copy", k);
            fclose(out);
            write_map(prefix + "_on_map.bin", mapper);
            write_map(prefix + "_copy_map.bin", copy);
            unsigned long long rendered = 0;
            kicp_bridge::check(kicp_view_info(mapper.View().get(), nullptr, nullptr, &rendered), "kicp_view_info");
            printf("frames_rendered %llu\n", rendered);
            mapper.DisableSeeThroughRemoval();
            printf("disabled %d %llu\n", mapper.View() ? 0 : 1, mapper.LastRemoval()[1]);
        }
        {
            Manual manual(cfg);
            auto view = kicp_bridge::make_view(view_config);
            FILE *out = open_out(prefix + "_manual.bin");
            for (size_t k = 0; k < frames.size(); ++k) manual.Step(frames[k], ext, view.get(), out, k);
            fclose(out);
            write_map(prefix + "_manual_map.bin", manual);
        }
        {
            kinematic_icp::pipeline::Config prior_cfg = cfg;
            prior_cfg.update_map = false;
            KinematicICP prior(prior_cfg);
            prior.LoadMap(prefix + "_plain_map.pcd");
            write_map(prefix + "_prior_before_map.bin", prior);
            prior.EnableSeeThroughRemoval(view_config);
            Sophus::SE3d at;  // the pose before frame 4: the deltas so far
            for (size_t k = 0; k < 4; ++k) at = at * frames[k].delta;
            prior.SetPose(at);
            FILE *out = open_out(prefix + "_prior.bin");
            for (size_t k = 4; k < frames.size(); ++k) step(prior, frames[k], ext, out, "prior", k);
            fclose(out);
            write_map(prefix + "_prior_map.bin", prior);
            unsigned long long rendered = 0;
            kicp_bridge::check(kicp_view_info(prior.View().get(), nullptr, nullptr, &rendered), "kicp_view_info");
            printf("prior_frames_rendered %llu\n", rendered);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
