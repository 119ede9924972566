// elev_carve_facade_test.cpp -- the height columns' carve through the drop-in C++ headers: KinematicICP::EnableElevationCarving,
// DisableElevationCarving, ElevationCarving, LastElevationCarveStats, and the setting carried by copy, move and swap.
// Input: the drive file tests/test_elev_carve_facade.py writes (the format of tests/test_facade.py's pipeline mode), a file with the
// eight doubles of the layer's configuration and G, W, keep_ground behind them, and a prefix for what it writes:
//   <prefix>_off.bin, <prefix>_on.bin        per frame the pose and the two returned clouds (count, then points), carving off / on
//   <prefix>_off_columns.bin, <prefix>_on_columns.bin, <prefix>_copy_columns.bin
//                                            the columns after the drive: carving off, on, and of a copy made after frame 3
// and on stdout "off <k> <six words>" and "on <k> <nine words>" per frame and one line per property named below.
// Second mode, for tools/bench_elev.py: `elev_carve_facade_test timed <drive> <layer config> <none|off|on>` runs the drive once - without
// a layer, with a layer, with a layer that carves - and prints the wall time of every RegisterFrame call ("frame <k> ms <t>").
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
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
static void write_cloud(FILE *f, const std::vector<Eigen::Vector3d> &cloud) {
    const double n = static_cast<double>(cloud.size());
    write_bytes(f, &n, sizeof n);
    if (!cloud.empty()) write_bytes(f, cloud.front().data(), cloud.size() * 3 * sizeof(double));
}
static void write_columns(const std::string &path, const kicp_elev *elev) {
    kicp_elev_config c{};
    kicp_bridge::check(kicp_elev_info(elev, &c, nullptr, nullptr), "kicp_elev_info");
    std::vector<unsigned long long> columns(static_cast<size_t>(c.width) * c.height);
    kicp_bridge::check(kicp_elev_columns(elev, columns.data(), columns.size()), "kicp_elev_columns");
    FILE *f = open_out(path);
    write_bytes(f, columns.data(), columns.size() * sizeof(unsigned long long));
    fclose(f);
}
struct Frame {
    std::vector<Eigen::Vector3d> points;
    std::vector<double> stamps;
    Sophus::SE3d delta;
};
static void step(KinematicICP &icp, const Frame &fr, const Sophus::SE3d &ext, FILE *out) {
    const auto [frame, source] = icp.RegisterFrame(fr.points, fr.stamps, ext, fr.delta);
    if (!out) return;
    double p[7];
    kicp_bridge::to_params(icp.pose(), p);
    write_bytes(out, p, sizeof p);
    write_cloud(out, frame), write_cloud(out, source);
}
template <class Error, class Call>
static bool throws(Call call) {
    try {
        call();
    } catch (const Error &) {
        return true;
    }
    return false;
}

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
        const auto ec = read_doubles(g, 11);
        const kicp_bridge::ElevationConfig layer_config{ec[0], ec[1], ec[2], static_cast<unsigned int>(ec[3]), static_cast<unsigned int>(ec[4]), ec[5], ec[6], ec[7]};
        const kicp_bridge::ElevationCarveConfig carve_config{static_cast<unsigned int>(ec[8]), static_cast<unsigned int>(ec[9]), static_cast<unsigned int>(ec[10])};
        if (timed) {
            KinematicICP icp(cfg);
            if (prefix != "none") icp.EnableElevation(layer_config);
            if (prefix == "on") icp.EnableElevationCarving(carve_config);
            for (size_t k = 0; k < frames.size(); ++k) {
                const auto t0 = std::chrono::steady_clock::now();
                const auto result = icp.RegisterFrame(frames[k].points, frames[k].stamps, ext, frames[k].delta);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                printf("frame %zu ms %.4f in %zu\n", k, ms, std::get<0>(result).size());
            }
            printf("bits_cleared %llu\n", icp.LastElevationCarveStats()[7]);
            return 0;
        }
        {
            KinematicICP plain(cfg);
            printf("refused_without_layer %d\n", throws<std::runtime_error>([&] { plain.EnableElevationCarving(carve_config); }) && !plain.ElevationCarving() ? 1 : 0);
            plain.EnableElevation(layer_config);
            printf("off_by_default %d\n", plain.ElevationCarving() ? 0 : 1);
            const bool bad_w = throws<std::invalid_argument>([&] { plain.EnableElevationCarving(kicp_bridge::ElevationCarveConfig{0u, 65u, 1u}); });
            const bool bad_keep = throws<std::invalid_argument>([&] { plain.EnableElevationCarving(kicp_bridge::ElevationCarveConfig{0u, 1u, 2u}); });
            printf("refused_bad_config %d\n", bad_w && bad_keep && !plain.ElevationCarving() ? 1 : 0);
            FILE *out = open_out(prefix + "_off.bin");
            for (size_t k = 0; k < frames.size(); ++k) {
                step(plain, frames[k], ext, out);
                const auto &s = plain.LastElevationStats();
                printf("off %zu %llu %llu %llu %llu %llu %llu\n", k, s[0], s[1], s[2], s[3], s[4], s[5]);
            }
            fclose(out);
            const auto &c = plain.LastElevationCarveStats();
            printf("off_carve_stats_stay_zero %d\n", c == kicp_bridge::ElevationCarveStats{} ? 1 : 0);
            write_columns(prefix + "_off_columns.bin", plain.Elevation().get());
        }
        KinematicICP mapper(cfg);
        mapper.EnableElevation(layer_config);
        mapper.EnableElevationCarving(carve_config);
        FILE *out = open_out(prefix + "_on.bin");
        bool six_agree = true;
        auto stepped = [&](size_t k) {
            step(mapper, frames[k], ext, out);
            const auto &s = mapper.LastElevationCarveStats();
            printf("on %zu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", k, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8]);
            six_agree = six_agree && std::equal(s.begin(), s.begin() + 6, mapper.LastElevationStats().begin());
        };
        for (size_t k = 0; k < 3; ++k) stepped(k);
        KinematicICP copy(mapper);  // a deep copy: the map, the layer, and the setting
        printf("copy_carves %d\n", copy.ElevationCarving() && copy.Elevation() != mapper.Elevation() && copy.LastElevationCarveStats() == mapper.LastElevationCarveStats() ? 1 : 0);
        KinematicICP moved(std::move(copy));  // ... moved on, and assigned back
        printf("moved_carves %d\n", moved.ElevationCarving() ? 1 : 0);
        KinematicICP assigned(cfg);
        assigned = std::move(moved);
        printf("assigned_carves %d\n", assigned.ElevationCarving() ? 1 : 0);
        for (size_t k = 3; k < frames.size(); ++k) stepped(k), step(assigned, frames[k], ext, nullptr);
        fclose(out);
        printf("six_words_agree %d\n", six_agree ? 1 : 0);
        printf("copy_stats_agree %d\n", assigned.LastElevationCarveStats() == mapper.LastElevationCarveStats() ? 1 : 0);
        write_columns(prefix + "_on_columns.bin", mapper.Elevation().get());
        write_columns(prefix + "_copy_columns.bin", assigned.Elevation().get());
        mapper.DisableElevationCarving();
        printf("disabled %d\n", !mapper.ElevationCarving() && mapper.Elevation() && mapper.LastElevationCarveStats() == kicp_bridge::ElevationCarveStats{} ? 1 : 0);
        mapper.EnableElevationCarving(carve_config);
        mapper.EnableElevation(layer_config);  // a new layer starts with carving off
        printf("new_layer_starts_off %d\n", mapper.ElevationCarving() ? 0 : 1);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
