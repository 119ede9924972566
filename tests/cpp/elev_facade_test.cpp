// elev_facade_test.cpp -- the height columns through the drop-in C++ headers: KinematicICP::EnableElevation, Elevation,
// ElevationTraversability, ElevationLastWindow, LastElevationStats and the deep copy of the layer with the object.
// Input: the drive file tests/test_elev_facade.py writes (the format of tests/test_facade.py's pipeline mode), a file with the eight
// doubles of the layer's configuration and S, H behind them, and a prefix for what it writes:
//   <prefix>_plain.bin, <prefix>_elev.bin    per frame the pose, the two returned clouds (count, then points), without / with a layer
//   <prefix>_columns.bin, <prefix>_copy_columns.bin   the columns of the drive's layer and of the layer of a copy made after frame 3
//   <prefix>_classes.bin                      ElevationTraversability of the full layer: the classes, then the ground bytes
//   <prefix>_window.bin                       the same for ElevationLastWindow grown by one cell: the classes alone
// and on stdout one line "stats <k> <six words>" per frame, "window <x0> <y0> <w> <h>" and "counts <four words>".
// Second mode, for tools/bench_elev.py: `elev_facade_test timed <drive> <layer config> <on|off>` runs the drive once, with or without
// a layer, and prints the wall time of every RegisterFrame call ("frame <k> ms <t>"; the clock around the call alone).
#include <chrono>
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
        const auto ec = read_doubles(g, 10);
        const kicp_bridge::ElevationConfig layer_config{ec[0], ec[1], ec[2], static_cast<unsigned int>(ec[3]), static_cast<unsigned int>(ec[4]), ec[5], ec[6], ec[7]};
        const kicp_bridge::ElevationTraversabilityConfig classes_config{static_cast<unsigned int>(ec[8]), static_cast<unsigned int>(ec[9])};
        if (timed) {
            KinematicICP icp(cfg);
            if (prefix == "on") icp.EnableElevation(layer_config);
            for (size_t k = 0; k < frames.size(); ++k) {
                const auto t0 = std::chrono::steady_clock::now();
                const auto result = icp.RegisterFrame(frames[k].points, frames[k].stamps, ext, frames[k].delta);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                printf("frame %zu ms %.4f in %zu\n", k, ms, std::get<0>(result).size());
            }
            unsigned long long integrated = 0;
            if (icp.Elevation()) kicp_bridge::check(kicp_elev_info(icp.Elevation().get(), nullptr, nullptr, &integrated), "kicp_elev_info");
            printf("frames_integrated %llu\n", integrated);
            return 0;
        }
        {
            KinematicICP plain(cfg);
            FILE *out = open_out(prefix + "_plain.bin");
            for (const Frame &fr : frames) step(plain, fr, ext, out);
            fclose(out);
            bool refused = false;
            std::vector<int8_t> data;
            try {
                plain.ElevationTraversability(classes_config, data);
            } catch (const std::runtime_error &) {
                refused = true;
            }
            printf("refused_without_layer %d %d\n", refused ? 1 : 0, plain.Elevation() ? 1 : 0);
        }
        KinematicICP mapper(cfg);
        mapper.EnableElevation(layer_config);
        FILE *out = open_out(prefix + "_elev.bin");
        auto stepped = [&](size_t k) {
            step(mapper, frames[k], ext, out);
            const auto &s = mapper.LastElevationStats();
            printf("stats %zu %llu %llu %llu %llu %llu %llu\n", k, s[0], s[1], s[2], s[3], s[4], s[5]);
        };
        for (size_t k = 0; k < 3; ++k) stepped(k);
        KinematicICP copy(mapper);  // a deep copy: the map, and the layer
        printf("copy_has_its_own_layer %d\n", copy.Elevation() && copy.Elevation() != mapper.Elevation() ? 1 : 0);
        for (size_t k = 3; k < frames.size(); ++k) stepped(k), step(copy, frames[k], ext, nullptr);
        fclose(out);
        unsigned long long integrated = 0;
        kicp_bridge::check(kicp_elev_info(mapper.Elevation().get(), nullptr, nullptr, &integrated), "kicp_elev_info");
        printf("frames_integrated %llu\n", integrated);
        write_columns(prefix + "_columns.bin", mapper.Elevation().get());
        write_columns(prefix + "_copy_columns.bin", copy.Elevation().get());
        std::vector<int8_t> classes;
        std::vector<uint8_t> ground;
        std::array<unsigned long long, 4> counts{};
        mapper.ElevationTraversability(classes_config, classes, nullptr, &ground, &counts);
        printf("counts %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3]);
        FILE *cls = open_out(prefix + "_classes.bin");
        write_bytes(cls, classes.data(), classes.size()), write_bytes(cls, ground.data(), ground.size());
        fclose(cls);
        const kicp_bridge::GridRect window = mapper.ElevationLastWindow(), grown = window.grown(1, layer_config.width, layer_config.height);
        printf("window %u %u %u %u\n", window.x0, window.y0, window.w, window.h);
        mapper.ElevationTraversability(classes_config, classes, &grown);
        FILE *win = open_out(prefix + "_window.bin");
        write_bytes(win, classes.data(), classes.size());
        fclose(win);
        mapper.DisableElevation();
        printf("disabled %d\n", mapper.Elevation() ? 0 : 1);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
