// grid_facade_test.cpp -- the occupancy grid through the drop-in C++ headers: KinematicICP::EnableGrid, Grid, GridOccupancy, SaveGrid and
// the deep copy of the grid with the object.
// Input: the drive file tests/test_grid_facade.py writes (the format of tests/test_facade.py's pipeline mode), a file with the eight
// doubles of the grid's configuration, and a prefix for what it writes:
//   <prefix>_plain.bin, <prefix>_grid.bin   per frame the pose, the two returned clouds (count, then points), without / with a grid
//   <prefix>_counts.bin, <prefix>_copy_counts.bin   the counters of the drive's grid and of the grid of a copy made after frame 3
//   <prefix>_occupancy.bin                   GridOccupancy at min_observations 2
//   <prefix>_map.pgm, <prefix>_map.yaml      SaveGrid
// Second mode, for tools/bench_grid.py: `grid_facade_test timed <drive> <grid config> <on|off>` runs the drive once, with or without
// a grid, and prints the wall time of every RegisterFrame call ("frame <k> ms <t>"; the clock around the call alone).
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
static void write_counts(const std::string &path, const kicp_grid *grid) {
    kicp_grid_config c{};
    kicp_bridge::check(kicp_grid_info(grid, &c, nullptr, nullptr), "kicp_grid_info");
    std::vector<unsigned short> counts(2 * static_cast<size_t>(c.width) * c.height);
    kicp_bridge::check(kicp_grid_counts(grid, counts.data(), counts.size() / 2), "kicp_grid_counts");
    FILE *f = open_out(path);
    write_bytes(f, counts.data(), counts.size() * sizeof(unsigned short));
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
        const auto gc = read_doubles(g, 8);
        const kicp_bridge::GridConfig grid_config{gc[0], gc[1], gc[2], static_cast<unsigned int>(gc[3]), static_cast<unsigned int>(gc[4]), gc[5], gc[6], gc[7]};
        if (timed) {
            KinematicICP icp(cfg);
            if (prefix == "on") icp.EnableGrid(grid_config);
            for (size_t k = 0; k < frames.size(); ++k) {
                const auto t0 = std::chrono::steady_clock::now();
                const auto result = icp.RegisterFrame(frames[k].points, frames[k].stamps, ext, frames[k].delta);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                printf("frame %zu ms %.4f in %zu\n", k, ms, std::get<0>(result).size());
            }
            unsigned long long integrated = 0;
            if (icp.Grid()) kicp_bridge::check(kicp_grid_info(icp.Grid().get(), nullptr, nullptr, &integrated), "kicp_grid_info");
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
                plain.GridOccupancy(data);
            } catch (const std::runtime_error &) {
                refused = true;
            }
            printf("refused_without_grid %d %d\n", refused ? 1 : 0, plain.Grid() ? 1 : 0);
        }
        KinematicICP mapper(cfg);
        mapper.EnableGrid(grid_config);
        FILE *out = open_out(prefix + "_grid.bin");
        for (size_t k = 0; k < 3; ++k) step(mapper, frames[k], ext, out);
        KinematicICP copy(mapper);  // a deep copy: the map, and the grid
        printf("copy_has_its_own_grid %d\n", copy.Grid() && copy.Grid() != mapper.Grid() ? 1 : 0);
        for (size_t k = 3; k < frames.size(); ++k) step(mapper, frames[k], ext, out), step(copy, frames[k], ext, nullptr);
        fclose(out);
        unsigned long long integrated = 0;
        kicp_bridge::check(kicp_grid_info(mapper.Grid().get(), nullptr, nullptr, &integrated), "kicp_grid_info");
        printf("frames_integrated %llu\n", integrated);
        write_counts(prefix + "_counts.bin", mapper.Grid().get());
        write_counts(prefix + "_copy_counts.bin", copy.Grid().get());
        std::vector<int8_t> occupancy;
        mapper.GridOccupancy(occupancy, 2);
        FILE *occ = open_out(prefix + "_occupancy.bin");
        write_bytes(occ, occupancy.data(), occupancy.size());
        fclose(occ);
        mapper.SaveGrid(prefix + "_map", 2);
        mapper.DisableGrid();
        printf("disabled %d\n", mapper.Grid() ? 0 : 1);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
