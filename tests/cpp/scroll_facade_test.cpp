// scroll_facade_test.cpp -- following through the drop-in C++ headers: KinematicICP::EnableGridFollow, DisableGridFollow, LastGridScroll,
// EnableElevationFollow, DisableElevationFollow, LastElevationScroll, and the setting carried by a copy and a move.
// Input: the drive file tests/test_scroll_facade.py writes (the format of tests/test_facade.py's pipeline mode), a file with the eight
// doubles of the grid's configuration and margin_cells, step_cells, z_origin, slab behind them, and a prefix for what it writes:
//   <prefix>_off.bin, <prefix>_on.bin   per frame the pose and the two returned clouds (count, then points), without / with following
//   <prefix>_scrolls.bin                per frame LastGridScroll() and LastElevationScroll(), four int32
//   <prefix>_origins.bin                per frame origin_x, origin_y of the grid and of the layer as their info entries report them
//   <prefix>_counts.bin                 per frame the grid's counters after it
//   <prefix>_columns.bin                per frame the layer's columns after it
// On stdout one line per property named below.
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
struct Frame {
    std::vector<Eigen::Vector3d> points;
    std::vector<double> stamps;
    Sophus::SE3d delta;
};
static void step(KinematicICP &icp, const Frame &fr, const Sophus::SE3d &ext, FILE *out) {
    auto [frame, source] = icp.RegisterFrame(fr.points, fr.stamps, ext, fr.delta);
    double p[7];
    kicp_bridge::to_params(icp.pose(), p);
    write_bytes(out, p, sizeof p);
    write_cloud(out, frame), write_cloud(out, source);
}
template <class Call>
static bool refused(Call call) {
    try {
        call();
    } catch (const std::invalid_argument &) {
        return true;
    } catch (const std::exception &) {
        return false;
    }
    return false;
}
template <class Call>
static bool throws(Call call) {
    try {
        call();
    } catch (const std::exception &) {
        return true;
    }
    return false;
}
static bool zero(const std::array<int, 2> &d) { return d[0] == 0 && d[1] == 0; }

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
        std::vector<Frame> frames(static_cast<size_t>(h[0]));
        for (Frame &fr : frames) {
            const auto n = read_doubles(f, 1);
            fr.points = to_points(read_doubles(f, static_cast<size_t>(n[0]) * 3));
            fr.stamps = read_doubles(f, static_cast<size_t>(n[0]));
            fr.delta = kicp_bridge::from_params(read_doubles(f, 7).data());
        }
        const auto gc = read_doubles(g, 12);
        const kicp_bridge::GridConfig grid_config{gc[0], gc[1], gc[2], static_cast<unsigned int>(gc[3]), static_cast<unsigned int>(gc[4]), gc[5], gc[6], gc[7]};
        const unsigned int margin = static_cast<unsigned int>(gc[8]), stride = static_cast<unsigned int>(gc[9]);
        const kicp_bridge::ElevationConfig elev_config{gc[0], gc[1], gc[2], grid_config.width, grid_config.height, gc[10], gc[11], gc[7]};
        const size_t cells = static_cast<size_t>(grid_config.width) * grid_config.height;

        KinematicICP plain(cfg), follower(cfg);
        printf("refused_without_grid %d\n", throws([&] { follower.EnableGridFollow(margin, stride); }) && throws([&] { follower.EnableElevationFollow(margin, stride); }) ? 1 : 0);
        plain.EnableGrid(grid_config), plain.EnableElevation(elev_config);
        follower.EnableGrid(grid_config), follower.EnableElevation(elev_config);
        printf("off_by_default %d\n", !follower.GridFollowEnabled() && !follower.ElevationFollowEnabled() && zero(follower.LastGridScroll()) && zero(follower.LastElevationScroll()) ? 1 : 0);
        const unsigned int w = grid_config.width;
        printf("refused_bad_pair %d\n", refused([&] { follower.EnableGridFollow(0u, stride); }) && refused([&] { follower.EnableGridFollow(margin, 0u); }) &&
                                                refused([&] { follower.EnableGridFollow(w / 2u, 1u); }) && refused([&] { follower.EnableElevationFollow(0u, stride); }) &&
                                                refused([&] { follower.EnableElevationFollow(margin, w); }) && !follower.GridFollowEnabled() && !follower.ElevationFollowEnabled() ? 1 : 0);
        follower.EnableGridFollow(margin, stride), follower.EnableElevationFollow(margin, stride);
        printf("enabled %d\n", follower.GridFollowEnabled() && follower.ElevationFollowEnabled() ? 1 : 0);

        FILE *off = open_out(prefix + "_off.bin"), *on = open_out(prefix + "_on.bin"), *scrolls = open_out(prefix + "_scrolls.bin"), *origins = open_out(prefix + "_origins.bin");
        FILE *counts_out = open_out(prefix + "_counts.bin"), *columns_out = open_out(prefix + "_columns.bin");
        std::vector<unsigned short> counts(2 * cells);
        std::vector<unsigned long long> columns(cells);
        bool plain_never_scrolls = true;
        for (size_t k = 0; k < frames.size(); ++k) {
            step(plain, frames[k], ext, off), step(follower, frames[k], ext, on);
            plain_never_scrolls = plain_never_scrolls && zero(plain.LastGridScroll()) && zero(plain.LastElevationScroll());
            const int32_t d[4] = {follower.LastGridScroll()[0], follower.LastGridScroll()[1], follower.LastElevationScroll()[0], follower.LastElevationScroll()[1]};
            write_bytes(scrolls, d, sizeof d);
            kicp_grid_config gi{};
            kicp_elev_config ei{};
            kicp_bridge::check(kicp_grid_info(follower.Grid().get(), &gi, nullptr, nullptr), "kicp_grid_info");
            kicp_bridge::check(kicp_elev_info(follower.Elevation().get(), &ei, nullptr, nullptr), "kicp_elev_info");
            const double o[4] = {gi.origin_x, gi.origin_y, ei.origin_x, ei.origin_y};
            write_bytes(origins, o, sizeof o);
            kicp_bridge::check(kicp_grid_counts(follower.Grid().get(), counts.data(), cells), "kicp_grid_counts");
            kicp_bridge::check(kicp_elev_columns(follower.Elevation().get(), columns.data(), cells), "kicp_elev_columns");
            write_bytes(counts_out, counts.data(), counts.size() * sizeof(unsigned short));
            write_bytes(columns_out, columns.data(), columns.size() * sizeof(unsigned long long));
            if (k == 2) {  // a copy and a move carry the setting; the copy's handles are its own
                KinematicICP copy(follower);
                const bool carried = copy.GridFollowEnabled() && copy.ElevationFollowEnabled() && copy.Grid() != follower.Grid() && copy.LastGridScroll() == follower.LastGridScroll();
                std::vector<unsigned short> copied(2 * cells);
                kicp_bridge::check(kicp_grid_counts(copy.Grid().get(), copied.data(), cells), "kicp_grid_counts");
                kicp_grid_config ci{};
                kicp_bridge::check(kicp_grid_info(copy.Grid().get(), &ci, nullptr, nullptr), "kicp_grid_info");
                printf("copy_carries_the_setting %d\n", carried && copied == counts && std::memcmp(&ci.origin_x, &gi.origin_x, sizeof(double)) == 0 &&
                                                                std::memcmp(&ci.origin_y, &gi.origin_y, sizeof(double)) == 0 ? 1 : 0);
                KinematicICP moved(std::move(copy));
                KinematicICP assigned(cfg);
                assigned = moved;
                printf("moved_carries_the_setting %d\n", moved.GridFollowEnabled() && moved.ElevationFollowEnabled() && assigned.GridFollowEnabled() && assigned.ElevationFollowEnabled() ? 1 : 0);
            }
        }
        fclose(off), fclose(on), fclose(scrolls), fclose(origins), fclose(counts_out), fclose(columns_out);
        printf("plain_never_scrolls %d\n", plain_never_scrolls ? 1 : 0);
        follower.DisableGridFollow(), follower.DisableElevationFollow();
        printf("disabled %d\n", !follower.GridFollowEnabled() && !follower.ElevationFollowEnabled() && zero(follower.LastGridScroll()) && zero(follower.LastElevationScroll()) ? 1 : 0);
        follower.EnableGridFollow(margin, stride), follower.EnableElevationFollow(margin, stride);
        follower.EnableGrid(grid_config), follower.EnableElevation(elev_config);  // a new grid and a new layer start without following
        printf("new_handles_start_off %d\n", !follower.GridFollowEnabled() && !follower.ElevationFollowEnabled() ? 1 : 0);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
