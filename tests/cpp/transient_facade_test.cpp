// transient_facade_test.cpp -- the transient obstacles through the drop-in C++ headers: KinematicICP::EnableTransients, DisableTransients,
// Transients, TransientPlane, and the switch carried by a copy.
// Input: the drive file tests/test_transient_facade.py writes (the format of tests/test_facade.py's pipeline mode), a file with the
// eight doubles of the grid's configuration and min_observations, free_max, min_points, min_size behind them, and a prefix for what it
// writes:
//   <prefix>_off.bin, <prefix>_on.bin   per frame the pose and the two returned clouds (count, then points), without / with transients
//   <prefix>_rows.bin                   per frame the number of Transients() (uint64) and their ten words, taken back out of the
//                                       named fields (uint64)
//   <prefix>_planes.bin                 per frame TransientPlane() after it (width * height bytes)
//   <prefix>_costmap_<k>.bin, <prefix>_occupancy_<k>.bin   GridCostmap (radius 3, Nav2's table) and GridOccupancy after frame k
//   <prefix>_counts.bin                 the counters after the drive
// On stdout "same_as_the_c_entry <k> 1" per frame - Transients() against kicp_grid_transients on the second pipeline's grid, whose
// counters are the first one's before that frame - and one line per property named below.
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
template <class T>
static void write_file(const std::string &path, const std::vector<T> &v) {
    FILE *f = open_out(path);
    write_bytes(f, v.data(), v.size() * sizeof(T));
    fclose(f);
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
// one frame through the pipeline -> the frame it returned
static std::vector<Eigen::Vector3d> step(KinematicICP &icp, const Frame &fr, const Sophus::SE3d &ext, FILE *out) {
    auto [frame, source] = icp.RegisterFrame(fr.points, fr.stamps, ext, fr.delta);
    double p[7];
    kicp_bridge::to_params(icp.pose(), p);
    write_bytes(out, p, sizeof p);
    write_cloud(out, frame), write_cloud(out, source);
    return frame;
}
static std::vector<unsigned long long> rows_of(const std::vector<kicp_bridge::Transient> &transients) {
    std::vector<unsigned long long> rows;
    for (const auto &t : transients) {
        for (unsigned long long v : {static_cast<unsigned long long>(t.label), static_cast<unsigned long long>(t.size), static_cast<unsigned long long>(t.returns),
                                     static_cast<unsigned long long>(t.sum_nx), static_cast<unsigned long long>(t.sum_ny), static_cast<unsigned long long>(t.min_x),
                                     static_cast<unsigned long long>(t.max_x), static_cast<unsigned long long>(t.min_y), static_cast<unsigned long long>(t.max_y),
                                     (static_cast<unsigned long long>(t.nearest_d2) << 32) | t.nearest_cell})
            rows.push_back(v);
        if (!(t.centroid_x() >= t.min_x && t.centroid_x() <= t.max_x && t.centroid_y() >= t.min_y && t.centroid_y() <= t.max_y)) exit(4);
    }
    return rows;
}
template <class Call>
static bool refused(Call call, const char *needle) {
    try {
        call();
    } catch (const std::runtime_error &e) {
        return std::string(e.what()).find(needle) != std::string::npos;
    }
    return false;
}

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
        const kicp_bridge::TransientConfig config{static_cast<unsigned int>(gc[8]), static_cast<unsigned int>(gc[9]), static_cast<unsigned int>(gc[10]),
                                                  static_cast<unsigned int>(gc[11])};
        const size_t cells = static_cast<size_t>(grid_config.width) * grid_config.height;
        const kicp_bridge::GridClearanceConfig clearance{config.min_observations, 0.65, 0, 3};
        std::vector<uint8_t> table(3 * 3 + 2);
        kicp_bridge::check(kicp_grid_cost_table_nav2(grid_config.cell, 3, 0.15, 3.0, table.data(), table.size()), "kicp_grid_cost_table_nav2");

        KinematicICP plain(cfg), mapper(cfg);
        printf("refused_without_grid %d\n", refused([&] { mapper.EnableTransients(config); }, "EnableGrid") && !mapper.TransientsEnabled() ? 1 : 0);
        plain.EnableGrid(grid_config), mapper.EnableGrid(grid_config);
        printf("off_by_default %d\n", !mapper.TransientsEnabled() && !kicp_grid_uses_transients(mapper.Grid().get()) && mapper.Transients().empty() ? 1 : 0);
        printf("refused_bad_config %d\n", refused([&] { mapper.EnableTransients(kicp_bridge::TransientConfig{1u, 101u, 1u, 1u}); }, "free_max") && !mapper.TransientsEnabled() ? 1 : 0);
        mapper.EnableTransients(config);
        printf("enabled %d\n", mapper.TransientsEnabled() && kicp_grid_uses_transients(mapper.Grid().get()) ? 1 : 0);

        FILE *off = open_out(prefix + "_off.bin"), *on = open_out(prefix + "_on.bin"), *rows_out = open_out(prefix + "_rows.bin"), *planes = open_out(prefix + "_planes.bin");
        std::vector<uint8_t> plane, costmap;
        std::vector<int8_t> occupancy;
        for (size_t k = 0; k < frames.size(); ++k) {
            const auto returned = step(mapper, frames[k], ext, on);
            const auto rows = rows_of(mapper.Transients());
            const unsigned long long count = mapper.Transients().size();
            write_bytes(rows_out, &count, sizeof count), write_bytes(rows_out, rows.data(), rows.size() * sizeof(unsigned long long));
            mapper.TransientPlane(plane);
            write_bytes(planes, plane.data(), plane.size());
            // the C entry on the other pipeline's grid, which has not seen this frame yet
            double pose[7];
            kicp_bridge::to_params(mapper.pose(), pose);
            const double sensor[3] = {ext.translation().x(), ext.translation().y(), ext.translation().z()};
            std::vector<unsigned long long> c_rows(rows.size() + KICP_TRANSIENT_WORDS);
            size_t n = 0;
            kicp_bridge::check(kicp_grid_transients(plain.Grid().get(), kicp_bridge::xyz(returned), returned.size(), pose, sensor, &config, c_rows.data(),
                                                    c_rows.size() / KICP_TRANSIENT_WORDS, &n, nullptr, 0, nullptr),
                               "kicp_grid_transients");
            c_rows.resize(n * KICP_TRANSIENT_WORDS);
            std::vector<uint8_t> c_plane(cells);
            kicp_bridge::check(kicp_grid_transient_plane(plain.Grid().get(), c_plane.data(), c_plane.size()), "kicp_grid_transient_plane");
            printf("same_as_the_c_entry %zu %d\n", k, c_rows == rows && c_plane == plane ? 1 : 0);
            step(plain, frames[k], ext, off);
            mapper.GridCostmap(costmap, clearance, table, false);
            mapper.GridOccupancy(occupancy, config.min_observations);
            write_file(prefix + "_costmap_" + std::to_string(k) + ".bin", costmap), write_file(prefix + "_occupancy_" + std::to_string(k) + ".bin", occupancy);
            if (k == 2) {  // a copy carries the switch and the configuration and starts with an empty plane
                KinematicICP copy(mapper);
                std::vector<uint8_t> copied;
                copy.TransientPlane(copied);
                bool empty = true;
                for (uint8_t b : copied) empty = empty && b == 0;
                printf("copy_carries_the_switch %d\n", copy.TransientsEnabled() && kicp_grid_uses_transients(copy.Grid().get()) && copy.Grid() != mapper.Grid() && empty &&
                                                               copy.Transients().empty() ? 1 : 0);
                KinematicICP moved(std::move(copy));
                printf("moved_carries_the_switch %d\n", moved.TransientsEnabled() && kicp_grid_uses_transients(moved.Grid().get()) ? 1 : 0);
            }
        }
        fclose(off), fclose(on), fclose(rows_out), fclose(planes);
        std::vector<unsigned short> counts(2 * cells), plain_counts(2 * cells);
        kicp_bridge::check(kicp_grid_counts(mapper.Grid().get(), counts.data(), cells), "kicp_grid_counts");
        kicp_bridge::check(kicp_grid_counts(plain.Grid().get(), plain_counts.data(), cells), "kicp_grid_counts");
        printf("counters_agree %d\n", counts == plain_counts ? 1 : 0);
        write_file(prefix + "_counts.bin", counts);
        mapper.DisableTransients();
        mapper.TransientPlane(plane);
        bool empty = true;
        for (uint8_t b : plane) empty = empty && b == 0;
        printf("disabled %d\n", !mapper.TransientsEnabled() && !kicp_grid_uses_transients(mapper.Grid().get()) && empty && mapper.Transients().empty() ? 1 : 0);
        mapper.EnableTransients(config, false);
        printf("enabled_without_sources %d\n", mapper.TransientsEnabled() && !kicp_grid_uses_transients(mapper.Grid().get()) ? 1 : 0);
        mapper.EnableGrid(grid_config);  // a new grid starts without transients
        printf("new_grid_starts_off %d\n", mapper.TransientsEnabled() ? 0 : 1);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
