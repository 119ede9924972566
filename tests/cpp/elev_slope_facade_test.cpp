// elev_slope_facade_test.cpp -- the slope limit of the height columns through the drop-in C++ headers:
// KinematicICP::ElevationTraversabilitySlope, ElevationSlopeLimit and kicp_bridge::ElevationSlopeConfig.
// Input: the drive file tests/test_elev_facade.py writes, a file with the eight doubles of the layer's configuration and S, H, L, K,
// min_cells and the limit's tangent behind them, and a prefix for what it writes:
//   <prefix>_columns.bin   the columns of the drive's layer
//   <prefix>_classes.bin   ElevationTraversabilitySlope of the full layer: the classes, then the ground bytes
//   <prefix>_fit.bin       its determinants, three int64 per cell
//   <prefix>_window.bin    the classes of ElevationLastWindow grown by L cells
// and on stdout "limit <rise> <run>", "counts <five words>", "window <x0> <y0> <w> <h>", "refused_without_layer <slope> <limit>",
// "refused_bad_config <n of 4>", "refused_bad_tangent <n of 2>".
#include <cmath>
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
static void write_file(const std::string &path, const void *v, size_t bytes, const void *more = nullptr, size_t more_bytes = 0) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (bytes && fwrite(v, 1, bytes, f) != bytes) || (more_bytes && fwrite(more, 1, more_bytes, f) != more_bytes) || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
}
template <class Call>
static int refuses(Call call) {
    try {
        call();
    } catch (const std::runtime_error &) {
        return 1;
    }
    return 0;
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
        const auto ec = read_doubles(g, 14);
        const kicp_bridge::ElevationConfig layer_config{ec[0], ec[1], ec[2], static_cast<unsigned int>(ec[3]), static_cast<unsigned int>(ec[4]), ec[5], ec[6], ec[7]};
        const kicp_bridge::ElevationTraversabilityConfig classes_config{static_cast<unsigned int>(ec[8]), static_cast<unsigned int>(ec[9])};
        const kicp_bridge::ElevationSlopeConfig fit_config{static_cast<unsigned int>(ec[10]), static_cast<unsigned int>(ec[11]), static_cast<unsigned int>(ec[12]), 0u, 1u};
        KinematicICP mapper(cfg);
        std::vector<int8_t> classes;
        printf("refused_without_layer %d %d\n", refuses([&] { mapper.ElevationTraversabilitySlope(classes_config, fit_config, classes); }),
               refuses([&] { mapper.ElevationSlopeLimit(ec[13]); }));
        mapper.EnableElevation(layer_config);
        for (size_t k = 0; k < static_cast<size_t>(h[0]); ++k) {
            const auto n = read_doubles(f, 1);
            const auto xyz = read_doubles(f, static_cast<size_t>(n[0]) * 3);
            std::vector<Eigen::Vector3d> points(xyz.size() / 3);
            if (!points.empty()) std::memcpy(points.front().data(), xyz.data(), xyz.size() * sizeof(double));
            const auto stamps = read_doubles(f, static_cast<size_t>(n[0]));
            mapper.RegisterFrame(points, stamps, ext, kicp_bridge::from_params(read_doubles(f, 7).data()));
        }
        const kicp_bridge::ElevationSlopeConfig slope = mapper.ElevationSlopeLimit(ec[13], fit_config);
        printf("limit %u %u\n", slope.rise_slabs, slope.run_cells);
        std::vector<unsigned long long> columns(static_cast<size_t>(layer_config.width) * layer_config.height);
        kicp_bridge::check(kicp_elev_columns(mapper.Elevation().get(), columns.data(), columns.size()), "kicp_elev_columns");
        write_file(prefix + "_columns.bin", columns.data(), columns.size() * sizeof(unsigned long long));
        std::vector<uint8_t> ground;
        std::vector<long long> fit;
        std::array<unsigned long long, KICP_ELEV_SLOPE_COUNTS> counts{};
        mapper.ElevationTraversabilitySlope(classes_config, slope, classes, nullptr, &ground, &counts, &fit);
        printf("counts %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4]);
        write_file(prefix + "_classes.bin", classes.data(), classes.size(), ground.data(), ground.size());
        write_file(prefix + "_fit.bin", fit.data(), fit.size() * sizeof(long long));
        const kicp_bridge::GridRect window = mapper.ElevationLastWindow(), grown = window.grown(slope.radius_cells, layer_config.width, layer_config.height);
        printf("window %u %u %u %u\n", window.x0, window.y0, window.w, window.h);
        mapper.ElevationTraversabilitySlope(classes_config, slope, classes, &grown);
        write_file(prefix + "_window.bin", classes.data(), classes.size());
        int bad = 0;
        for (kicp_bridge::ElevationSlopeConfig c : {kicp_bridge::ElevationSlopeConfig{0u, 6u, 12u, 1u, 1u}, kicp_bridge::ElevationSlopeConfig{4u, 64u, 12u, 1u, 1u},
                                                    kicp_bridge::ElevationSlopeConfig{4u, 6u, 2u, 1u, 1u}, kicp_bridge::ElevationSlopeConfig{4u, 6u, 12u, 1u, 0u}})
            bad += refuses([&] { mapper.ElevationTraversabilitySlope(classes_config, c, classes); });
        printf("refused_bad_config %d\n", bad);
        printf("refused_bad_tangent %d\n", refuses([&] { mapper.ElevationSlopeLimit(-1.0); }) + refuses([&] { mapper.ElevationSlopeLimit(std::nan("")); }));
        const kicp_bridge::ElevationSlopeConfig defaults = mapper.ElevationSlopeLimit(ec[13]);
        printf("defaults %u %u %u %u %u\n", defaults.radius_cells, defaults.gate_slabs, defaults.min_cells, defaults.rise_slabs, defaults.run_cells);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
