// elev_rough_facade_test.cpp -- the class ROUGH and the fill through the drop-in C++ headers: KinematicICP::ElevationTraversabilityRough,
// ElevationRoughLimit and ElevationIntoGrid in its four forms, kicp_bridge::ElevationRoughConfig and GridFillConfig.
// Input: the drive file tests/test_elev_facade.py writes, a file with the eight doubles of the layer's configuration and behind them
// S, H, L, K, min_cells, the slope limit's tangent, the ROUGH limit's r.m.s. residual in metres, the band z_min, z_max of the pipeline's
// own grid and the fill's min_observations, free_max, occupied_min, and a prefix for what it writes:
//   <prefix>_columns.bin   the columns of the drive's layer
//   <prefix>_source.bin    the counters of the pipeline's own grid
//   <prefix>_classes.bin   ElevationTraversabilityRough of the full layer: the classes, then the ground bytes
//   <prefix>_fit.bin       its five int64 per cell
//   <prefix>_plain.bin, _slope.bin, _rough.bin, _filled.bin   the planner grid's counters after ElevationIntoGrid in its four forms
// and on stdout "limit <num> <den>", "counts <six words>", "fill_counts <seven words>", "forms_equal <n of 4>" - each form against the
// C calls it wraps, on a second grid -, "refused_without_layer <n of 3>", "refused_rough_without_slope <0 | 1>",
// "refused_fill_without_grid <0 | 1>", "refused_bad_config <n of 3>".
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
template <class Error, class Call>
static int refuses(Call call) {
    try {
        call();
    } catch (const Error &) {
        return 1;
    }
    return 0;
}
static std::vector<unsigned short> counters(const kicp_grid *grid, size_t cells) {
    std::vector<unsigned short> v(2 * cells);
    kicp_bridge::check(kicp_grid_counts(grid, v.data(), cells), "kicp_grid_counts");
    return v;
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
        const auto ec = read_doubles(g, 20);
        const kicp_bridge::ElevationConfig layer_config{ec[0], ec[1], ec[2], static_cast<unsigned int>(ec[3]), static_cast<unsigned int>(ec[4]), ec[5], ec[6], ec[7]};
        const kicp_bridge::GridConfig source_config{ec[0], ec[1], ec[2], layer_config.width, layer_config.height, ec[15], ec[16], ec[7]};
        const kicp_bridge::GridConfig planner_config{ec[0], ec[1], ec[2], layer_config.width, layer_config.height, -1.0, 1.0, ec[7]};
        const kicp_bridge::ElevationTraversabilityConfig classes_config{static_cast<unsigned int>(ec[8]), static_cast<unsigned int>(ec[9])};
        const kicp_bridge::ElevationSlopeConfig fit_config{static_cast<unsigned int>(ec[10]), static_cast<unsigned int>(ec[11]), static_cast<unsigned int>(ec[12]), 0u, 1u};
        const kicp_bridge::GridFillConfig fill{static_cast<unsigned int>(ec[17]), static_cast<unsigned int>(ec[18]), static_cast<unsigned int>(ec[19])};
        const size_t cells = static_cast<size_t>(layer_config.width) * layer_config.height;
        const auto planner = kicp_bridge::make_grid(planner_config), direct = kicp_bridge::make_grid(planner_config);
        KinematicICP mapper(cfg);
        std::vector<int8_t> classes;
        const kicp_bridge::ElevationRoughConfig any{0u, 1u};
        printf("refused_without_layer %d\n", refuses<std::runtime_error>([&] { mapper.ElevationTraversabilityRough(classes_config, fit_config, any, classes); }) +
                                                 refuses<std::runtime_error>([&] { mapper.ElevationRoughLimit(ec[14]); }) +
                                                 refuses<std::runtime_error>([&] { mapper.ElevationIntoGrid(planner.get(), classes_config); }));
        {  // a layer, no grid: the fill is refused before anything is written
            KinematicICP bare(cfg);
            bare.EnableElevation(layer_config);
            bare.ElevationIntoGrid(planner.get(), classes_config, &fit_config, &any);
            printf("refused_fill_without_grid %d\n", refuses<std::runtime_error>([&] { bare.ElevationIntoGrid(planner.get(), classes_config, &fit_config, &any, &fill); }));
            printf("refused_rough_without_slope %d\n", refuses<std::invalid_argument>([&] { bare.ElevationIntoGrid(planner.get(), classes_config, nullptr, &any); }));
        }
        mapper.EnableGrid(source_config);
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
        const kicp_bridge::ElevationRoughConfig rough = mapper.ElevationRoughLimit(ec[14]);
        printf("limit %u %u\n", rough.num, rough.den);
        std::vector<unsigned long long> columns(cells);
        kicp_bridge::check(kicp_elev_columns(mapper.Elevation().get(), columns.data(), columns.size()), "kicp_elev_columns");
        write_file(prefix + "_columns.bin", columns.data(), columns.size() * sizeof(unsigned long long));
        const auto source = counters(mapper.Grid().get(), cells);
        write_file(prefix + "_source.bin", source.data(), source.size() * sizeof(unsigned short));
        std::vector<uint8_t> ground;
        std::vector<long long> fit;
        std::array<unsigned long long, KICP_ELEV_ROUGH_COUNTS> counts{};
        mapper.ElevationTraversabilityRough(classes_config, slope, rough, classes, nullptr, &ground, &counts, &fit);
        printf("counts %llu %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4], counts[5]);
        write_file(prefix + "_classes.bin", classes.data(), classes.size(), ground.data(), ground.size());
        write_file(prefix + "_fit.bin", fit.data(), fit.size() * sizeof(long long));
        // the four forms, each against the C calls it wraps
        const kicp_elev *elev = mapper.Elevation().get();
        int equal = 0;
        mapper.ElevationIntoGrid(planner.get(), classes_config);
        kicp_bridge::check(kicp_elev_to_grid(elev, &classes_config, direct.get()), "kicp_elev_to_grid");
        auto got = counters(planner.get(), cells);
        equal += got == counters(direct.get(), cells);
        write_file(prefix + "_plain.bin", got.data(), got.size() * sizeof(unsigned short));
        mapper.ElevationIntoGrid(planner.get(), classes_config, &slope);
        kicp_bridge::check(kicp_elev_to_grid_slope(elev, &classes_config, &slope, direct.get()), "kicp_elev_to_grid_slope");
        got = counters(planner.get(), cells);
        equal += got == counters(direct.get(), cells);
        write_file(prefix + "_slope.bin", got.data(), got.size() * sizeof(unsigned short));
        mapper.ElevationIntoGrid(planner.get(), classes_config, &slope, &rough);
        kicp_bridge::check(kicp_elev_to_grid_rough(elev, &classes_config, &slope, &rough, direct.get()), "kicp_elev_to_grid_rough");
        got = counters(planner.get(), cells);
        equal += got == counters(direct.get(), cells);
        write_file(prefix + "_rough.bin", got.data(), got.size() * sizeof(unsigned short));
        kicp_bridge::GridFillCounts words{}, direct_words{};
        mapper.ElevationIntoGrid(planner.get(), classes_config, &slope, &rough, &fill, &words);
        kicp_bridge::check(kicp_grid_fill_unknown(direct.get(), mapper.Grid().get(), &fill, direct_words.data()), "kicp_grid_fill_unknown");
        got = counters(planner.get(), cells);
        equal += got == counters(direct.get(), cells) && words == direct_words && counters(mapper.Grid().get(), cells) == source;
        write_file(prefix + "_filled.bin", got.data(), got.size() * sizeof(unsigned short));
        printf("fill_counts %llu %llu %llu %llu %llu %llu %llu\n", words[0], words[1], words[2], words[3], words[4], words[5], words[6]);
        printf("forms_equal %d\n", equal);
        int bad = 0;
        for (kicp_bridge::ElevationRoughConfig c : {kicp_bridge::ElevationRoughConfig{65536u, 1u}, kicp_bridge::ElevationRoughConfig{1u, 0u}, kicp_bridge::ElevationRoughConfig{1u, 65536u}})
            bad += refuses<std::runtime_error>([&] { mapper.ElevationTraversabilityRough(classes_config, slope, c, classes); });
        printf("refused_bad_config %d\n", bad);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f), fclose(g);
    return 0;
}
