// elev_host_test.cpp -- elev_host::integrate and elev_host::classify (kicp_elev_host.hpp), the host restatements of the height columns'
// frame update and classification over the very arithmetic the kernels call, in a program of its own: tests/test_elev_host.py builds it
// plainly and under ASan + UBSan - a shift by 64 in the classification is exactly what UBSan reports - and compares what it writes with
// the numpy restatement (tests/elev_ref.py).
// Input (argv[1]), doubles: cell, origin_x, origin_y, width, height, z_origin, slab, max_ray, frames, params; then `params` pairs (S, H);
// then per frame pose[7], sensor[3], n and the n points.  Optional argv[3]: width * height columns (uint64) the layer starts from.
// Output: one line "frame <used> <skipped> <outside_grid> <outside_column> <new_bits> <new_cells>" per frame and one line
// "counts <unknown> <traversable> <body> <step_only>" per pair on stdout; in argv[2] the columns after the last frame (uint64 per cell)
// and behind them, per pair, the classes (int8 per cell) and the ground bytes (uint8 per cell).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_elev_host.hpp"

static std::vector<double> read_doubles(FILE *f, size_t n) {
    std::vector<double> v(n);
    if (n && fread(v.data(), sizeof(double), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    const auto h = read_doubles(f, 10);
    const double inf = INFINITY;
    const kicp::ElevGeom g{kicp::GridGeom{h[0], h[1], h[2], -inf, inf, static_cast<uint32_t>(h[3]), static_cast<uint32_t>(h[4]), static_cast<int32_t>(std::ceil(h[7] / h[0]))},
                           h[5], h[6]};
    if (g.plane.reach > kicp::kGridMaxReach) return 1;
    const size_t cells = static_cast<size_t>(g.plane.width) * g.plane.height, frames = static_cast<size_t>(h[8]), n_params = static_cast<size_t>(h[9]);
    const auto params = read_doubles(f, 2 * n_params);
    std::vector<uint64_t> columns(cells, 0);
    if (argc > 3) {
        FILE *start = fopen(argv[3], "rb");
        if (!start || fread(columns.data(), sizeof(uint64_t), cells, start) != cells) return 1;
        fclose(start);
    }
    for (size_t k = 0; k < frames; ++k) {
        const auto head = read_doubles(f, 11);
        const auto xyz = read_doubles(f, 3 * static_cast<size_t>(head[10]));
        unsigned long long stats[6];
        kicp::elev_host::integrate(g, columns.data(), xyz.data(), xyz.size() / 3, head.data(), head.data() + 7, stats);
        printf("frame %llu %llu %llu %llu %llu %llu\n", stats[0], stats[1], stats[2], stats[3], stats[4], stats[5]);
    }
    fclose(f);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    bool ok = fwrite(columns.data(), sizeof(uint64_t), cells, out) == cells;
    std::vector<int8_t> classes(cells);
    std::vector<uint8_t> ground(cells);
    for (size_t k = 0; k < n_params; ++k) {
        const kicp::ElevParams p{static_cast<uint32_t>(params[2 * k]), static_cast<uint32_t>(params[2 * k + 1])};
        unsigned long long counts[4];
        kicp::elev_host::classify(columns.data(), g.plane.width, g.plane.height, p, kicp::ElevRect{0u, 0u, g.plane.width, g.plane.height}, classes.data(), ground.data(),
                                  counts);
        printf("counts %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3]);
        ok = ok && fwrite(classes.data(), 1, cells, out) == cells && fwrite(ground.data(), 1, cells, out) == cells;
    }
    return (fclose(out) == 0 && ok) ? 0 : 1;
}
