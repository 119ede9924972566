// grid_host_test.cpp -- grid_host::integrate (kicp_grid_host.hpp), the host restatement of the occupancy grid's frame update and the
// very geometry the kernels call, in a program of its own: tests/test_grid_host.py builds it plainly and under ASan + UBSan and
// compares what it prints with the numpy restatement (tests/grid_ref.py).
// Input (argv[1]), doubles: cell, origin_x, origin_y, width, height, z_min, z_max, max_ray, frames; then per frame pose[7], sensor[3],
// n and the n points.  Output: one line "frame <used> <skipped> <hit> <miss>" per frame on stdout, the counters after the last frame as
// uint16 (cells x 2) in argv[2], and the readout at min_observations 1 as int8 behind them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_grid_host.hpp"

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
    const auto h = read_doubles(f, 9);
    kicp::GridGeom g{h[0], h[1], h[2], h[5], h[6], static_cast<uint32_t>(h[3]), static_cast<uint32_t>(h[4]), static_cast<int32_t>(std::ceil(h[7] / h[0]))};
    if (g.reach > kicp::kGridMaxReach) return 1;
    const size_t cells = static_cast<size_t>(g.width) * g.height;
    std::vector<uint16_t> counts(2 * cells, 0);
    const size_t frames = static_cast<size_t>(h[8]);
    for (size_t k = 0; k < frames; ++k) {
        const auto head = read_doubles(f, 11);
        const auto xyz = read_doubles(f, 3 * static_cast<size_t>(head[10]));
        unsigned long long stats[4];
        kicp::grid_host::integrate(g, counts.data(), xyz.data(), xyz.size() / 3, head.data(), head.data() + 7, stats);
        printf("frame %llu %llu %llu %llu\n", stats[0], stats[1], stats[2], stats[3]);
    }
    fclose(f);
    std::vector<int8_t> occupancy(cells);
    for (size_t i = 0; i < cells; ++i) occupancy[i] = kicp::grid_readout(counts[2 * i], counts[2 * i + 1], 1u);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    const bool ok = fwrite(counts.data(), sizeof(uint16_t), counts.size(), out) == counts.size() && fwrite(occupancy.data(), 1, cells, out) == cells;
    return (fclose(out) == 0 && ok) ? 0 : 1;
}
