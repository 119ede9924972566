// elev_carve_host_test.cpp -- elev_host::update (kicp_elev_host.hpp), the host restatement of the height columns' carve and mark over
// the very arithmetic the kernels call, in a program of its own: tests/test_elev_carve_host.py builds it plainly and under ASan + UBSan -
// a shift by 64 in a step's mask or a column index outside the grid is exactly what they report - and compares what it writes with the
// numpy restatement (tests/elev_carve_ref.py).
// Input (argv[1]), doubles: cell, origin_x, origin_y, width, height, z_origin, slab, max_ray, frames; then width * height start columns
// (uint64); then per frame pose[7], sensor[3], G, W, keep_ground, n and the n points.
// Output: one line "frame <the nine words>" per frame on stdout; in argv[2] the columns after every frame (uint64 per cell).
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
    const auto h = read_doubles(f, 9);
    const double inf = INFINITY;
    const kicp::ElevGeom g{kicp::GridGeom{h[0], h[1], h[2], -inf, inf, static_cast<uint32_t>(h[3]), static_cast<uint32_t>(h[4]), static_cast<int32_t>(std::ceil(h[7] / h[0]))},
                           h[5], h[6]};
    if (g.plane.reach > kicp::kGridMaxReach) return 1;
    const size_t cells = static_cast<size_t>(g.plane.width) * g.plane.height, frames = static_cast<size_t>(h[8]);
    std::vector<uint64_t> columns(cells, 0);
    if (fread(columns.data(), sizeof(uint64_t), cells, f) != cells) return 1;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    bool ok = true;
    for (size_t k = 0; k < frames; ++k) {
        const auto head = read_doubles(f, 14);
        const auto xyz = read_doubles(f, 3 * static_cast<size_t>(head[13]));
        const kicp::ElevCarveParams p{static_cast<uint32_t>(head[10]), static_cast<uint32_t>(head[11]), static_cast<uint32_t>(head[12])};
        if (p.widen_slabs > kicp::kElevMaxWiden || p.keep_ground > 1u) return 1;
        unsigned long long stats[9];
        kicp::elev_host::update(g, columns.data(), xyz.data(), xyz.size() / 3, head.data(), head.data() + 7, p, stats);
        printf("frame %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", stats[0], stats[1], stats[2], stats[3], stats[4], stats[5], stats[6], stats[7], stats[8]);
        ok = ok && fwrite(columns.data(), sizeof(uint64_t), cells, out) == cells;
    }
    fclose(f);
    return (fclose(out) == 0 && ok) ? 0 : 1;
}
