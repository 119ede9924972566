// elev_slope_host_test.cpp -- elev_host::classify_slope (kicp_elev_host.hpp), the host restatement of the slope limit over the very
// arithmetic the kernels call - the nine sums, the determinants, the 128-bit comparison -, in a program of its own:
// tests/test_elev_slope_host.py builds it plainly and under ASan + UBSan - a window that leaves the layer or a product that
// overflows is exactly what they report - and compares what it writes with the numpy restatement (tests/elev_slope_ref.py).
// Input (argv[1]), doubles: width, height, runs; then per run S, H, L, K, min_cells, rise, run, x0, y0, w, h; then width * height
// columns (uint64).  Output: one line "counts <unknown> <traversable> <body> <step_only> <slope_only>" per run on stdout; in argv[2]
// per run the classes (int8 per cell of the rectangle), the ground bytes (uint8 per cell) and the fit (three int64 per cell).
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
    const auto h = read_doubles(f, 3);
    const uint32_t width = static_cast<uint32_t>(h[0]), height = static_cast<uint32_t>(h[1]);
    const size_t cells = static_cast<size_t>(width) * height, runs = static_cast<size_t>(h[2]);
    const auto params = read_doubles(f, 11 * runs);
    std::vector<uint64_t> columns(cells);
    if (fread(columns.data(), sizeof(uint64_t), cells, f) != cells) return 1;
    fclose(f);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    bool ok = true;
    for (size_t k = 0; k < runs; ++k) {
        const double *v = params.data() + 11 * k;
        const kicp::ElevParams p{static_cast<uint32_t>(v[0]), static_cast<uint32_t>(v[1])};
        const kicp::ElevSlopeParams sp{static_cast<uint32_t>(v[2]), static_cast<uint32_t>(v[3]), static_cast<uint32_t>(v[4]), static_cast<uint32_t>(v[5]),
                                       static_cast<uint32_t>(v[6])};
        const kicp::ElevRect r{static_cast<uint32_t>(v[7]), static_cast<uint32_t>(v[8]), static_cast<uint32_t>(v[9]), static_cast<uint32_t>(v[10])};
        if (sp.radius < 1u || sp.radius > kicp::kElevSlopeMaxRadius || sp.gate > kicp::kElevSlopeMaxGate || r.w < 1u || r.h < 1u || r.x0 + r.w > width || r.y0 + r.h > height) return 1;
        const size_t n = static_cast<size_t>(r.w) * r.h;
        std::vector<int8_t> classes(n);
        std::vector<uint8_t> ground(n);
        std::vector<long long> fit(3 * n);
        unsigned long long counts[5];
        kicp::elev_host::classify_slope(columns.data(), width, height, p, sp, r, classes.data(), ground.data(), fit.data(), counts);
        printf("counts %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4]);
        ok = ok && fwrite(classes.data(), 1, n, out) == n && fwrite(ground.data(), 1, n, out) == n && fwrite(fit.data(), sizeof(long long), 3 * n, out) == 3 * n;
    }
    return (fclose(out) == 0 && ok) ? 0 : 1;
}
