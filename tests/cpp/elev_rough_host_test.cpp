// elev_rough_host_test.cpp -- elev_host::classify_rough (kicp_elev_host.hpp) and grid_host::fill_unknown (kicp_grid_host.hpp), the host
// restatements of the class ROUGH and of the fill over the very arithmetic the kernels call - the ten sums, the determinants, the
// residual in 64 bits, the 128-bit comparison; the readout and the classes of two cells -, in a program of its own:
// tests/test_elev_rough_host.py and tests/test_grid_fill_host.py build it plainly and under ASan + UBSan - a window that leaves the
// layer or a product that overflows is exactly what they report - and compare what it writes with the numpy restatement
// (tests/elev_rough_ref.py).
// "rough" <in> <out>.  Input, doubles: width, height, runs; then per run S, H, L, K, min_cells, rise, run, num, den, x0, y0, w, h; then
//   width * height columns (uint64).  Output: one line "counts" and six words per run on stdout; in <out> per run the classes (int8
//   per cell of the rectangle), the ground bytes (uint8 per cell) and the fit (five int64 per cell).
// "fill" <in> <out>.  Input, doubles: cells, min_observations, free_max, occupied_min; then the destination's and the source's
//   counters (uint16, cells x 2 each).  Output: one line "counts" and seven words on stdout; in <out> the destination's counters.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static int run_rough(FILE *f, FILE *out) {
    const auto h = read_doubles(f, 3);
    const uint32_t width = static_cast<uint32_t>(h[0]), height = static_cast<uint32_t>(h[1]);
    const size_t cells = static_cast<size_t>(width) * height, runs = static_cast<size_t>(h[2]);
    const auto params = read_doubles(f, 13 * runs);
    std::vector<uint64_t> columns(cells);
    if (fread(columns.data(), sizeof(uint64_t), cells, f) != cells) return 1;
    bool ok = true;
    for (size_t k = 0; k < runs; ++k) {
        const double *v = params.data() + 13 * k;
        const kicp::ElevParams p{static_cast<uint32_t>(v[0]), static_cast<uint32_t>(v[1])};
        const kicp::ElevSlopeParams sp{static_cast<uint32_t>(v[2]), static_cast<uint32_t>(v[3]), static_cast<uint32_t>(v[4]), static_cast<uint32_t>(v[5]),
                                       static_cast<uint32_t>(v[6])};
        const kicp::ElevRoughParams rp{static_cast<uint32_t>(v[7]), static_cast<uint32_t>(v[8])};
        const kicp::ElevRect r{static_cast<uint32_t>(v[9]), static_cast<uint32_t>(v[10]), static_cast<uint32_t>(v[11]), static_cast<uint32_t>(v[12])};
        if (sp.radius < 1u || sp.radius > kicp::kElevSlopeMaxRadius || sp.gate > kicp::kElevSlopeMaxGate || rp.den < 1u || r.w < 1u || r.h < 1u || r.x0 + r.w > width ||
            r.y0 + r.h > height)
            return 1;
        const size_t n = static_cast<size_t>(r.w) * r.h;
        std::vector<int8_t> classes(n);
        std::vector<uint8_t> ground(n);
        std::vector<long long> fit(5 * n);
        unsigned long long counts[6];
        kicp::elev_host::classify_rough(columns.data(), width, height, p, sp, rp, r, classes.data(), ground.data(), fit.data(), counts);
        printf("counts %llu %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4], counts[5]);
        ok = ok && fwrite(classes.data(), 1, n, out) == n && fwrite(ground.data(), 1, n, out) == n && fwrite(fit.data(), sizeof(long long), 5 * n, out) == 5 * n;
    }
    return ok ? 0 : 1;
}

static int run_fill(FILE *f, FILE *out) {
    const auto h = read_doubles(f, 4);
    const size_t cells = static_cast<size_t>(h[0]);
    const kicp::GridFillParams p{static_cast<uint32_t>(h[1]), static_cast<uint32_t>(h[2]), static_cast<uint32_t>(h[3])};
    if (p.min_observations < 1u || p.free_max > 100u || !(p.free_max < p.occupied_min && p.occupied_min <= 101u)) return 1;
    std::vector<uint16_t> dst(2 * cells), src(2 * cells);
    if (cells && (fread(dst.data(), sizeof(uint16_t), 2 * cells, f) != 2 * cells || fread(src.data(), sizeof(uint16_t), 2 * cells, f) != 2 * cells)) return 1;
    unsigned long long counts[7];
    kicp::grid_host::fill_unknown(dst.data(), src.data(), cells, p, counts);
    printf("counts %llu %llu %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4], counts[5], counts[6]);
    return fwrite(dst.data(), sizeof(uint16_t), 2 * cells, out) == 2 * cells ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc < 4) return 1;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 1;
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 1;
    const int rc = !strcmp(argv[1], "rough") ? run_rough(f, out) : !strcmp(argv[1], "fill") ? run_fill(f, out) : 1;
    fclose(f);
    return (fclose(out) == 0 && rc == 0) ? 0 : 1;
}
