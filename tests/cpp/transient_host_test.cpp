// transient_host_test.cpp -- transient_host::transients (kicp_transient_host.hpp), the host side of the transient obstacles and the very
// arithmetic the kernels call, in a program of its own: tests/test_transient_host.py builds it plainly and under ASan + UBSan and
// compares what it writes with the restatement (tests/transient_ref.py).
// Input (argv[1]): 8 x uint32 - width, height, reach, min_observations, free_max, min_points, min_size, cap_rows - then a uint64, the
// number of points n, 15 doubles - cell, origin_x, origin_y, z_min, z_max, the pose's seven and the sensor's three - the counters
// (width * height x 2 x uint16) and the points (n x 3 doubles).
// Output (argv[2]): the number of transients that passed the filter (uint64), the four statistics (uint64), the stored rows
// (min(cap_rows, that number) x 10 x uint64; the buffer holds exactly cap_rows rows, so nothing may be written past it), the label
// plane (width * height x uint32) and the plane (width * height bytes).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_transient_host.hpp"

template <class T>
static std::vector<T> read_values(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}
template <class T>
static void write_values(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "cannot write\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!f || !out) return 1;
    const auto h = read_values<uint32_t>(f, 8);
    const size_t n = read_values<unsigned long long>(f, 1)[0];
    const auto d = read_values<double>(f, 15);
    const uint32_t width = h[0], height = h[1];
    if (width < 1u || height < 1u || h[2] > 4095u || h[3] < 1u || h[4] > 100u || h[5] < 1u || h[6] < 1u) return 1;
    const kicp::GridGeom g{d[0], d[1], d[2], d[3], d[4], width, height, static_cast<int32_t>(h[2])};
    const kicp::TransientParams p{h[3], h[4], h[5], h[6]};
    const size_t cells = static_cast<size_t>(width) * height, cap = h[7];
    const auto counts = read_values<uint16_t>(f, 2 * cells);
    const auto points = read_values<double>(f, 3 * n);
    std::vector<unsigned long long> rows(cap * kicp::kTransientWords), stats(4);
    std::vector<uint32_t> labels(cells);
    std::vector<uint8_t> plane(cells);
    const size_t found = kicp::transient_host::transients(g, counts.data(), points.data(), n, d.data() + 5, d.data() + 12, p, rows.data(), cap, labels.data(), plane.data(),
                                                         stats.data());
    rows.resize((found < cap ? found : cap) * kicp::kTransientWords);
    write_values(out, std::vector<unsigned long long>{found}), write_values(out, stats), write_values(out, rows), write_values(out, labels), write_values(out, plane);
    fclose(f);
    return fclose(out) == 0 ? 0 : 1;
}
