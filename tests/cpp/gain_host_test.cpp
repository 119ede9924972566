// gain_host_test.cpp -- gain_host::gain (kicp_gain_host.hpp), the host side of the information gain and the very arithmetic the
// kernels call, in a program of its own: tests/test_gain_host.py builds it plainly and under ASan + UBSan and compares what it writes
// with the restatement (tests/gain_ref.py).
// Input (argv[1]): 4 x uint32 - width, height, range_cells, n_views - then occupied_thresh (a double), width * height bytes of readout
// and n_views x uint32 viewpoints (cell indices).
// Output (argv[2]): n_views x 4 x uint32, the rows - the buffer holds exactly that, so nothing may be written past it - and then
// 8 R x 2 x int32, the perimeter offsets in the order of the ray index.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_gain_host.hpp"

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
    const auto h = read_values<uint32_t>(f, 4);
    const uint32_t width = h[0], height = h[1], R = h[2];
    const size_t n = h[3];
    const double thresh = read_values<double>(f, 1)[0];
    if (width < 1u || height < 1u || R < 1u || R > kicp::kGainMaxRange || !(0.0 <= thresh && thresh <= 1.0)) return 1;
    const size_t cells = static_cast<size_t>(width) * height;
    const auto occupancy = read_values<int8_t>(f, cells);
    const auto views = read_values<uint32_t>(f, n);
    for (uint32_t v : views)
        if (v >= cells) return 1;
    std::vector<uint32_t> rows(n * kicp::kGainWords);
    kicp::gain_host::gain(occupancy.data(), width, height, kicp::clear_source_min(thresh), R, views.data(), n, rows.data());
    std::vector<int32_t> perimeter(2u * kicp::gain_rays(R));
    for (uint32_t i = 0; i < kicp::gain_rays(R); ++i) kicp::gain_ray(R, i, perimeter[2u * i], perimeter[2u * i + 1u]);
    write_values(out, rows), write_values(out, perimeter);
    fclose(f);
    return fclose(out) == 0 ? 0 : 1;
}
