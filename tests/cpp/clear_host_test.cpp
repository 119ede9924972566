// clear_host_test.cpp -- clear_host::clearance, clear_host::costmap and clear_host::cost_table_nav2 (kicp_clear_host.hpp), the host side of
// the grid's clearance and costmap and the very arithmetic the kernels call, in a program of its own: tests/test_clearance_host.py
// builds it plainly and under ASan + UBSan and compares what it writes with the numpy restatement (tests/clearance_ref.py).
// Input (argv[1]): 14 doubles - width, height, occupied_thresh, unknown_is_obstacle, radius, inflate_unknown, x0, y0, w, h, cell,
// inscribed_radius, cost_scaling_factor, cases - then `cases` times: width * height bytes of readout and radius^2 + 2 bytes of table.
// Output (argv[2]), per case: the clearance of the rectangle as uint16 (w * h), its costmap as uint8 (w * h); then once the Nav2 table
// of (cell, radius, inscribed_radius, cost_scaling_factor) as radius^2 + 2 bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_clear_host.hpp"

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
    const auto h = read_values<double>(f, 14);
    const uint32_t width = static_cast<uint32_t>(h[0]), height = static_cast<uint32_t>(h[1]), radius = static_cast<uint32_t>(h[4]);
    if (radius < 1u || radius > static_cast<uint32_t>(kicp::kClearMaxRadius)) return 1;
    const kicp::ClearParams p{1u, kicp::clear_source_min(h[2]), h[3] != 0.0 ? 1u : 0u, radius};
    const kicp::ClearRect r{static_cast<uint32_t>(h[6]), static_cast<uint32_t>(h[7]), static_cast<uint32_t>(h[8]), static_cast<uint32_t>(h[9])};
    if (r.w < 1u || r.h < 1u || r.x0 + r.w > width || r.y0 + r.h > height) return 1;
    const size_t table_len = static_cast<size_t>(kicp::clear_far(radius)) + 1u;
    for (size_t k = 0; k < static_cast<size_t>(h[13]); ++k) {
        const auto occupancy = read_values<int8_t>(f, static_cast<size_t>(width) * height);
        const auto table = read_values<uint8_t>(f, table_len);
        std::vector<uint16_t> clearance(static_cast<size_t>(r.w) * r.h);
        std::vector<uint8_t> cost(clearance.size());
        kicp::clear_host::clearance(occupancy.data(), width, height, p, r, clearance.data());
        kicp::clear_host::costmap(occupancy.data(), width, height, p, table.data(), h[5] != 0.0 ? 1u : 0u, r, cost.data());
        write_values(out, clearance), write_values(out, cost);
    }
    std::vector<uint8_t> nav2(table_len);
    kicp::clear_host::cost_table_nav2(h[10], radius, h[11], h[12], nav2.data());
    write_values(out, nav2);
    fclose(f);
    return fclose(out) == 0 ? 0 : 1;
}
