// front_host_test.cpp -- front_host::frontiers (kicp_front_host.hpp), the host side of the exploration frontiers and the very
// arithmetic the kernels call, in a program of its own: tests/test_frontier_host.py builds it plainly and under ASan + UBSan and
// compares what it writes with the restatement (tests/frontier_ref.py).
// Input (argv[1]): 5 x uint32 - width, height, min_size, has_potential, cap_rows - then occupied_thresh (a double), width * height
// bytes of readout and, with has_potential, width * height x uint32.
// Output (argv[2]): the number of frontiers that passed the filter (uint64), the stored rows (min(cap_rows, that number) x 10 x uint64;
// the buffer holds exactly cap_rows rows, so nothing may be written past it) and the label plane (width * height x uint32).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_front_host.hpp"

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
    const auto h = read_values<uint32_t>(f, 5);
    const uint32_t width = h[0], height = h[1];
    const double thresh = read_values<double>(f, 1)[0];
    if (width < 1u || height < 1u || h[2] < 1u || !(0.0 <= thresh && thresh <= 1.0)) return 1;
    const size_t cells = static_cast<size_t>(width) * height, cap = h[4];
    const auto occupancy = read_values<int8_t>(f, cells);
    const auto potential = read_values<uint32_t>(f, h[3] ? cells : 0u);
    std::vector<unsigned long long> rows(cap * kicp::kFrontWords);
    std::vector<uint32_t> labels(cells);
    const size_t n = kicp::front_host::frontiers(occupancy.data(), width, height, kicp::clear_source_min(thresh), h[2], h[3] ? potential.data() : nullptr, rows.data(), cap,
                                                 labels.data());
    rows.resize((n < cap ? n : cap) * kicp::kFrontWords);
    write_values(out, std::vector<unsigned long long>{n}), write_values(out, rows), write_values(out, labels);
    fclose(f);
    return fclose(out) == 0 ? 0 : 1;
}
