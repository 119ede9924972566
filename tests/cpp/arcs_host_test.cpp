// arcs_host_test.cpp -- arcs_host::score, steps, box and best (kicp_arcs_host.hpp), the host side of scoring a fan of arcs and the
// very arithmetic the kernel calls, in a program of its own: tests/test_arcs_host.py builds it plainly and under ASan + UBSan and
// compares what it writes with the restatement (tests/arcs_ref.py).
// Input (argv[1]): 19 doubles - width, height, cell, origin_x, origin_y, n_arcs, n_steps, n_samples, dt, the box x_min, x_max, y_min,
// y_max, spacing, the box's cap in samples, then w_potential, w_cost, w_blocked, min_free_steps - then start[4], the arcs
// (n_arcs x 4), the footprint (n_samples x 2), v and omega (n_arcs each), all doubles, then q (width * height bytes) and the potential
// (width * height x uint32).
// Output (argv[2]): the results (n_arcs x 4 x uint32), arcs_host::steps of (v, omega, dt) (n_arcs x 4 doubles), the box's count
// (uint64) and its first min(count, cap) samples (the buffer holds exactly those, so nothing may be written past it), and
// arcs_host::best over the results (uint64).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_arcs_host.hpp"

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
    const auto h = read_values<double>(f, 19);
    const uint32_t width = static_cast<uint32_t>(h[0]), height = static_cast<uint32_t>(h[1]), n_steps = static_cast<uint32_t>(h[6]), n_samples = static_cast<uint32_t>(h[7]);
    const size_t n_arcs = static_cast<size_t>(h[5]), box_cap = static_cast<size_t>(h[14]);
    if (width < 1u || height < 1u || !(h[2] > 0.0) || n_arcs < 1u || n_arcs > kicp::kArcsMaxK || n_steps < 1u || n_steps > kicp::kArcsMaxT || n_samples < 1u ||
        n_samples > kicp::kArcsMaxP || !(h[9] <= h[10]) || !(h[11] <= h[12]) || !(h[13] > 0.0))
        return 1;
    const auto start = read_values<double>(f, 4), arcs = read_values<double>(f, 4 * n_arcs), footprint = read_values<double>(f, 2 * static_cast<size_t>(n_samples));
    const auto v = read_values<double>(f, n_arcs), omega = read_values<double>(f, n_arcs);
    const auto q = read_values<uint8_t>(f, static_cast<size_t>(width) * height);
    const auto potential = read_values<uint32_t>(f, static_cast<size_t>(width) * height);

    std::vector<uint32_t> results(4 * n_arcs);
    kicp::arcs_host::score(kicp::ArcGeom{h[2], h[3], h[4], width, height}, q.data(), potential.data(), start.data(), arcs.data(), n_arcs, n_steps, footprint.data(), n_samples,
                           results.data());
    write_values(out, results);
    std::vector<double> steps(4 * n_arcs);
    kicp::arcs_host::steps(v.data(), omega.data(), h[8], n_arcs, steps.data());
    write_values(out, steps);
    const double nx = kicp::arcs_host::box_count(h[9], h[10], h[13]), ny = kicp::arcs_host::box_count(h[11], h[12], h[13]);
    if (!(nx * ny <= static_cast<double>(kicp::kArcsMaxP))) return 1;
    const size_t count = static_cast<size_t>(nx) * static_cast<size_t>(ny);
    std::vector<double> box(2 * (count < box_cap ? count : box_cap));
    kicp::arcs_host::box(h[9], h[10], h[11], h[12], static_cast<size_t>(nx), static_cast<size_t>(ny), box.data(), box.size() / 2);
    write_values(out, std::vector<unsigned long long>{count});
    write_values(out, box);
    const size_t best = kicp::arcs_host::best(results.data(), n_arcs, static_cast<uint32_t>(h[15]), static_cast<uint32_t>(h[16]), static_cast<uint32_t>(h[17]), n_steps,
                                              static_cast<uint32_t>(h[18]));
    write_values(out, std::vector<unsigned long long>{best});
    fclose(f);
    return fclose(out) == 0 ? 0 : 1;
}
