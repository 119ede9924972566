// gain_facade_test.cpp -- the information gain through the drop-in C++ headers: KinematicICP::GridGain on a grid whose counters the
// test sets, against the C entry it wraps, and the exceptions without a grid and for a viewpoint outside it.
// Input: a file with the grid's width and height, the range in cells and the number of viewpoints (4 x uint32), the grid's counters
// (width * height x 2 x uint16) and the viewpoints (cell indices, uint32), and a prefix for what it writes:
//   <prefix>_rows.bin   GridGain's result: per viewpoint the four words of kicp_grid_gain, taken back out of the named fields (uint32)
// It prints same_as_the_c_entry 1 when the rows equal what kicp_grid_gain itself returns for the same arguments.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "kinematic_icp/pipeline/KinematicICP.hpp"

using kinematic_icp::pipeline::KinematicICP;

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
static void write_file(const std::string &path, const std::vector<T> &v) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
}
template <class F>
static bool refused(F &&call, const char *needle) {
    try {
        call();
    } catch (const std::runtime_error &e) {
        return std::string(e.what()).find(needle) != std::string::npos;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    const std::string prefix = argv[2];
    try {
        const auto head = read_values<uint32_t>(f, 4);
        const unsigned int W = head[0], H = head[1];
        const auto counts = read_values<unsigned short>(f, 2 * static_cast<size_t>(W) * H);
        const std::vector<unsigned int> cells = read_values<unsigned int>(f, head[3]);
        const kicp_bridge::GainConfig config{1u, 0.65, head[2]};
        KinematicICP icp{kinematic_icp::pipeline::Config{}};
        std::vector<kicp_bridge::Gain> gains;
        printf("refused_without_grid %d\n", refused([&] { icp.GridGain(cells, config, gains); }, "EnableGrid") ? 1 : 0);
        icp.EnableGrid(kicp_bridge::GridConfig{0.05, 0.0, 0.0, W, H, 0.0, 1.0, 1.0});
        kicp_bridge::check(kicp_grid_set_counts(icp.Grid().get(), counts.data(), counts.size() / 2), "kicp_grid_set_counts");
        printf("refused_outside_the_grid %d\n", refused([&] { icp.GridGain({0u, W * H}, config, gains); }, "viewpoint 1 ") ? 1 : 0);
        icp.GridGain({}, config, gains);
        printf("no_viewpoints %zu\n", gains.size());
        icp.GridGain(cells, config, gains);
        std::vector<uint32_t> rows;
        for (const auto &g : gains)
            for (uint32_t v : {g.seen, g.blocked, g.left, g.view_class}) rows.push_back(v);
        std::vector<unsigned int> c_rows(cells.size() * KICP_GAIN_WORDS);
        kicp_bridge::check(kicp_grid_gain(icp.Grid().get(), &config, cells.data(), cells.size(), c_rows.data(), c_rows.size()), "kicp_grid_gain");
        printf("same_as_the_c_entry %d\n", std::vector<uint32_t>(c_rows.begin(), c_rows.end()) == rows ? 1 : 0);
        write_file(prefix + "_rows.bin", rows);
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    fclose(f);
    return 0;
}
