// view_host_test.cpp -- view_host::render / classify / sweep (kicp_view_host.hpp), the host restatement of the depth view over the very
// geometry and verdict the kernels call, and HostMap::RemovePointsIf, in a program of its own: tests/test_view_host.py builds it plainly
// and under ASan + UBSan and compares what it prints and writes with the numpy restatement (tests/view_ref.py).
// Input (argv[1]), doubles: res, window, min_rays, max_ray, margin, margin_per_metre, voxel_size, max_distance, max_points_per_voxel,
// n_map, n_frame, n_query; pose[7], sensor[3]; then the map's points (inserted in this order), the frame's, the queries'.
// Output: "render <used> <skipped>", "sweep <in range> <removed> <voxels touched> <voxels erased>", "map <points> <voxels>",
// "check <violations after the sweep> <after inserting the map's points once more>" on stdout; in argv[2] the image (6 res^2 floats),
// the queries' verdicts (bytes) and the swept map's cloud (doubles).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_view_host.hpp"

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
    const auto h = read_doubles(f, 22);
    const kicp::ViewGeom g{static_cast<uint32_t>(h[0]), static_cast<int32_t>(h[1]), static_cast<uint32_t>(h[2]), h[3], h[4], h[5]};
    if (const char *why = kicp::view_config_error(g.res, g.window, g.min_rays, g.max_ray, g.margin, g.margin_per_metre)) {
        fprintf(stderr, "%s\n", why);
        return 1;
    }
    const size_t n_map = static_cast<size_t>(h[9]), n_frame = static_cast<size_t>(h[10]), n_query = static_cast<size_t>(h[11]);
    const auto map_xyz = read_doubles(f, 3 * n_map), frame = read_doubles(f, 3 * n_frame), query = read_doubles(f, 3 * n_query);
    fclose(f);
    kicp::HostMap map(h[6], h[7], static_cast<uint32_t>(h[8]));
    if (!map.AddPoints(map_xyz.data(), n_map)) return 1;

    std::vector<uint32_t> depth(6 * static_cast<size_t>(g.res) * g.res);
    unsigned long long rs[2], ss[4];
    const kicp::ViewFrame vf = kicp::view_host::render(g, depth.data(), frame.data(), n_frame, h.data() + 12, h.data() + 19, rs);
    printf("render %llu %llu\n", rs[0], rs[1]);
    std::vector<uint8_t> verdicts(n_query);
    kicp::view_host::classify(g, vf, depth.data(), query.data(), n_query, verdicts.data());
    kicp::view_host::sweep(g, vf, depth.data(), map, ss);
    printf("sweep %llu %llu %llu %llu\n", ss[0], ss[1], ss[2], ss[3]);
    printf("map %zu %zu\n", map.num_points(), map.num_voxels());
    std::vector<double> cloud(3 * map.num_points());
    map.Pointcloud(cloud.data(), map.num_points());
    const size_t bad = map.CheckInvariants();
    if (!map.AddPoints(map_xyz.data(), n_map)) return 1;  // freed buckets are taken again, shortened ones filled up
    printf("check %zu %zu\n", bad, map.CheckInvariants());

    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    // (an empty vector's data() may be null, which fwrite must not be given: a map swept empty, or no queries)
    const bool ok = fwrite(depth.data(), 4, depth.size(), out) == depth.size() && (n_query == 0 || fwrite(verdicts.data(), 1, n_query, out) == n_query) &&
                    (cloud.empty() || fwrite(cloud.data(), 8, cloud.size(), out) == cloud.size());
    return (fclose(out) == 0 && ok) ? 0 : 1;
}
