// HostMap (kicp_host_map.hpp) under random insertions and removals, in a program of its own: CheckInvariants() - which holds every
// point's second mirror word to the float bits of its quantised z, and every slot behind a bucket's count to the empty pattern - stays 0,
// and buckets that were freed and handed out again read empty behind their new count although they held more points before.
// Removals go both ways a map loses points: whole voxels far from a location (RemovePointsFarFromLocation: the bucket returns to the
// free list) and single points (RemovePointsIf: the bucket is compacted, its tail marked empty).  max_points_per_voxel 20 (one trip of
// the pass kernel), 21 and 40 (two trips).
// Built by tests/test_mirror_point.py with `hipcc --cuda-host-only`.
#include <cstdio>
#include <random>
#include <vector>

#include "kicp_host_map.hpp"

using namespace kicp;

// every bucket of an occupied voxel, read the way the kernels read it: `count` points, then empty slots up to the stride
static long wrong_slots(const HostMap &map) {
    long bad = 0;
    for (const Slot &e : map.table()) {
        if (e.val == kEmptyVal) continue;
        const uint32_t count = val_count(e.val, map.count_bits()), bucket = val_bucket(e.val, map.count_bits());
        if (!count) continue;
        const MirrorPoint *row = &map.pool16()[static_cast<size_t>(bucket) * map.cap16()];
        for (uint32_t k = 0; k < map.cap16(); ++k) {
            if (mirror_is_point(row[k]) != (k < count)) ++bad;
            if (k >= count && (mirror_z(row[k]) != 4294901760.0f || row[k].y != mirror_empty().y)) ++bad;
            if (k < count && mirror_z(row[k]) != static_cast<float>(mirror_qz(row[k]))) ++bad;
        }
    }
    return bad;
}

int main() {
    long bad = 0;
    for (uint32_t cap : {20u, 21u, 40u}) {
        std::mt19937_64 rng(77 + cap);
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        HostMap map(1.0, 6.0, cap);
        size_t reused = 0, shrunk = 0;
        for (int round = 0; round < 60; ++round) {
            // a burst of points over a few voxels around a moving centre: dense enough to fill buckets (the spacing rule rejects some)
            const double cx = 3.0 * (round % 7), cy = 2.0 * (round % 5);
            std::vector<double> pts;
            const int n = 200 + static_cast<int>(rng() % 1800);
            for (int i = 0; i < n; ++i) {
                pts.push_back(cx + 4.0 * u01(rng) - 2.0), pts.push_back(cy + 4.0 * u01(rng) - 2.0), pts.push_back(2.0 * u01(rng) - 1.0);
                if (i % 97 == 0) pts[pts.size() - 1] = std::floor(pts[pts.size() - 1]);  // on a voxel's near z face: mirror z = 0
                if (i % 89 == 0) pts[pts.size() - 1] = std::floor(pts[pts.size() - 1]) + 1.0 - 1.0 / 1048576.0;  // just inside the far face: 65 535
            }
            const size_t free_before = map.free_list().size();
            if (!map.AddPoints(pts.data(), pts.size() / 3)) ++bad, std::printf("cap %u round %d: AddPoints refused\n", cap, round);
            if (map.free_list().size() < free_before) reused += free_before - map.free_list().size();
            if (map.CheckInvariants() != 0) ++bad, std::printf("cap %u round %d: %zu violations after AddPoints\n", cap, round, map.CheckInvariants());
            bad += wrong_slots(map);
            if (round % 3 == 1) {  // whole voxels go: their buckets return to the free list with their old contents
                const double origin[3] = {cx, cy, 0.0};
                map.RemovePointsFarFromLocation(origin);
            } else {  // single points go: a third of them, by position
                unsigned long long out[3];
                map.RemovePointsIf([&](const double *p) { return (static_cast<long long>(std::floor(p[0] * 64.0) + std::floor(p[1] * 64.0)) + round) % 3 == 0; }, out);
                shrunk += out[1];
            }
            if (map.CheckInvariants() != 0) ++bad, std::printf("cap %u round %d: %zu violations after a removal\n", cap, round, map.CheckInvariants());
            bad += wrong_slots(map);
        }
        // the scenario did what it was built for: buckets were freed and re-used, buckets lost single points, full buckets exist
        size_t full = 0;
        for (const Slot &e : map.table())
            if (e.val != kEmptyVal && val_count(e.val, map.count_bits()) == cap) ++full;
        std::printf("cap %u: %zu points in %zu voxels, %zu buckets re-used, %zu shortened, %zu full at the end\n", cap, map.num_points(), map.num_voxels(), reused, shrunk, full);
        if (reused < 20 || shrunk < 20) ++bad, std::printf("cap %u: the scenario did not re-use or shorten buckets\n", cap);
    }
    std::printf("mirror host map: %ld bad\n", bad);
    return bad ? 1 : 0;
}
