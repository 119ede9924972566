// map_asan_main.cpp -- drives the voxel map's host code (kicp_map.hip, kicp_map_update.hip, kicp_map_cloud.hip, kicp_core.hip, compiled
// for the host with -fsanitize=address,undefined: `make -C kinematic_icp_amd/csrc map-asan`) over the malloc-backed HIP stand-in of
// hip_standin.cpp, on the CPU: the paths that allocate, swap and free the mirror's buffers - full and delta upload with pool growth,
// grow_pools with the free list, the one-queue, staged and deferred ends of an update, the hand-over to the host map, both Pointcloud
// entries with an update pending, clone / clear / destroy with an update pending, bulk insertion.  No kernel runs, so the "device"
// state stays what the host uploaded; what is checked is who owns which block, not the map's contents.  argv[1]: points of the first
// host insertion (it decides which delta upload grows the pools).  Exit status 0: no call failed and the sanitizers found nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kicp_internal.hpp"

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        int rc_ = (x);                                                                             \
        std::printf("%-70s -> %d %s\n", #x, rc_, rc_ < 0 ? kicp_last_error() : "");              \
        if (rc_ < 0) ++g_failed;                                                                   \
    } while (0)

static int g_failed = 0;
static std::vector<double> grid(size_t n, double x0, double y0) {  // one point per unit voxel, 128 wide
    std::vector<double> p(3 * n);
    for (size_t i = 0; i < n; ++i) p[3 * i] = x0 + double(i % 128) + 0.5, p[3 * i + 1] = y0 + double(i / 128) + 0.5, p[3 * i + 2] = 0.5;
    return p;
}
// what k_up_publish would have written: the device counters (the stand-in's memory is host memory) and the sequence number
static void publish(kicp_map *m, unsigned error) {
    kicp::DevMapCounters c;
    std::memcpy(&c, m->mirror.d_ctr.get(), sizeof c);
    c.error = error;
    std::memcpy(m->mirror.h_ctr.get(), &c, sizeof c);
    m->mirror.h_ctr.get()[7] = m->mirror.ctr_seq;
}
static void counts(kicp_map *m, const char *what) {
    unsigned long long c[12];
    kicp_map_update_counts(m, c);
    std::printf("  [%s] one_queue %llu staged %llu second %llu rehash %llu growths %llu host %llu deferred %llu | device_updates %llu pending %d host_only %d\n", what, c[0], c[1], c[2],
                c[3], c[4], c[8], c[9], kicp_map_device_updates(m), int(m->pending.active), int(m->host_updates_only));
}

int main(int argc, char **argv) {
    const size_t first = argc > 1 ? std::strtoul(argv[1], nullptr, 10) : 3000;
    const double pose[7] = {0, 0, 0, 1, 0, 0, 0};
    kicp_map *m = nullptr;
    CHECK(kicp_map_create(1.0, 1000.0, 20, &m));
    auto a = grid(first, 0, 0);
    CHECK(kicp_map_add_points(m, a.data(), first));  // host insertion: the table is sized on the host
    CHECK(kicp_map_sync(m, 0));                     // full upload: replace_pools without keeping
    for (int k = 0; k < 5; ++k) {  // delta uploads; one of them has to grow the pools with their contents (replace_pools on a stream)
        auto b = grid(400, 0, 100 + 4 * k);
        CHECK(kicp_map_add_points(m, b.data(), 400));
        const size_t before = m->mirror.d_pool.capacity();
        CHECK(kicp_map_sync(m, 0));
        size_t bytes; int full;
        kicp_map_last_upload(m, &bytes, &full);
        std::printf("  upload %d: full=%d bytes=%zu pool %zu -> %zu doubles\n", k, full, bytes, before, m->mirror.d_pool.capacity());
    }
    auto c = grid(4000, 0, 200);                    // "device" points are host memory here
    CHECK(kicp_map_update_pose_device(m, 0, c.data(), 4000, pose));  // grow_pools + free list, scratch, staged tail
    counts(m, "4000");
    auto d = grid(100, 0, 300);
    CHECK(kicp_map_update_pose_device(m, 0, d.data(), 100, pose));   // one queue, collected at once
    counts(m, "100");
    CHECK(kicp_map_update_pose_device_begin(m, 0, d.data(), 100, pose));
    counts(m, "begun");
    publish(m, 0);
    double cloud[3 * 64];
    std::printf("kicp_map_pointcloud with a pending update -> %zu\n", kicp_map_pointcloud(m, cloud, 64));  // collects; the gather's count check fails (no kernel ran): fall-back
    counts(m, "collected by pointcloud");
    std::vector<float> rec(3 * 6000);
    size_t total = 0;
    CHECK(kicp_map_pointcloud_f32(m, rec.data(), 6000, &total));
    // the host takes a deferred update over (error 1 from the claim step)
    CHECK(kicp_map_update_pose_device(m, 0, d.data(), 100, pose));  // device ahead again
    CHECK(kicp_map_update_pose_device_begin(m, 0, d.data(), 100, pose));
    publish(m, 1);
    CHECK(kicp_map_update_finish(m));
    counts(m, "handed to the host");
    std::printf("  points %zu voxels %zu check %zu\n", kicp_map_num_points(m), kicp_map_num_voxels(m), kicp_map_check(m));
    kicp_map *copy = nullptr;
    CHECK(kicp_map_clone(m, &copy));
    CHECK(kicp_map_update_pose_device(copy, 0, d.data(), 100, pose));  // stays on the host
    CHECK(kicp_map_clear(copy));
    CHECK(kicp_map_update_pose_device(copy, 0, c.data(), 4000, pose));  // fresh table: re-hash on the "device", pools from nothing
    counts(copy, "copy after clear");
    CHECK(kicp_map_update_pose_device_begin(copy, 0, d.data(), 100, pose));
    if (copy->pending.active) publish(copy, 0);
    kicp_map_destroy(copy);  // destroyed with the update pending
    // bulk insertion through the staging buffer into a fresh map
    kicp_map *bulk = nullptr;
    CHECK(kicp_map_create(1.0, 1000.0, 20, &bulk));
    CHECK(kicp_map_set_device(bulk, 0));
    auto e = grid(5000, 500, 0);
    CHECK(kicp_map_add_points(bulk, e.data(), 5000));
    CHECK(kicp_map_update_pose(bulk, e.data(), 5000, pose));
    counts(bulk, "bulk");
    double q[3] = {1, 1, 1}, nn[3], dist;
    CHECK(kicp_map_closest(bulk, 0, q, 1, nn, &dist));
    kicp_map_destroy(bulk);
    kicp_map_destroy(m);
    std::printf("done, %d calls failed\n", g_failed);
    return g_failed ? 1 : 0;
}
