// kicp_map.hip -- kiss_icp::VoxelHashMap behind include/kicp.h: the handle's C entries, the host map (kicp_host_map.hpp), its HBM
// mirror (full and delta upload, lazy refresh of the host copy) and the batch GetClosestNeighbor.  The device-side Update is
// kicp_map_update.hip's, Pointcloud() kicp_map_cloud.hip's (kicp_map_internal.hpp says which unit holds what).
#include "kicp_map_internal.hpp"
#include "kicp_map_kernels.hpp"  // k_scatter_rows, k_closest

using namespace kicp;
using namespace kicp::host;

namespace {
// release every device buffer of a mirror (on its own device) and reset it
void free_mirror(DeviceMirror &mr) {
    if (mr.device >= 0) hipSetDevice(mr.device);
    mr = DeviceMirror{};
}

// per-slot helper arrays, free list and counters of the device-side maintenance, rebuilt after every upload
int sync_aux(kicp_map *map, hipStream_t stream) {
    DeviceMirror &mr = map->mirror;
    const HostMap &h = map->host;
    const size_t slots = h.table().size();
    if (slots != mr.d_seg_start.capacity()) {  // (d_seg_start: the last of the three, so that a failed growth is made up for here)
        mr.d_keys64.release(), mr.d_cnt.release(), mr.d_seg_start.release();
        if (int rc = mr.d_keys64.reserve(slots)) return rc;
        if (int rc = mr.d_cnt.reserve(slots)) return rc;
        if (int rc = mr.d_seg_start.reserve(slots)) return rc;
        HIP_TRY(hipMemsetAsync(mr.d_cnt.get(), 0, slots * 4, stream));
    }
    const size_t bucket_cap = bucket_capacity(mr, h.cap());
    if (bucket_cap > free_cap(mr))
        if (int rc = mr.d_free_list.reserve(bucket_cap + 1)) return rc;
    if (int rc = mr.d_ctr.reserve(1)) return rc;
    enqueue_build_keys64(mr, slots, stream);
    DevMapCounters c{};
    c.n_points = h.num_points(), c.n_voxels = static_cast<uint32_t>(h.num_voxels()), c.n_entries = static_cast<uint32_t>(h.num_entries());
    c.n_buckets_hi = static_cast<uint32_t>(h.buckets_in_use_hi()), c.free_count = static_cast<uint32_t>(h.free_list().size());
    if (c.free_count) HIP_TRY(hipMemcpyAsync(mr.d_free_list.get(), h.free_list().data(), c.free_count * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(mr.d_ctr.get(), &c, sizeof c, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    map->dev = c;
    return KICP_OK;
}

// scatter `rows` staged rows of `row_words` 8-byte words each into dst at the given row indices
int upload_rows(DeviceMirror &mr, const std::vector<uint2> &staged, const std::vector<uint32_t> &index, uint32_t row_words, void *dst,
                hipStream_t stream) {
    if (index.empty()) return KICP_OK;
    if (staged.size() > mr.d_stage.capacity())
        if (int rc = mr.d_stage.reserve(staged.size() + staged.size() / 2)) return rc;
    if (index.size() > mr.d_index.capacity())
        if (int rc = mr.d_index.reserve(index.size() + index.size() / 2)) return rc;
    HIP_TRY(hipMemcpyAsync(mr.d_stage.get(), staged.data(), staged.size() * sizeof(uint2), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(mr.d_index.get(), index.data(), index.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    const size_t total = staged.size();
    const uint32_t grid = static_cast<uint32_t>(std::min<size_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(k_scatter_rows, dim3(grid), dim3(256), 0, stream, mr.d_stage.get(), mr.d_index.get(), static_cast<uint32_t>(index.size()), row_words,
                       static_cast<uint2 *>(dst));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));  // the staging vectors are reused by the caller
    mr.last_upload_bytes += staged.size() * sizeof(uint2) + index.size() * sizeof(uint32_t);
    return KICP_OK;
}

}  // namespace

namespace kicp {
namespace host {

int replace_pools(DeviceMirror &mr, uint32_t cap, size_t doubles, PoolContents keep, hipStream_t stream) {
    DevBuf<double> np;
    DevBuf<MirrorPoint> np32;
    if (int rc = np.reserve(doubles)) return rc;
    if (int rc = np32.reserve(mirror_points(doubles, cap))) return rc;
    if (keep != PoolContents::kDrop && mr.d_pool.get()) {
        const size_t bytes = mr.d_pool.capacity() * sizeof(double), bytes32 = mirror_points(mr.d_pool.capacity(), cap) * sizeof(MirrorPoint);
        if (keep == PoolContents::kOnStream) {
            HIP_TRY(hipMemcpyAsync(np.get(), mr.d_pool.get(), bytes, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(np32.get(), mr.d_pool16.get(), bytes32, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        } else {
            HIP_TRY(hipMemcpy(np.get(), mr.d_pool.get(), bytes, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(np32.get(), mr.d_pool16.get(), bytes32, hipMemcpyDeviceToDevice));
        }
    }
    std::swap(mr.d_pool, np), std::swap(mr.d_pool16, np32);  // (the old pools go with the locals)
    mr.view.pool = mr.d_pool.get(), mr.view.pool16 = mr.d_pool16.get();
    return KICP_OK;
}

int map_sync(kicp_map *map, int device, hipStream_t stream) {
    if (int rc = map_finish_pending(map)) return rc;
    DeviceMirror &mr = map->mirror;
    HostMap &h = map->host;
    if (map->device_ahead) {
        if (mr.device == device) return KICP_OK;  // the HBM copy is the current one
        if (int rc = ensure_host_current(map)) return rc;
    }
    if (mr.device == device && mr.synced_epoch == h.epoch()) return KICP_OK;
    if (int rc = set_device(device)) return rc;
    if (mr.device != device && mr.device >= 0) {  // mirror lives on another GPU: drop it
        free_mirror(mr);
        hipSetDevice(device);
    }
    mr.device = device;
    const size_t slots = h.table().size();
    const uint32_t cap = h.cap();
    const size_t pool_doubles = h.buckets_in_use_hi() * static_cast<size_t>(cap) * 3;
    bool full = mr.synced_generation != h.generation() || mr.live_slots != slots;
    if (slots > mr.d_table.capacity()) {
        if (int rc = mr.d_table.reserve(slots)) return rc;
        full = true;
    }
    if (pool_doubles > mr.d_pool.capacity())  // grow the pools; a delta upload keeps what is already there
        if (int rc = replace_pools(mr, cap, pool_doubles + pool_doubles / 2 + 3 * 1024, full ? PoolContents::kDrop : PoolContents::kOnStream, stream)) return rc;
    mr.last_upload_bytes = 0;
    // delta only pays off while the changed part is small
    if (!full && (h.dirty_slots().size() * 4 > slots || h.dirty_buckets().size() * 2 > h.buckets_in_use_hi())) full = true;
    if (full) {
        HIP_TRY(hipMemcpyAsync(mr.d_table.get(), h.table().data(), slots * sizeof(Slot), hipMemcpyHostToDevice, stream));
        if (pool_doubles) HIP_TRY(hipMemcpyAsync(mr.d_pool.get(), h.pool().data(), pool_doubles * sizeof(double), hipMemcpyHostToDevice, stream));
        if (pool_doubles) HIP_TRY(hipMemcpyAsync(mr.d_pool16.get(), h.pool16().data(), mirror_points(pool_doubles, cap) * sizeof(MirrorPoint), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        mr.last_upload_bytes = slots * sizeof(Slot) + pool_doubles * sizeof(double) + mirror_points(pool_doubles, cap) * sizeof(MirrorPoint);
    } else {
        // gather the changed rows on the host, ship them with their indices, scatter on the device
        std::vector<uint2> staged;
        const std::vector<uint32_t> &ds = h.dirty_slots(), &db = h.dirty_buckets();
        staged.resize(ds.size() * (sizeof(Slot) / 8));
        for (size_t i = 0; i < ds.size(); ++i) std::memcpy(&staged[i * (sizeof(Slot) / 8)], &h.table()[ds[i]], sizeof(Slot));
        if (int rc = upload_rows(mr, staged, ds, sizeof(Slot) / 8, mr.d_table.get(), stream)) return rc;
        staged.resize(db.size() * static_cast<size_t>(cap) * 3);
        for (size_t i = 0; i < db.size(); ++i)
            std::memcpy(&staged[i * static_cast<size_t>(cap) * 3], &h.pool()[static_cast<size_t>(db[i]) * cap * 3], static_cast<size_t>(cap) * 24);
        if (int rc = upload_rows(mr, staged, db, cap * 3, mr.d_pool.get(), stream)) return rc;
        const size_t cap16 = h.cap16();
        staged.resize(db.size() * cap16);  // one 8-byte word per mirror point
        for (size_t i = 0; i < db.size(); ++i)
            std::memcpy(&staged[i * cap16], &h.pool16()[static_cast<size_t>(db[i]) * cap16], cap16 * sizeof(MirrorPoint));
        if (int rc = upload_rows(mr, staged, db, static_cast<uint32_t>(cap16), mr.d_pool16.get(), stream)) return rc;
    }
    mr.last_upload_full = full ? 1 : 0;
    if (int rc = sync_aux(map, stream)) return rc;
    h.mark_synced(full);
    mr.view = MapView{mr.d_table.get(), static_cast<uint32_t>(slots - 1), mr.d_pool.get(), mr.d_pool16.get(), cap, h.cap16(), h.voxel_size(), h.count_bits()};
    mr.synced_epoch = h.epoch(), mr.synced_generation = h.generation(), mr.live_slots = slots;
    return KICP_OK;
}

// bring the host copy up to date after device-side updates: same layouts, so this is a plain download
int ensure_host_current(kicp_map *map) {
    if (int rc = map_finish_pending(map)) return rc;
    if (!map->device_ahead) return KICP_OK;
    TraceScope trace_scope_("  (host copy refreshed from HBM)");
    DeviceMirror &mr = map->mirror;
    if (int rc = set_device(mr.device)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    DevMapCounters c{};
    HIP_TRY(hipMemcpy(&c, mr.d_ctr.get(), sizeof c, hipMemcpyDeviceToHost));
    const uint32_t cap = map->host.cap();
    std::vector<Slot> table(mr.live_slots);
    std::vector<double> pool(static_cast<size_t>(c.n_buckets_hi) * cap * 3);
    std::vector<MirrorPoint> pool16(static_cast<size_t>(c.n_buckets_hi) * map->host.cap16());
    std::vector<uint32_t> free_list(c.free_count);
    HIP_TRY(hipMemcpy(table.data(), mr.d_table.get(), table.size() * sizeof(Slot), hipMemcpyDeviceToHost));
    if (!pool.empty()) HIP_TRY(hipMemcpy(pool.data(), mr.d_pool.get(), pool.size() * 8, hipMemcpyDeviceToHost));
    if (!pool16.empty()) HIP_TRY(hipMemcpy(pool16.data(), mr.d_pool16.get(), pool16.size() * sizeof(MirrorPoint), hipMemcpyDeviceToHost));
    if (!free_list.empty()) HIP_TRY(hipMemcpy(free_list.data(), mr.d_free_list.get(), free_list.size() * 4, hipMemcpyDeviceToHost));
    map->host.Adopt(std::move(table), std::move(pool), std::move(pool16), c.n_buckets_hi, std::move(free_list));
    map->host.mark_synced(true);
    mr.synced_epoch = map->host.epoch(), mr.synced_generation = map->host.generation();  // the mirror already holds this state
    map->device_ahead = false;
    return KICP_OK;
}

}  // namespace host
}  // namespace kicp

extern "C" {

// ---- map ------------------------------------------------------------------------------------------------------------
int kicp_map_create(double voxel_size, double max_distance, unsigned int max_points_per_voxel, kicp_map **out) {
    if (!out || !(voxel_size > 0.0) || max_points_per_voxel == 0) return fail(KICP_ERR_ARG, "bad map parameters");
    if (max_points_per_voxel > kMaxPointsPerVoxel) return fail(KICP_ERR_CAPACITY, "max_points_per_voxel > 65535");
    *out = new kicp_map(voxel_size, max_distance, max_points_per_voxel);
    return KICP_OK;
}
void kicp_map_destroy(kicp_map *map) {
    if (!map) return;
    collect_pending(map);
    if (map->d_bulk.get()) {
        hipSetDevice(map->bulk_device >= 0 ? map->bulk_device : 0);
        map->d_bulk.release();
    }
    free_mirror(map->mirror);
    delete map;
}
int kicp_map_clone(const kicp_map *map, kicp_map **out) {
    if (!map || !out) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = ensure_host_current(const_cast<kicp_map *>(map))) return rc;  // (refreshing the host copy does not change the map's value)
    kicp_map *c = new kicp_map(map->host.voxel_size(), map->host.max_distance(), map->host.cap());
    c->host = map->host;  // table, pools, free list, counters; the copy's mirror starts empty and uploads on first use
    c->bulk_device = map->bulk_device;
    c->host_updates_only = map->host_updates_only;
    *out = c;
    return KICP_OK;
}
int kicp_map_set_device(kicp_map *map, int device) {
    if (!map) return fail(KICP_ERR_ARG, "null map");
    if (device >= 0) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return fail(KICP_ERR_ARG, "device index out of range");
    }
    if (map->d_bulk.get() && device != map->bulk_device) {
        hipSetDevice(map->bulk_device);
        map->d_bulk.release();
    }
    map->bulk_device = device < 0 ? -1 : device;
    return KICP_OK;
}
int kicp_map_clear(kicp_map *map) {
    KICP_TRACE_CALL();
    if (!map) return fail(KICP_ERR_ARG, "null map");
    collect_pending(map);  // (its kernels must have left the table before anything else is queued on it)
    map->device_ahead = false;  // whatever the device holds is obsolete now
    map->host_updates_only = false;
    map->host.Clear();
    return KICP_OK;
}
int kicp_map_empty(const kicp_map *map) {
    if (!map) return 1;
    collect_pending(map);
    return (map->device_ahead ? map->dev.n_voxels == 0 : map->host.Empty()) ? 1 : 0;
}
int kicp_map_remove_far(kicp_map *map, const double origin[3]) {
    KICP_TRACE_CALL();
    if (!map || !origin) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = ensure_host_current(map)) return rc;
    map->host.RemovePointsFarFromLocation(origin);
    return KICP_OK;
}
unsigned long long kicp_map_device_updates(const kicp_map *map) { return map ? map->device_updates : 0ull; }  // (no collecting: kicp.h)
int kicp_map_update_counts(const kicp_map *map, unsigned long long out[12]) {
    if (!map || !out) return fail(KICP_ERR_ARG, "null argument");
    for (int k = 0; k < 12; ++k) out[k] = map->update_counts[k];  // (host-side counters: no device call, a pending update stays pending)
    return KICP_OK;
}
int kicp_map_last_update_on_device(const kicp_map *map) {
    if (map) collect_pending(map);
    return map ? map->last_update_on_device : 0;
}
size_t kicp_map_num_points(const kicp_map *map) {
    if (!map) return 0;
    collect_pending(map);
    return map->device_ahead ? static_cast<size_t>(map->dev.n_points) : map->host.num_points();
}
size_t kicp_map_num_voxels(const kicp_map *map) {
    if (!map) return 0;
    collect_pending(map);
    return map->device_ahead ? map->dev.n_voxels : map->host.num_voxels();
}
size_t kicp_map_check(const kicp_map *map) {
    if (!map || ensure_host_current(const_cast<kicp_map *>(map)) != KICP_OK) return 1;
    return map->host.CheckInvariants();
}
int kicp_map_sync(kicp_map *map, int device) {
    KICP_TRACE_CALL();
    if (!map) return fail(KICP_ERR_ARG, "null map");
    if (int rc = set_device(device)) return rc;
    return map_sync(map, device, nullptr);
}
size_t kicp_map_device_bytes(const kicp_map *map) {
    if (!map || !map->mirror.d_table.get()) return 0;
    // what a query can touch: the table's entries (occupied + halo) and the buckets of the occupied voxels, not the head-room
    // around them
    const size_t entries = map->device_ahead ? map->dev.n_entries : map->host.num_entries();
    const size_t voxels = map->device_ahead ? map->dev.n_voxels : map->host.num_voxels();
    return entries * sizeof(Slot) + voxels * (static_cast<size_t>(map->host.cap()) * 24 + static_cast<size_t>(map->host.cap16()) * sizeof(MirrorPoint));
}
int kicp_map_last_upload(const kicp_map *map, size_t *bytes, int *was_full) {
    if (!map || !bytes || !was_full) return fail(KICP_ERR_ARG, "null argument");
    *bytes = map->mirror.last_upload_bytes, *was_full = map->mirror.last_upload_full;
    return KICP_OK;
}
int kicp_map_closest(kicp_map *map, int device, const double *queries_xyz, size_t n, double *out_nn_xyz, double *out_dist) {
    KICP_TRACE_CALL();
    if (!map || (!queries_xyz && n) || !out_nn_xyz || !out_dist) return fail(KICP_ERR_ARG, "null argument");
    if (n == 0) return KICP_OK;
    if (kicp_map_empty(map)) {
        for (size_t i = 0; i < n; ++i) out_nn_xyz[3 * i] = out_nn_xyz[3 * i + 1] = out_nn_xyz[3 * i + 2] = 0.0, out_dist[i] = DBL_MAX;
        return KICP_OK;
    }
    if (int rc = kicp_map_sync(map, device)) return rc;
    DevBuf<double> d_q, d_nn, d_d;
    if (int rc = d_q.reserve(n * 3)) return rc;
    if (int rc = d_nn.reserve(n * 3)) return rc;
    if (int rc = d_d.reserve(n)) return rc;
    if (int rc = staged_upload(map->mirror.stage, 0, d_q.get(), queries_xyz, n * 24, nullptr)) return rc;
    hipLaunchKernelGGL(k_closest, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, nullptr, d_q.get(), static_cast<uint32_t>(n),
                       map->mirror.view, d_nn.get(), d_d.get());
    HIP_TRY(hipGetLastError());
    if (int rc = staged_download(map->mirror.stage, out_nn_xyz, d_nn.get(), n * 24, nullptr)) return rc;
    return staged_download(map->mirror.stage, out_dist, d_d.get(), n * 8, nullptr);
}

}  // extern "C"
