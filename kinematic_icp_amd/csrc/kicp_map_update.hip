// kicp_map_update.hip -- VoxelHashMap::Update on the device copy of the map (kernels: kicp_mapdev.hpp): map_update_device with its
// re-hash and pool growth, the deferred end of an update (map_finish_pending), bulk insertions of host points, and the C entries
// that add points.  The mirror it works on is kicp_map.hip's (kicp_map_internal.hpp says which unit holds what).
#include "kicp_map_internal.hpp"
#include "kicp_mapdev.hpp"

using namespace kicp;
using namespace kicp::host;

namespace kicp {
namespace host {
void enqueue_build_keys64(const DeviceMirror &mr, size_t slots, hipStream_t stream) {
    hipLaunchKernelGGL(k_build_keys64, dim3(static_cast<uint32_t>(std::min<size_t>((slots + 255) / 256, 4096))), dim3(256), 0, stream, mr.d_table.get(),
                       static_cast<uint32_t>(slots), mr.d_keys64.get());
}
}  // namespace host
}  // namespace kicp

namespace {

// one update as its steps pass it on (and as a deferred one waits in kicp_map::pending): the points, still in the local frame and
// in HBM, the pose, and the origin of the pruning step if there is one
using Update = kicp_map::PendingUpdate;
Update make_update(const double *d_points, size_t n, const Pose &pose, const double *remove_origin) {
    Update u;
    u.points = d_points, u.n = n, u.pose = pose, u.has_origin = remove_origin != nullptr;
    if (remove_origin) u.origin[0] = remove_origin[0], u.origin[1] = remove_origin[1], u.origin[2] = remove_origin[2];
    return u;
}

// What DevMapCounters::error says at the end of an update: 0 = done (KICP_OK), 1 = a voxel the packed keys cannot express, the host
// map redoes the update (kRerunOnHost, a positive value no C-ABI call returns), 3 = table full, anything else = out of room.
constexpr int kRerunOnHost = 1;
int decode_update_error(uint32_t error) {
    if (error == 3) return fail(KICP_ERR_CAPACITY, "device-side map update: voxel table full");
    if (error == 1) return kRerunOnHost;
    if (error) return fail(KICP_ERR_CAPACITY, "device-side map update ran out of room");
    return KICP_OK;
}

// A frame's worth of points, or of touched voxels: up to here an update may be one queue of kernels, scans its voxels in one
// workgroup (k_up_scan) and applies them a wave each (k_up_apply); beyond, it is a bulk insertion
constexpr size_t kFrameSizedUpdate = 16384;
// The table keeps a load factor of at most 0.75, so that no probe sequence can run away, even if each of `count` voxels adds
// `per_voxel` entries to the `entries` it holds: 27 for a point that may be a new voxel with 26 new neighbours, 26 for a voxel whose
// own entry is already claimed
bool has_head_room(const DeviceMirror &mr, uint32_t entries, unsigned long long per_voxel, size_t count) {
    return (entries + per_voxel * count) * 4 <= mr.live_slots * 3ull;
}

// the update on the host map: what degenerate calls take, and maps that hold a voxel the packed keys cannot express
int update_on_host(kicp_map *map, const Update &u) {
    const size_t n = u.n;
    map->last_update_on_device = 0;
    ++map->update_counts[kCountHostUpdates];
    std::vector<double> pts(3 * n);
    if (n) HIP_TRY(hipMemcpy(pts.data(), u.points, n * 24, hipMemcpyDeviceToHost));
    if (int rc = ensure_host_current(map)) return rc;
    map->host.ReserveEntries(32 * n + 1024);
    std::vector<double> w(3 * n);
    for (size_t i = 0; i < n; ++i) {
        double rx, ry, rz;
        quat_rotate(u.pose, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], rx, ry, rz);
        w[3 * i] = rx + u.pose.tx, w[3 * i + 1] = ry + u.pose.ty, w[3 * i + 2] = rz + u.pose.tz;
    }
    if (!map->host.AddPoints(w.data(), n)) return fail(KICP_ERR_CAPACITY, "more than 2^24-2 voxels");
    if (u.has_origin) map->host.RemovePointsFarFromLocation(u.origin);
    return KICP_OK;
}
// A voxel coordinate beyond +-2^20 (the packed keys' range; the reference has no such limit): nothing was inserted for such points,
// and what the claim step did insert are plain halo entries.  The host map takes this update - and every later one of this map - over.
int hand_to_host(kicp_map *map, const Update &u) {
    map->host_updates_only = true;
    return update_on_host(map, u);
}

// make the device pools (and the free-list stack) hold at least `want_buckets` buckets, keeping their contents
int grow_pools(kicp_map *map, size_t want_buckets) {
    DeviceMirror &mr = map->mirror;
    const uint32_t cap = map->host.cap();
    const size_t have = bucket_capacity(mr, cap);
    if (want_buckets <= have && have <= free_cap(mr)) return KICP_OK;
    const size_t buckets = std::max(want_buckets + want_buckets / 2 + 1024, have);
    DevBuf<uint32_t> nf;
    if (int rc = nf.reserve(buckets + 1)) return rc;
    if (int rc = replace_pools(mr, cap, buckets * cap * 3, PoolContents::kBlocking, nullptr)) return rc;
    if (free_cap(mr)) HIP_TRY(hipMemcpy(nf.get(), mr.d_free_list.get(), std::min(free_cap(mr), buckets) * 4, hipMemcpyDeviceToDevice));
    std::swap(mr.d_free_list, nf);  // (the old one goes with the local)
    ++map->update_counts[kCountPoolGrowths];
    return KICP_OK;
}

int ensure_update_scratch(DeviceMirror &mr, size_t n) {
    if (n <= mr.d_touched.capacity()) return KICP_OK;
    mr.d_world.release(), mr.d_slot_of.release(), mr.d_order.release(), mr.d_touched.release();  // (d_touched's capacity speaks for all four)
    const size_t cap = n + n / 4 + 1024;
    if (int rc = mr.d_world.reserve(cap * 3)) return rc;
    if (int rc = mr.d_slot_of.reserve(cap)) return rc;
    if (int rc = mr.d_order.reserve(cap)) return rc;
    return mr.d_touched.reserve(cap);
}

// Move the live entries of the device table into a fresh table with room for `extra_entries` more at a load factor of
// at most 0.25 (the host map's ReserveEntries rule).  The HBM copy becomes the authoritative one.
int device_rehash(kicp_map *map, size_t extra_entries) {
    DeviceMirror &mr = map->mirror;
    hipStream_t st = nullptr;
    const size_t old_slots = mr.live_slots;
    ++map->update_counts[kCountRehashes];
    HIP_TRY(hipMemsetAsync(&mr.d_ctr.get()->touched, 0, 8, st));  // touched (borrowed as the live counter) + error
    mr.ctr_clean = false;
    const uint32_t grid_old = static_cast<uint32_t>(std::min<size_t>((old_slots + 255) / 256, 8192));
    hipLaunchKernelGGL(k_rehash_count, dim3(grid_old), dim3(256), 0, st, mr.d_table.get(), static_cast<uint32_t>(old_slots), map->host.count_bits(), &mr.d_ctr.get()->touched);
    uint32_t live = 0;
    HIP_TRY(hipMemcpy(&live, &mr.d_ctr.get()->touched, 4, hipMemcpyDeviceToHost));
    size_t want = 1024;
    while ((live + extra_entries) * 4 > want) want *= 2;
    if (want > (1ull << 31)) return fail(KICP_ERR_CAPACITY, "voxel table would exceed 2^31 slots");
    DevBuf<Slot> nt;
    DevBuf<unsigned long long> nk;
    DevBuf<uint32_t> nc, ns;
    if (int rc = nt.reserve(want)) return rc;
    if (int rc = nk.reserve(want)) return rc;
    if (int rc = nc.reserve(want)) return rc;
    if (int rc = ns.reserve(want)) return rc;
    const uint32_t grid_new = static_cast<uint32_t>(std::min<size_t>((want + 255) / 256, 8192));
    hipLaunchKernelGGL(k_table_clear, dim3(grid_new), dim3(256), 0, st, nt.get(), static_cast<uint32_t>(want));
    HIP_TRY(hipMemsetAsync(nk.get(), 0xFF, want * 8, st));
    HIP_TRY(hipMemsetAsync(nc.get(), 0, want * 4, st));
    hipLaunchKernelGGL(k_rehash_move, dim3(grid_old), dim3(256), 0, st, mr.d_table.get(), static_cast<uint32_t>(old_slots), nt.get(), nk.get(),
                       static_cast<uint32_t>(want - 1), map->host.count_bits(), &mr.d_ctr.get()->error);
    HIP_TRY(hipGetLastError());
    map->dev.n_entries = live, map->dev.touched = 0;
    HIP_TRY(hipMemcpyAsync(&mr.d_ctr.get()->n_entries, &map->dev.n_entries, 4, hipMemcpyHostToDevice, st));
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, &mr.d_ctr.get()->error, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipStreamSynchronize(st));
    std::swap(mr.d_table, nt), std::swap(mr.d_keys64, nk), std::swap(mr.d_cnt, nc), std::swap(mr.d_seg_start, ns);  // (the old ones go with the locals)
    mr.live_slots = want;
    mr.view.table = mr.d_table.get(), mr.view.mask = static_cast<uint32_t>(want - 1);
    map->device_ahead = true;
    if (err) return fail(KICP_ERR_CAPACITY, "a voxel coordinate left the +-2^20 range of the device-side map update");
    return KICP_OK;
}

// ---- the steps of map_update_device, in the order it takes them; the map's kernels run on the null stream ------------------------
constexpr hipStream_t kMapStream = nullptr;

// The mirror current on `device`, with room for the points' own voxels: <= n new buckets (the pools grow on the device) and <= n new
// table entries without leaving the probing regime (re-hash, on the device, when the table is short)
int prepare_update(kicp_map *map, int device, size_t n) {
    if (int rc = set_device(device)) return rc;
    if (int rc = map_sync(map, device, nullptr)) return rc;
    if (map->dev.n_buckets_hi + n > max_buckets(map->host.count_bits())) return fail(KICP_ERR_CAPACITY, "more voxels than the table's bucket index can address (2^24-2 for max_points_per_voxel <= 255)");
    if (int rc = grow_pools(map, map->dev.n_buckets_hi + n)) return rc;
    if (int rc = ensure_update_scratch(map->mirror, n)) return rc;
    if ((map->dev.n_entries + n) * 2 > map->mirror.live_slots) return device_rehash(map, 32 * n + 1024);
    return KICP_OK;
}
// the kernels' arguments; taken again after a re-hash, which replaces the table
UpdateParams bind_update(const kicp_map &map, const Update &u) {
    const DeviceMirror &mr = map.mirror;
    UpdateParams up{};
    up.m = dev_map(map);
    up.in = u.points, up.n = static_cast<uint32_t>(u.n), up.pose = u.pose, up.world = mr.d_world.get(), up.slot_of = mr.d_slot_of.get(), up.order = mr.d_order.get();
    up.touched = mr.d_touched.get();
    return up;
}
// steps 1 and 2: the per-update counters at zero (`trust_clean`: unless k_up_publish left them so), the claim, the scan
int enqueue_claims(kicp_map *map, const UpdateParams &up, bool trust_clean) {
    DeviceMirror &mr = map->mirror;
    const size_t n = up.n;
    const uint32_t grid = static_cast<uint32_t>((n + 255) / 256);
    if (!(trust_clean && mr.ctr_clean)) HIP_TRY(hipMemsetAsync(&mr.d_ctr.get()->touched, 0, 12, kMapStream));  // touched + error + may_occupy
    mr.ctr_clean = false;
    hipLaunchKernelGGL(k_up_claim, dim3(grid), dim3(256), 0, kMapStream, up);
    if (n > kFrameSizedUpdate) {  // bulk: the scan over many workgroups (the number of touched voxels is only known on the device: <= n)
        const uint32_t spans = static_cast<uint32_t>((n + kScanSpan - 1) / kScanSpan);
        ++map->update_counts[kCountWideScans];
        hipLaunchKernelGGL(k_up_scan_local, dim3(spans), dim3(256), 0, kMapStream, up, mr.d_order.get());
        hipLaunchKernelGGL(k_up_scan_sums, dim3(1), dim3(1024), 0, kMapStream, up, mr.d_order.get());
        hipLaunchKernelGGL(k_up_scan_add, dim3(grid), dim3(256), 0, kMapStream, up, mr.d_order.get());
    } else {
        hipLaunchKernelGGL(k_up_scan, dim3(1), dim3(1024), 0, kMapStream, up);
    }
    return KICP_OK;
}
// steps 3, 4 and the far-voxel sweep; `touched_bound`: the number of touched voxels, or an upper bound of it (the kernels
// read the exact number on the device)
int enqueue_apply(kicp_map *map, const UpdateParams &up, const Update &u, size_t touched_bound) {
    hipLaunchKernelGGL(k_up_scatter, dim3(static_cast<uint32_t>((u.n + 255) / 256)), dim3(256), 0, kMapStream, up);
    if (touched_bound <= kFrameSizedUpdate && up.m.cap <= kApplyMaxPoints) {  // a frame's worth of voxels: one wave each; bulk insertions: one thread each (kicp_mapdev.hpp steps 4 / 4b)
        hipLaunchKernelGGL(k_up_apply, dim3(static_cast<uint32_t>((touched_bound + kApplyWaves - 1) / kApplyWaves)), dim3(64 * kApplyWaves), 0, kMapStream, up);
        ++map->update_counts[kCountApplyWave];
    } else {
        hipLaunchKernelGGL(k_up_apply_thread, dim3(static_cast<uint32_t>((touched_bound + 63) / 64)), dim3(64), 0, kMapStream, up);
        ++map->update_counts[kCountApplyThread];
    }
    if (u.has_origin)
        hipLaunchKernelGGL(k_up_remove, dim3(static_cast<uint32_t>(std::min<size_t>((map->mirror.live_slots / 4 + 255) / 256, 8192))), dim3(256), 0, kMapStream, up.m,
                           u.origin[0], u.origin[1], u.origin[2]);
    HIP_TRY(hipGetLastError());
    return KICP_OK;
}
// wait for what is queued and bring the counters it left; the table carries the update's entries from here on
int read_counters(kicp_map *map, DevMapCounters &c) {
    HIP_TRY(hipMemcpyAsync(&c, map->mirror.d_ctr.get(), sizeof c, hipMemcpyDeviceToHost, kMapStream));
    HIP_TRY(hipStreamSynchronize(kMapStream));
    map->device_ahead = true;
    return KICP_OK;
}
// The claims of an update without room for the worst case, with the host looking at the counters in between: every touched voxel
// that holds no point yet - a fresh entry or a halo entry that existed before - may become occupied in k_up_apply and then adds up
// to 26 halo entries of its own; the update only goes ahead with that head-room.  Too tight: the entries just claimed are still
// plain halo entries without an occupied neighbour, so a re-hash drops them together with the per-slot counters of this attempt;
// then claim again, once, in the larger table.  kRerunOnHost: the claim step met a voxel the packed keys cannot express.
int staged_claims(kicp_map *map, const Update &u, UpdateParams &up, DevMapCounters &c) {
    for (int attempt = 0;; ++attempt) {
        up = bind_update(*map, u);
        if (attempt) ++map->update_counts[kCountSecondClaims];
        if (int rc = enqueue_claims(map, up, false)) return rc;
        if (int rc = read_counters(map, c)) return rc;
        const int rc = decode_update_error(c.error);  // (the claim and scan steps raise 1 or 3 only)
        if (rc != KICP_OK && rc != kRerunOnHost) return rc;
        map->dev = c;
        if (rc) return rc;
        if (has_head_room(map->mirror, c.n_entries, 26, c.may_occupy)) return KICP_OK;
        if (attempt) return fail(KICP_ERR_CAPACITY, "device-side map update found no room after a re-hash");
        if (int rc2 = device_rehash(map, 32 * u.n + 1024)) return rc2;
    }
}
// the end of a one-queue update left for the caller to collect later (kicp_map_update_finish, or whatever it calls on the map next):
// the counters land in pinned memory, nothing is waited for here
int defer_end(kicp_map *map, const Update &u) {
    DeviceMirror &mr = map->mirror;
    if (!mr.h_ctr.get()) {
        if (int rc = mr.h_ctr.reserve(8, hipHostMallocMapped | hipHostMallocCoherent)) return rc;
        std::memset(mr.h_ctr.get(), 0, 8 * sizeof(unsigned long long));
    }
    hipLaunchKernelGGL(k_up_publish, dim3(1), dim3(64), 0, kMapStream, mr.d_ctr.get(), mr.h_ctr.dev(), ++mr.ctr_seq);
    HIP_TRY(hipGetLastError());
    mr.ctr_clean = true;
    map->device_ahead = true;
    map->pending = u, map->pending.active = true;
    map->last_update_on_device = 1;  // (corrected by the finish step should the host have to take the update over)
    ++map->update_counts[kCountDeferred];
    return KICP_OK;
}
// The end of an update whose last counters `c` have arrived: take them over; an error is returned; error 1 hands the update to the
// host map where that can still redo it (`host_redo`; nullptr: too late for the host, the points are in - KICP_ERR_CAPACITY then);
// otherwise the update counts as done on the device.
int end_update(kicp_map *map, const DevMapCounters &c, const Update *host_redo) {
    map->dev = c;
    if (int rc = decode_update_error(c.error)) {
        if (rc != kRerunOnHost) return rc;
        return host_redo ? hand_to_host(map, *host_redo) : fail(KICP_ERR_CAPACITY, "device-side map update ran out of room");
    }
    map->last_update_on_device = 1, ++map->device_updates;
    map->update_counts[kCountTouched] = c.touched;  // (k_up_publish sends the counters before it zeroes this one)
    return KICP_OK;
}

// VoxelHashMap::Update(points, pose) = transform + AddPoints + RemovePointsFarFromLocation(pose.translation) with the points
// already in HBM.  Runs on the device, table growth and pool growth included; only degenerate calls (no points) take the
// host path.  `defer`: a one-queue update leaves its end to map_finish_pending.
int map_update_device(kicp_map *map, int device, const Update &u, bool defer = false) {
    if (int rc = map_finish_pending(map)) return rc;
    map->last_update_on_device = 0;
    // (a map that holds a voxel the packed keys cannot express - through host-side AddPoints, or inherited by a clone - stays on
    //  the host: the device kernels would alias its key)
    if (u.n == 0 || u.n > 0x7FFFFFF0ull / 3 || map->host_updates_only || map->host.has_far_voxel()) return update_on_host(map, u);
    if (int rc = prepare_update(map, device, u.n)) return rc;
    UpdateParams up{};
    DevMapCounters c{};
    // With room for the worst case - every point a new voxel with 26 new neighbours - nothing has to be asked of the device in
    // between and the update is ONE queue of kernels behind one synchronisation; a claim step that gives up (voxel coordinate out
    // of range) turns the later steps into no-ops.
    if (u.n <= kFrameSizedUpdate && has_head_room(map->mirror, map->dev.n_entries, 27, u.n)) {
        up = bind_update(*map, u);
        ++map->update_counts[kCountOneQueue];
        if (int rc = enqueue_claims(map, up, true)) return rc;
        if (int rc = enqueue_apply(map, up, u, u.n)) return rc;
        if (defer) return defer_end(map, u);
        if (int rc = read_counters(map, c)) return rc;
        return end_update(map, c, &u);
    }
    ++map->update_counts[kCountStaged];
    if (int rc = staged_claims(map, u, up, c)) return rc == kRerunOnHost ? hand_to_host(map, u) : rc;
    if (int rc = enqueue_apply(map, up, u, c.touched)) return rc;
    if (int rc = read_counters(map, c)) return rc;
    return end_update(map, c, nullptr);
}

// Host-side AddPoints / Update calls with many points go through the device path when the map has a preferred device
// (kicp_map_set_device): the points are staged into HBM and inserted there - the same map as the host insertion builds
// (tests/test_gpu_mapdev.py), an order of magnitude faster (the host table's 128-byte slots and 27 neighbour records per
// newly occupied voxel make the host insertion cache-miss bound: 9 us per point at cfg5's 2.9M voxels).
constexpr size_t kBulkThreshold = 4096;
int bulk_insert(kicp_map *map, const double *xyz, size_t n, const Pose &pose, const double *remove_origin) {
    const int device = map->bulk_device;
    if (int rc = set_device(device)) return rc;
    if (n > map->d_bulk.capacity() / 3)
        if (int rc = map->d_bulk.reserve((n + n / 4 + 1024) * 3)) return rc;
    if (int rc = staged_upload(map->mirror.stage, 0, map->d_bulk.get(), xyz, n * 24, nullptr)) return rc;
    return map_update_device(map, device, make_update(map->d_bulk.get(), n, pose, remove_origin));
}
// Update(points, pose) with the points in HBM, pruning around the pose's translation
int update_pose_device(kicp_map *map, int device, const double *d_points_xyz, size_t n, const double pose_qt[7], bool defer) {
    if (!map || (!d_points_xyz && n) || !pose_qt) return fail(KICP_ERR_ARG, "null argument");
    const Pose pose = pose_from(pose_qt);
    const double origin[3] = {pose.tx, pose.ty, pose.tz};
    return map_update_device(map, device, make_update(d_points_xyz, n, pose, origin), defer);
}
bool use_bulk(const kicp_map *map, size_t n) { return map->bulk_device >= 0 && n >= kBulkThreshold; }
const Pose kIdentityPose{0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};

}  // namespace

namespace kicp {
namespace host {
// The end of an update begun with defer = true: wait for its kernels, take the counters over, and - should the claim step have met
// a voxel the packed keys cannot express - let the host map redo the update from the (still borrowed) points.
int map_finish_pending(kicp_map *map) {
    if (!map->pending.active) return KICP_OK;
    map->pending.active = false;
    DeviceMirror &mr = map->mirror;
    if (int rc = set_device(mr.device)) return rc;
    // the update's last launch said so in host memory (k_up_publish)
    const volatile unsigned long long *words = mr.h_ctr.get();
    if (int rc = wait_word(words + 7, mr.ctr_seq, ~0ull, nullptr, 2.0, "the map update finished without handing its counters over")) return rc;
    DevMapCounters c;
    unsigned long long raw[5];
    for (int w = 0; w < 5; ++w) raw[w] = words[w];
    std::memcpy(&c, raw, sizeof c);
    return end_update(map, c, &map->pending);
}
}  // namespace host
}  // namespace kicp

extern "C" {

int kicp_map_add_points(kicp_map *map, const double *xyz, size_t n) {
    KICP_TRACE_CALL();
    if (!map || (!xyz && n)) return fail(KICP_ERR_ARG, "null argument");
    if (use_bulk(map, n)) return bulk_insert(map, xyz, n, kIdentityPose, nullptr);
    if (int rc = ensure_host_current(map)) return rc;
    return map->host.AddPoints(xyz, n) ? KICP_OK : fail(KICP_ERR_CAPACITY, "more than 2^24-2 voxels");
}
int kicp_map_update_origin(kicp_map *map, const double *xyz, size_t n, const double origin[3]) {
    KICP_TRACE_CALL();
    if (!map || (!xyz && n) || !origin) return fail(KICP_ERR_ARG, "null argument");
    if (use_bulk(map, n)) return bulk_insert(map, xyz, n, kIdentityPose, origin);
    if (int rc = ensure_host_current(map)) return rc;
    return map->host.Update(xyz, n, origin) ? KICP_OK : fail(KICP_ERR_CAPACITY, "more than 2^24-2 voxels");
}
int kicp_map_update_pose(kicp_map *map, const double *xyz, size_t n, const double pose_qt[7]) {
    KICP_TRACE_CALL();
    if (!map || (!xyz && n) || !pose_qt) return fail(KICP_ERR_ARG, "null argument");
    if (use_bulk(map, n)) {
        const Pose pose = pose_from(pose_qt);
        const double origin[3] = {pose.tx, pose.ty, pose.tz};
        return bulk_insert(map, xyz, n, pose, origin);
    }
    if (int rc = ensure_host_current(map)) return rc;
    return map->host.Update(xyz, n, pose_from(pose_qt)) ? KICP_OK : fail(KICP_ERR_CAPACITY, "more than 2^24-2 voxels");
}
int kicp_map_update_pose_device(kicp_map *map, int device, const double *d_points_xyz, size_t n, const double pose_qt[7]) {
    KICP_TRACE_CALL();
    return update_pose_device(map, device, d_points_xyz, n, pose_qt, false);
}
// The same update in two halves: _begin queues its kernels (and the copy of its counters) and returns without waiting - the caller
// goes on with host-side work that does not touch the map (the pipeline collects the frame's returned clouds) -, kicp_map_update_finish
// waits and takes the result over.  `d_points_xyz` stays borrowed until then.  Frame-sized updates into a table with room for the
// worst case take this route; anything else (table growth, bulk insertions, a map that lives on the host) runs to completion inside
// _begin.  Any other call on the map finishes a pending update first.
int kicp_map_update_pose_device_begin(kicp_map *map, int device, const double *d_points_xyz, size_t n, const double pose_qt[7]) {
    KICP_TRACE_CALL();
    // (queuing the update's six launches from a thread of the map's own - ~20 us of API time off the caller's thread - was measured:
    //  the frame then waits that much longer for its way back; no gain)
    return update_pose_device(map, device, d_points_xyz, n, pose_qt, true);
}
int kicp_map_update_finish(kicp_map *map) {
    KICP_TRACE_CALL();
    if (!map) return fail(KICP_ERR_ARG, "null map");
    return map_finish_pending(map);
}

}  // extern "C"
