// kicp_map_internal.hpp -- what the voxel map's translation units share beyond kicp_internal.hpp (the handle, map_sync,
// ensure_host_current, map_finish_pending).  Each unit includes the kernel header of what it launches and no other:
//   kicp_map.hip          the handle's C entries, the HBM mirror (map_sync: full and delta upload; ensure_host_current), the batch
//                         GetClosestNeighbor                                                       kicp_map_kernels.hpp
//   kicp_map_update.hip   Update on the device: map_update_device with its re-hash and pool growth, map_finish_pending, bulk insertions,
//                         the C entries that add points                                            kicp_mapdev.hpp
//   kicp_map_cloud.hip    Pointcloud() from the device copy, as doubles and as FLOAT32 records    kicp_map_pc.hpp, kicp_scan_blocks.hpp
// kicp_view.hip (the sweep of kicp_map_remove_seen_through) includes this header for dev_map().
#pragma once
#include "kicp_devmap.hpp"
#include "kicp_internal.hpp"

namespace kicp {
namespace host {

// the entries of kicp_map::update_counts (kicp_map_update_counts, include/kicp.h)
enum UpdateCount { kCountOneQueue = 0, kCountStaged, kCountSecondClaims, kCountRehashes, kCountPoolGrowths, kCountApplyWave, kCountApplyThread,
                   kCountWideScans, kCountHostUpdates, kCountDeferred, kCountTouched, kCountRecordPieces };

// points of the 16-bit mirror that go with `pool_doubles` doubles of the fp64 pool (bucket strides cap / cap16)
inline size_t mirror_points(size_t pool_doubles, uint32_t cap) { return pool_doubles / (static_cast<size_t>(cap) * 3) * mirror_stride(cap); }
// room of the free-list stack in buckets (the allocation holds one more element)
inline size_t free_cap(const DeviceMirror &mr) { return mr.d_free_list.capacity() ? mr.d_free_list.capacity() - 1 : 0; }
// buckets the device pools can hold
inline size_t bucket_capacity(const DeviceMirror &mr, uint32_t cap) { return mr.d_pool.capacity() / (static_cast<size_t>(cap) * 3); }

// the table of a synced map (map_sync) as the kernels that maintain it take it
inline DevMap dev_map(const kicp_map &map) {
    const DeviceMirror &mr = map.mirror;
    const HostMap &h = map.host;
    DevMap m{};
    m.table = mr.d_table.get(), m.keys64 = mr.d_keys64.get(), m.mask = static_cast<uint32_t>(mr.live_slots - 1);
    m.pool = mr.d_pool.get(), m.pool16 = mr.d_pool16.get(), m.cap = h.cap(), m.cbits = h.count_bits();
    m.bucket_capacity = static_cast<uint32_t>(bucket_capacity(mr, h.cap()));
    m.voxel_size = h.voxel_size(), m.max_distance = h.max_distance();
    m.free_list = mr.d_free_list.get(), m.cnt = mr.d_cnt.get(), m.seg_start = mr.d_seg_start.get(), m.ctr = mr.d_ctr.get();
    return m;
}

// Replace both device pools by new ones of `doubles` doubles (and the mirror points that go with them), with what the old ones hold
// - copied on the device, queued on `stream` and waited for (kOnStream: map_sync) or by plain hipMemcpy (kBlocking: the update) - or
// without (kDrop: a full upload follows).  mirror.view follows.  Nothing has changed when this fails.  (kicp_map.hip)
enum class PoolContents { kDrop, kOnStream, kBlocking };
int replace_pools(DeviceMirror &mr, uint32_t cap, size_t doubles, PoolContents keep, hipStream_t stream);
// k_build_keys64 over the first `slots` slots of the mirror's table, queued on `stream` (kicp_map_update.hip: the kernel is one of
// kicp_mapdev.hpp's, sync_aux of kicp_map.hip needs it after every upload)
void enqueue_build_keys64(const DeviceMirror &mr, size_t slots, hipStream_t stream);
// collect a pending update where the caller has no way to report its failure
inline void collect_pending(const kicp_map *map) { (void)map_finish_pending(const_cast<kicp_map *>(map)); }

}  // namespace host
}  // namespace kicp
