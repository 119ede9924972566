// kicp_devmap.hpp -- the device-maintained voxel table as a kernel sees it: the DevMap aggregate, the packed voxel keys and the two
// lookups over them.  No kernel in here, so any unit that works on the device table may include it without emitting one:
//   kicp_mapdev.hpp   the update's kernels (kicp_map_update.hip)
//   kicp_map_pc.hpp   the Pointcloud kernels (kicp_map_cloud.hip)
//   kicp_view.hpp     the sweep of kicp_map_remove_seen_through (kicp_view.hip)
// The host fills a DevMap in one place, dev_map() of kicp_map_internal.hpp.
//
// Table slots are claimed with a 64-bit CAS on a parallel array of packed voxel keys (voxel coordinates within +-2^20: beyond that the
// host map takes the update over - the reference has no such limit).
#pragma once
#include "kicp_common.hpp"

namespace kicp {

constexpr unsigned long long kEmptyKey64 = ~0ull;

struct DevMap {
    Slot *table;
    unsigned long long *keys64;  // packed key of every live entry, kEmptyKey64 otherwise (find-or-insert by CAS)
    uint32_t mask;
    double *pool;
    MirrorPoint *pool16;
    uint32_t cap;
    uint32_t cbits;              // count bits of Slot::val (count_bits_for(cap))
    uint32_t bucket_capacity;    // buckets the pools can hold
    double voxel_size, max_distance;
    uint32_t *free_list;         // stack of reusable bucket ids
    uint32_t *cnt;               // per slot: new points of the running update (zero between updates)
    uint32_t *seg_start;         // per slot: start of the voxel's group in `order`
    DevMapCounters *ctr;
};

__device__ __forceinline__ unsigned long long pack_key64(int32_t x, int32_t y, int32_t z, bool &ok) {
    const int lim = 1 << 20;
    ok = x >= -lim && x < lim && y >= -lim && y < lim && z >= -lim && z < lim;
    return (static_cast<unsigned long long>(static_cast<uint32_t>(z + lim) & 0x1FFFFFu) << 42) |
           (static_cast<unsigned long long>(static_cast<uint32_t>(y + lim) & 0x1FFFFFu) << 21) |
           static_cast<unsigned long long>(static_cast<uint32_t>(x + lim) & 0x1FFFFFu);
}

// slot of voxel (x,y,z); creates a halo entry when absent.  Same probe sequence as the host map (voxel_hash, linear).
// The host keeps the table below a load factor of 0.75 (has_head_room, kicp_map_update.hip), so a probe sequence is
// short; should the table ever be full all the same, the walk stops after one lap, raises ctr->error = 3 and returns
// kNoSlot (callers skip their writes; the host reports KICP_ERR_CAPACITY) instead of spinning for ever.
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t dev_find_or_insert(const DevMap &m, int32_t x, int32_t y, int32_t z) {
    bool ok;
    const unsigned long long key = pack_key64(x, y, z, ok);
    if (!ok) {  // outside the packable range: nothing is inserted; the host sees the flag and takes the update over (kicp_map_update.hip)
        m.ctr->error = 1u;
        return kNoSlot;
    }
    uint32_t h = voxel_hash(x, y, z) & m.mask;
    for (uint32_t probes = 0;; ++probes) {
        if (probes > m.mask) {
            m.ctr->error = 3u;
            return kNoSlot;
        }
        const unsigned long long seen = atomicCAS(m.keys64 + h, kEmptyKey64, key);
        if (seen == kEmptyKey64) {  // this thread owns the new entry: key fields and the halo marker (nbr is already 0)
            m.table[h].x = x, m.table[h].y = y, m.table[h].z = z;
            m.table[h].val = halo_val(m.cbits);
            atomicAdd(&m.ctr->n_entries, 1u);
            return h;
        }
        if (seen == key) return h;
        h = (h + 1) & m.mask;
    }
}
// read-only lookup; 0xFFFFFFFF when the voxel has no entry
__device__ __forceinline__ uint32_t dev_find(const DevMap &m, int32_t x, int32_t y, int32_t z) {
    bool ok;
    const unsigned long long key = pack_key64(x, y, z, ok);
    uint32_t h = voxel_hash(x, y, z) & m.mask;
    for (uint32_t probes = 0; probes <= m.mask; ++probes) {
        const unsigned long long seen = m.keys64[h];
        if (seen == kEmptyKey64) return kNoSlot;
        if (seen == key) return h;
        h = (h + 1) & m.mask;
    }
    return kNoSlot;
}

// The later steps of an update that the claim step gave up on (a voxel coordinate out of the packable range: error 1; table
// full: 3) do nothing - with a single host synchronisation per update the host only learns of it at the end.  (Error 2 is
// raised inside step 4 itself and is not a reason for its other waves to stop.)
__device__ __forceinline__ bool claim_failed(const DevMap &m) {
    const uint32_t err = m.ctr->error;
    return err == 1u || err == 3u;
}

}  // namespace kicp
