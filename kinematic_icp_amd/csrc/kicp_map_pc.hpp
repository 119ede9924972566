// kicp_map_pc.hpp -- Pointcloud() from the device copy of the map (KinematicICP.hpp:92, published by the ROS node when someone listens):
// k_pc_count, k_pc_gather (kicp_map_pointcloud) and k_pc_records (kicp_map_pointcloud_f32).  `static __global__`: a unit that includes
// this header emits all three, so only kicp_map_cloud.hip, which launches them, does.  The block scan between the count and the gather
// is kicp_scan_blocks.hpp's.
//
// All points, voxel by voxel in table order - the order HostMap::Pointcloud emits - without bringing the table and the
// pools back to the host: count per 256-slot block, scan the block totals, then every slot copies its bucket's points.
// (Free slots are recognised in the packed-key side array, 8 B per slot: the 128-byte slots of a mostly empty table are never read.)
#pragma once
#include "kicp_devmap.hpp"

namespace kicp {

static __global__ __launch_bounds__(256) void k_pc_count(const Slot *table, const unsigned long long *keys64, uint32_t slots, uint32_t cbits, uint32_t *block_counts) {
    __shared__ uint32_t s_sum[4];
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    uint32_t c = 0;
    if (h < slots && keys64[h] != kEmptyKey64 && table[h].val != kEmptyVal) c = val_count(table[h].val, cbits);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}
static __global__ __launch_bounds__(256) void k_pc_gather(const Slot *table, const unsigned long long *keys64, uint32_t slots, const double *pool,
                                                   uint32_t cap, uint32_t cbits, const uint32_t *block_offsets, double *out) {
    __shared__ uint32_t s_wave[4];
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c = 0, bucket = 0;
    if (h < slots && keys64[h] != kEmptyKey64 && table[h].val != kEmptyVal) c = val_count(table[h].val, cbits), bucket = val_bucket(table[h].val, cbits);
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t pos = block_offsets[blockIdx.x] + incl - c;
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
    const double *b = pool + static_cast<size_t>(bucket) * cap * 3;
    double *o = out + static_cast<size_t>(pos) * 3;
    for (uint32_t k = 0; k < 3 * c; ++k) o[k] = b[k];
}

// ---- the local map as PointCloud2 records (kicp_map_pointcloud_f32; RosUtils.cpp:40-63 EigenToPointCloud2) ------------------
// The same table walk as k_pc_gather, narrowed on the device (static_cast<float>: v_cvt_f32_f64, round to nearest even, float
// subnormals kept, +-inf beyond the float range, signs of zeros kept) and stored as x y z FLOAT32 records - 12 bytes, i.e. the
// fp64 cloud's doubles one by one as floats - straight into host-mapped pinned memory.  One launch writes the records [lo, hi) of
// the map (a "piece"; the host cuts the map into pieces and reuses a few landing slots); its last workgroup announces the piece in
// host memory as k_push_frame does: bytes, system-scope release, ticket, flag = (seq << 32) | the table's own point count.
//
// Shape: a workgroup takes one 256-slot block of the table at a time (grid-stride from the first block that reaches `lo`, found by
// binary search over the scanned block offsets).  Its records are contiguous in the output but each lane owns a run of 0..cap of
// them, at an offset no lane controls: the lanes first put their floats into LDS (kPcRoundRecords records per round, 24 KB), then
// the workgroup writes the round out in 16-byte units - lane i the i-th unit - so that every store instruction of a wave covers
// 1 KB of contiguous PCIe writes; only the up to three words before the first and after the last 16-byte boundary of a round go
// out as single dwords.  (Stores of 12-byte records straight from the lanes would be 3-dword stores at the lanes' own scattered
// offsets.)  Record lo sits at dst[0]; lo is a multiple of 4, so 16-byte boundaries of the map's word index are those of dst.
constexpr uint32_t kPcRoundRecords = 2048;
struct PcRecordParams {
    const Slot *table;
    const unsigned long long *keys64;
    uint32_t slots, cap, cbits, blocks;
    const double *pool;
    const uint32_t *block_offsets;  // [blocks + 1]: k_scan_blocks of k_pc_count's counts, the total behind them
    uint32_t lo, hi;                // records of this piece
    float *dst;                     // its landing slot as the device sees it
    unsigned long long *ticket;     // device counter of the slot, never reset
    unsigned long long ticket_done; // its value once this launch's last workgroup has drawn
    unsigned long long *host_flag;  // pinned, host-coherent
    uint32_t seq;
};
static __global__ __launch_bounds__(256) void k_pc_records(const PcRecordParams q) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    __shared__ float s_rec[3 * kPcRoundRecords];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the first block whose records reach past lo: block_offsets[b + 1] > lo (the offsets never decrease)
    uint32_t first = 0, last = q.blocks;
    while (first < last) {
        const uint32_t mid = (first + last) >> 1;
        if (q.block_offsets[mid + 1] > q.lo) last = mid;
        else first = mid + 1;
    }
    for (uint32_t blk = first + blockIdx.x; blk < q.blocks && q.block_offsets[blk] < q.hi; blk += gridDim.x) {
        const uint32_t h = blk * 256 + threadIdx.x;
        uint32_t c = 0, bucket = 0;
        if (h < q.slots && q.keys64[h] != kEmptyKey64 && q.table[h].val != kEmptyVal) c = val_count(q.table[h].val, q.cbits), bucket = val_bucket(q.table[h].val, q.cbits);
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        __syncthreads();  // (s_wave and s_rec of the previous block are free)
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        const uint32_t base = q.block_offsets[blk];
        uint32_t mine = base + incl - c;  // this lane's first record
        for (int w = 0; w < wave; ++w) mine += s_wave[w];
        const uint32_t block_end = base + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        const uint32_t r0 = base > q.lo ? base : q.lo, r1 = block_end < q.hi ? block_end : q.hi;
        const double *b = q.pool + static_cast<size_t>(bucket) * q.cap * 3;
        for (uint32_t rs = r0; rs < r1; rs += kPcRoundRecords) {
            const uint32_t re = rs + kPcRoundRecords < r1 ? rs + kPcRoundRecords : r1;
            const uint32_t k0 = rs > mine ? rs - mine : 0u, k1 = re > mine ? (re - mine < c ? re - mine : c) : 0u;
            for (uint32_t k = k0; k < k1; ++k) {
                float *o = s_rec + 3 * (mine + k - rs);
                o[0] = static_cast<float>(b[3 * k]), o[1] = static_cast<float>(b[3 * k + 1]), o[2] = static_cast<float>(b[3 * k + 2]);
            }
            __syncthreads();
            // words [w0, w1) of the map go out; word w sits at dst[w - 3 lo] and at s_rec[w - w0]
            const uint32_t w0 = 3 * rs, w1 = 3 * re, wlo = 3 * q.lo;
            const uint32_t u0 = (w0 + 3) & ~3u, u1 = w1 & ~3u;  // the 16-byte units wholly inside
            if (u0 < u1) {
                for (uint32_t u = u0 + 4 * threadIdx.x; u < u1; u += 1024) {
                    const float *s = s_rec + (u - w0);
                    *reinterpret_cast<f32x4 *>(q.dst + (u - wlo)) = f32x4{s[0], s[1], s[2], s[3]};
                }
                if (threadIdx.x < u0 - w0) q.dst[w0 + threadIdx.x - wlo] = s_rec[threadIdx.x];
                if (threadIdx.x >= 64 && threadIdx.x - 64 < w1 - u1) q.dst[u1 + (threadIdx.x - 64) - wlo] = s_rec[u1 + (threadIdx.x - 64) - w0];
            } else if (threadIdx.x < w1 - w0) {  // (fewer words than one unit's boundary to the next)
                q.dst[w0 + threadIdx.x - wlo] = s_rec[threadIdx.x];
            }
            __syncthreads();
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        // system scope: this workgroup's bytes are in host memory before its ticket - and so before the flag, whoever writes it
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = __hip_atomic_fetch_add(q.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == q.ticket_done ? 1u : 0u;
        if (s_last) __hip_atomic_store(q.host_flag, (static_cast<unsigned long long>(q.seq) << 32) | q.block_offsets[q.blocks], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace kicp
