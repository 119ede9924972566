// kicp_pre_ingest.hpp -- the kernels that decode a sensor message on the GPU (PointCloud2 records, LaserScan ranges) and the
// projector's rules the host shares with them (laser_rules); included by kicp_pre_ingest.hip alone.
#pragma once
#include <cmath>
#include "kicp_common.hpp"
#include "kicp_se3.hpp"
#include "kicp_ordered_key.hpp"
#include "kicp_pre_shared.hpp"

namespace kicp {

// ---- PointCloud2 wire-format ingest ----------------------------------------------------
// ros/src/kinematic_icp_ros/utils/RosUtils.cpp:30-39 (PointCloud2ToEigen: float32 x,y,z at point_step stride -> fp64,
// T * p) and TimeStampHandler.cpp:57-104 (per-point stamp of type uint32 / float32 / float64 -> double seconds, values
// with more than 10 integer digits are nanoseconds) + :106,:121-128 (min/max, normalisation to [0,1]).
// The raw message bytes are what crosses PCIe (point_step bytes per point instead of 32 B of inflated fp64).
struct IngestParams {
    const unsigned char *raw;  // first record of THIS launch's piece: pinned host memory as the device sees it (the records are decoded
                               // straight out of the staging buffer, round 6: no copy of the bytes in HBM), or HBM where that is unavailable
    uint32_t first;            // index of that record in the cloud (a multiple of 256)
    uint32_t n;                // records of the piece
    uint32_t point_step;
    uint32_t off_x, off_y, off_z, off_t;
    int32_t stamp_type;  // 0 none, 6 UINT32, 7 FLOAT32, 8 FLOAT64 (sensor_msgs::msg::PointField datatype codes)
    int32_t transform;   // 0: identity (what LidarOdometryServer.cpp:203 passes)
    int32_t aligned;     // every field sits at a multiple of its size (base pointer, point_step and offsets): plain loads instead of byte-wise ones
    Pose T;
    double *out_xyz;     // the whole cloud's arrays
    double *out_stamps;  // seconds, NOT normalised: the extrema go to the host, which hands them to whoever consumes the stamps
    unsigned long long *block_minmax;  // [workgroups of the cloud][2] the stamps' extrema per workgroup as order-preserving integer keys
    // the cloud's pieces are launches of their own (each behind the CPU's copy of its bytes into the staging buffer); the workgroup
    // that finishes LAST - over all pieces - folds the extrema and tells the host, which polls `host_rec`
    unsigned long long *ticket;      // device counter, never reset
    unsigned long long ticket_done;  // its value once the cloud's last workgroup has drawn
    uint32_t total_blocks;
    unsigned long long *host_rec;    // pinned: [0] min key [1] max key [2] seq
    unsigned long long seq;
};

template <typename T>
__device__ __forceinline__ T load_unaligned(const unsigned char *p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}
// (ordered_key / ordered_value, the order-preserving map double <-> uint64 the block extrema are merged through: kicp_ordered_key.hpp)
template <typename T>
__device__ __forceinline__ T load_field(const unsigned char *p, bool aligned) {
    return aligned ? *reinterpret_cast<const T *>(p) : load_unaligned<T>(p);
}
// a decoded stamp in seconds (k_ingest, k_ingest_scan)
// TimeStampHandler.cpp:60-63,73-78: floor(log10(uint64(round(stamp))) + 1) > 10  <=>  round(stamp) >= 1e10
__device__ __forceinline__ double stamp_seconds(double stamp) {
    if (round(stamp) >= 1e10) stamp *= 1e-9;
    return stamp;
}
static __global__ __launch_bounds__(256) void k_ingest(const IngestParams p) {
    __shared__ unsigned long long s_min[4], s_max[4];
    __shared__ uint32_t s_last;
    unsigned long long kmin = ~0ull, kmax = 0ull;
    const bool al = p.aligned != 0;  // (wave-uniform: the usual PointCloud2 layouts are naturally aligned)
    // A workgroup's 256 records are contiguous bytes: they cross PCIe as full 16-byte loads per lane (one request per 64 bytes
    // whatever the field layout is; four 4-byte field loads per record were four times the requests and 17 GB/s) into LDS and are
    // picked apart there.  Records longer than kLdsStep bytes are read field by field from where they are.
    // The launch's workgroups go round its tiles of 256 records: this call's message has one workgroup per tile; a look-ahead message
    // gets a few dozen (kicp_pre_ingest.hip ingest_run) - with all of its 2 MB requested at once, every kernel the frame dispatched in
    // the meantime waited ~50 us for ITS packet and arguments to cross the same PCIe read queue.
    constexpr uint32_t kLdsStep = 128;
    __shared__ __attribute__((aligned(16))) unsigned char s_rec[256 * kLdsStep];
    const bool via_lds = p.point_step <= kLdsStep;
    const uint32_t tiles = (p.n + 255u) / 256u;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t first_local = tile * 256u, local = first_local + threadIdx.x, i = p.first + local;
        if (via_lds) {
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            const uint32_t wg_bytes = (p.n - first_local < 256u ? p.n - first_local : 256u) * p.point_step;
            const unsigned char *src = p.raw + static_cast<size_t>(first_local) * p.point_step;
            if (tile != blockIdx.x) __syncthreads();  // (the previous tile's records have been picked apart)
            for (uint32_t o = threadIdx.x * 16u; o < wg_bytes; o += 4096u) {
                if (o + 16u <= wg_bytes) *reinterpret_cast<u32x4 *>(s_rec + o) = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src + o));
                else
                    for (uint32_t k = o; k < wg_bytes; ++k) s_rec[k] = src[k];
            }
            __syncthreads();
        }
        kmin = ~0ull, kmax = 0ull;
        if (local < p.n) {
            const unsigned char *rec = via_lds ? s_rec + threadIdx.x * p.point_step : p.raw + static_cast<size_t>(local) * p.point_step;
            double x = static_cast<double>(load_field<float>(rec + p.off_x, al));
            double y = static_cast<double>(load_field<float>(rec + p.off_y, al));
            double z = static_cast<double>(load_field<float>(rec + p.off_z, al));
            if (p.transform) {
                double rx, ry, rz;
                quat_rotate(p.T, x, y, z, rx, ry, rz);
                x = rx + p.T.tx, y = ry + p.T.ty, z = rz + p.T.tz;
            }
            store_through(p.out_xyz + 3 * i, x), store_through(p.out_xyz + 3 * i + 1, y), store_through(p.out_xyz + 3 * i + 2, z);
            if (p.stamp_type) {
                double stamp;
                if (p.stamp_type == 6) stamp = static_cast<double>(load_field<uint32_t>(rec + p.off_t, al));
                else if (p.stamp_type == 7) stamp = static_cast<double>(load_field<float>(rec + p.off_t, al));
                else stamp = load_field<double>(rec + p.off_t, al);
                stamp = stamp_seconds(stamp);
                store_through(p.out_stamps + i, stamp);
                kmin = kmax = ordered_key(stamp);
            }
        }
        if (p.stamp_type) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long a = __shfl_xor(kmin, off, 64), b = __shfl_xor(kmax, off, 64);
                kmin = a < kmin ? a : kmin, kmax = b > kmax ? b : kmax;
            }
            if (tile != blockIdx.x) __syncthreads();  // (the previous tile's extrema have been folded)
            if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = kmin, s_max[threadIdx.x >> 6] = kmax;
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int w = 1; w < 4; ++w) kmin = s_min[w] < kmin ? s_min[w] : kmin, kmax = s_max[w] > kmax ? s_max[w] : kmax;
                const uint32_t gb = p.first / 256u + tile;
                store_through(p.block_minmax + 2 * gb, kmin), store_through(p.block_minmax + 2 * gb + 1, kmax);
            }
        }
    }
    // The decoded cloud is read by kernels of other launches (and, after a look-ahead upload, of another stream) once the host has
    // seen the record: every store above went through to memory (store_through); every wave waits for its own, then the workgroup
    // draws its ticket.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(p.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == p.ticket_done ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    // TimeStampHandler.cpp:106: the extrema over the whole cloud
    kmin = ~0ull, kmax = 0ull;
    if (p.stamp_type) {
        for (uint32_t b = threadIdx.x; b < p.total_blocks; b += 256u) {
            const unsigned long long a = __hip_atomic_load(p.block_minmax + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long c = __hip_atomic_load(p.block_minmax + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            kmin = a < kmin ? a : kmin, kmax = c > kmax ? c : kmax;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long a = __shfl_xor(kmin, off, 64), c = __shfl_xor(kmax, off, 64);
            kmin = a < kmin ? a : kmin, kmax = c > kmax ? c : kmax;
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = kmin, s_max[threadIdx.x >> 6] = kmax;
        __syncthreads();
        for (int w = 0; w < 4; ++w) kmin = s_min[w] < kmin ? s_min[w] : kmin, kmax = s_max[w] > kmax ? s_max[w] : kmax;
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(p.host_rec + 0, kmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p.host_rec + 1, kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(p.host_rec + 2, p.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- 2-D LaserScan ingest ------------------------------------------------------------------------------------------------------
// ros/src/kinematic_icp_ros/nodes/online_node.cpp:44-58 (use_2d_lidar): laser_projector_.projectLaser(*msg, cloud, -1.0,
// channel_option::Timestamp), then RegisterFrame(cloud): ProcessTimestamps (the field "stamps" is accepted, TimeStampHandler.cpp:42-52)
// and PointCloud2ToEigen.  A projected scan is a PointCloud2 of 16-byte records (x y z stamps, FLOAT32), so from the stamps on the
// FLOAT32 branch of the cloud ingest above applies unchanged (stamp_seconds, the extrema, ts_raw normalisation where consumed).
//
// [RECALLED] laser_geometry is not part of the reference tree.  Every choice below restates laser_geometry 2.x
// (LaserProjection::projectLaser_) from memory, not from its source; this block is the one place to correct them:
//   - the cosine table C[i] = (cos a_i, sin a_i) in double (libm, on the host), a_i = angle_min + (float)i * angle_increment in
//     FLOAT (one product, one sum, each rounded); cached per projector (per kicp_pre handle) and rebuilt only when n, angle_min or
//     angle_max changes - angle_increment is NOT part of the key (a scan that changes only the increment projects with the old table);
//   - range_cutoff < 0 means (double)range_max (the node passes -1.0); a positive cutoff is taken as given, above range_max too;
//   - beam i is kept iff r < cutoff && r >= range_min (float r as written: NaN and +-inf are dropped, range_min is kept, the cutoff is
//     not); the kept beams keep their order;
//   - x = (float)((double)r * C[i].cos), y = (float)((double)r * C[i].sin), z = 0;
//   - the stamp is (float)i * time_increment in float, i the ORIGINAL beam index.
namespace laser_rules {
inline bool table_stale(bool valid, size_t n, float angle_min, float angle_max, size_t cached_n, float cached_min, float cached_max) {
    return !valid || n != cached_n || angle_min != cached_min || angle_max != cached_max;  // (float compares: a NaN angle rebuilds)
}
inline void table_entry(float angle_min, float angle_increment, uint32_t i, double &c, double &s) {  // host: glibc's cos / sin
    const float step = static_cast<float>(i) * angle_increment;
    const float a = angle_min + step;
    c = std::cos(static_cast<double>(a)), s = std::sin(static_cast<double>(a));
}
inline double cutoff(double range_cutoff, float range_max) { return range_cutoff < 0.0 ? static_cast<double>(range_max) : range_cutoff; }
KICP_HD bool keep(float r, double cutoff, float range_min) { return r < cutoff && r >= range_min; }
KICP_HD float coord(float r, double cs) { return static_cast<float>(static_cast<double>(r) * cs); }
KICP_HD float stamp(uint32_t i, float time_increment) { return static_cast<float>(i) * time_increment; }
}  // namespace laser_rules

// One launch on the handle's stream: the keep test, the order-preserving compaction, the points and the raw stamps into the ingest
// slot (d_in / d_ts), and - by the ingest's ticket - the extrema and the kept count into the host record.  A workgroup takes
// `tiles_per_wg` consecutive tiles of 1024 beams (4 per lane, one 16-byte load); its offset in the output is the number of kept beams
// before its first tile, which it counts itself from the ranges (a real scan - <= 8k beams - is a few workgroups; the grid is capped
// at kScanMaxWgs, so the recount reads at most kScanMaxWgs x the scan whatever its size).  Integer counts only: the result does not
// depend on the order in which workgroups run.
constexpr uint32_t kScanTile = 1024, kScanMaxWgs = 32;
struct ScanParams {
    const float *ranges;  // msg->ranges: the pinned staging buffer as the device sees it (or HBM where that is unavailable)
    const double *cs;     // [n][2] the cosine table (HBM)
    uint32_t n;
    uint32_t tiles_per_wg;
    float range_min, time_increment;
    double cutoff;
    double *out_xyz, *out_stamps;       // the ingest slot; stamps in seconds, NOT normalised (as k_ingest)
    uint32_t *wg_counts;                // [workgroups] kept beams of each
    unsigned long long *block_minmax;   // [workgroups][2] the kept stamps' extrema as ordered keys
    unsigned long long *ticket;         // the ingest's device counter (never reset)
    unsigned long long ticket_done;
    unsigned long long *host_rec;       // pinned: [0] min key [1] max key [2] seq [3] kept beams
    unsigned long long seq;
};
// ranges j .. j + 3 (j a multiple of 4) -> the kept ones as bits 0..3; past the end counts as dropped
__device__ __forceinline__ uint32_t scan_keep4(const ScanParams &p, uint32_t j, float r[4]) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    if (j + 4u <= p.n) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p.ranges + j));
        r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
    } else {
        for (uint32_t k = 0; k < 4u; ++k) r[k] = j + k < p.n ? p.ranges[j + k] : __builtin_nanf("");
    }
    uint32_t bits = 0u;
    for (uint32_t k = 0; k < 4u; ++k) bits |= laser_rules::keep(r[k], p.cutoff, p.range_min) ? 1u << k : 0u;
    return bits;
}
__device__ __forceinline__ uint32_t block_sum(uint32_t v) {
    __shared__ uint32_t s_part[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();  // (a caller that loops: the previous turn's readers are done)
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}
static __global__ __launch_bounds__(256) void k_ingest_scan(const ScanParams p) {
    __shared__ unsigned long long s_min[4], s_max[4];
    __shared__ uint32_t s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t first = blockIdx.x * p.tiles_per_wg * kScanTile;  // (< n: the grid has no empty workgroup)
    float r[4];
    uint32_t before = 0u;
#pragma unroll 4
    for (uint32_t j = threadIdx.x * 4u; j < first; j += kScanTile) before += static_cast<uint32_t>(__popc(scan_keep4(p, j, r)));
    const uint32_t offset0 = block_sum(before);
    uint32_t offset = offset0;
    unsigned long long kmin = ~0ull, kmax = 0ull;
    for (uint32_t t = 0; t < p.tiles_per_wg; ++t) {
        const uint32_t base = first + t * kScanTile;
        if (base >= p.n) break;  // (uniform)
        const uint32_t j = base + threadIdx.x * 4u;
        const uint32_t bits = scan_keep4(p, j, r), c = static_cast<uint32_t>(__popc(bits));
        uint32_t incl = c;  // inclusive scan of the lanes' counts: the tile's kept beams stay in beam order
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        __shared__ uint32_t s_wave[4];
        __syncthreads();  // (the previous tile's readers of s_wave are done)
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t pos = offset + incl - c;
        for (int w = 0; w < wave; ++w) pos += s_wave[w];
        for (uint32_t k = 0; k < 4u; ++k) {
            if (!(bits >> k & 1u)) continue;
            const uint32_t i = j + k;
            const double x = static_cast<double>(laser_rules::coord(r[k], p.cs[2 * i]));
            const double y = static_cast<double>(laser_rules::coord(r[k], p.cs[2 * i + 1]));
            const double stamp = stamp_seconds(static_cast<double>(laser_rules::stamp(i, p.time_increment)));
            store_through(p.out_xyz + 3 * pos, x), store_through(p.out_xyz + 3 * pos + 1, y), store_through(p.out_xyz + 3 * pos + 2, 0.0);
            store_through(p.out_stamps + pos, stamp);
            const unsigned long long key = ordered_key(stamp);
            kmin = key < kmin ? key : kmin, kmax = key > kmax ? key : kmax;
            ++pos;
        }
        offset += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long a = __shfl_xor(kmin, off, 64), b = __shfl_xor(kmax, off, 64);
        kmin = a < kmin ? a : kmin, kmax = b > kmax ? b : kmax;
    }
    if (lane == 0) s_min[wave] = kmin, s_max[wave] = kmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) kmin = s_min[w] < kmin ? s_min[w] : kmin, kmax = s_max[w] > kmax ? s_max[w] : kmax;
        store_through(p.block_minmax + 2 * blockIdx.x, kmin), store_through(p.block_minmax + 2 * blockIdx.x + 1, kmax);
        __hip_atomic_store(p.wg_counts + blockIdx.x, offset - offset0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // as k_ingest: every store went through to memory, every wave waits for its own, then the workgroup draws its ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(p.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == p.ticket_done ? 1u : 0u;
    __syncthreads();
    if (!s_last || threadIdx.x != 0) return;
    // the last workgroup: TimeStampHandler.cpp:106 over the kept beams, and their count (gridDim.x <= kScanMaxWgs: one lane suffices)
    kmin = ~0ull, kmax = 0ull;
    unsigned long long kept = 0ull;
    for (uint32_t b = 0; b < gridDim.x; ++b) {
        const unsigned long long a = __hip_atomic_load(p.block_minmax + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long c = __hip_atomic_load(p.block_minmax + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        kmin = a < kmin ? a : kmin, kmax = c > kmax ? c : kmax;
        kept += __hip_atomic_load(p.wg_counts + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_store(p.host_rec + 0, kmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(p.host_rec + 1, kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(p.host_rec + 3, kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(p.host_rec + 2, p.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace kicp
