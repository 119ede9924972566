// kicp_pre.hpp -- the pipeline's pre-steps on the GPU (reference call sites
// pipeline/KinematicICP.cpp:54-62): kiss_icp::Preprocessor::Preprocess (constant-velocity deskew + range crop, kiss-icp
// v1.2.0 core/Preprocessing.cpp) fused with transform_points (KinematicICP.cpp:31-36), and kiss_icp::VoxelDownsample
// (core/VoxelUtils.cpp: first point of every voxel wins, output in the hash table's iteration order).  All of them are
// order-sensitive on the CPU; here the order is made explicit - the crop keeps input order, "first" means lowest input
// index (atomicMin), and the downsample's output order is the reference table's, replayed per cluster - so the results
// are deterministic and equal to the sequential reference's, order included.
// HBM bound streaming kernels: 24-32 B read + <= 24 B written per point, fp64 throughout.
// The kernels of the steps and of the fused chain; included by kicp_pre.hip alone.  The ingest's are in kicp_pre_ingest.hpp, the
// frame's way back in kicp_pre_egress.hpp, the block scan (shared with kicp_map_cloud.hip) in kicp_scan_blocks.hpp.
#pragma once
#include <cmath>
#include "kicp_common.hpp"
#include "kicp_se3.hpp"
#include "kicp_table_order.hpp"
#include "kicp_pre_shared.hpp"
#include "kicp_scan_blocks.hpp"

namespace kicp {

struct PreprocessParams {
    const double *in;          // raw scan, sensor frame
    const double *timestamps;  // normalised to [0,1], or nullptr
    // ts_normalise != 0: `timestamps` still holds the stamps in seconds as the ingest decoded them; (t - ts_lo) / (ts_hi - ts_lo) -
    // TimeStampHandler.cpp:121-128, the same two fp64 operations - happens here, where the stamp is consumed (round 6: the
    // separate normalisation kernel is gone; the extrema come back from the ingest and travel by value)
    double ts_lo, ts_hi;
    int32_t ts_normalise;
    uint32_t n;
    int32_t deskew;
    double omega[6];           // log(relative_motion)
    Pose motion_inverse;       // relative_motion^-1
    Pose lidar_to_base;
    double max_range, min_range;
    uint32_t *flags;           // 1 = survives the crop
    double *staged;            // transformed point of every input (base frame), compacted afterwards
    uint32_t *block_counts;    // survivors per 256-thread block
};

// block-wide count of set predicates -> *out (lane 0 of wave 0 writes)
__device__ __forceinline__ void block_count_store_at(bool pred, uint32_t *out) {
    __shared__ uint32_t s_cnt[4];
    __syncthreads();  // (a caller that loops: the previous turn's reader is done with s_cnt)
    const unsigned long long ballot = __ballot(pred);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(ballot));
    __syncthreads();
    if (threadIdx.x == 0) *out = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}
__device__ __forceinline__ void block_count_store(bool pred, uint32_t *block_counts) { block_count_store_at(pred, block_counts + blockIdx.x); }

// Preprocess + transform_points of point i: deskew to the scan end (when asked), crop decision in the sensor frame, the point in
// the base frame.  Returns whether the point survives the crop.
__device__ __forceinline__ bool preprocess_point(const PreprocessParams &p, uint32_t i, double &bx, double &by, double &bz) {
    double x = p.in[3 * i], y = p.in[3 * i + 1], z = p.in[3 * i + 2];
    if (p.deskew) {  // p' = (relative_motion^-1 * exp(t_i * omega)) * p_i : deskew to the scan end
        double t = p.timestamps[i];
        if (p.ts_normalise) t = (t - p.ts_lo) / (p.ts_hi - p.ts_lo);
        const double xi[6] = {t * p.omega[0], t * p.omega[1], t * p.omega[2], t * p.omega[3], t * p.omega[4], t * p.omega[5]};
        const Pose M = pose_mul(p.motion_inverse, pose_exp(xi));
        double rx, ry, rz;
        quat_rotate(M, x, y, z, rx, ry, rz);
        x = rx + M.tx, y = ry + M.ty, z = rz + M.tz;
    }
    const double r = sqrt(x * x + y * y + z * z);
    quat_rotate(p.lidar_to_base, x, y, z, bx, by, bz);  // transform_points: into the base frame
    bx += p.lidar_to_base.tx, by += p.lidar_to_base.ty, bz += p.lidar_to_base.tz;
    return r < p.max_range && r > p.min_range;  // strict on both sides
}
static __global__ __launch_bounds__(256) void k_preprocess(const PreprocessParams p) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < p.n) {
        double bx, by, bz;
        keep = preprocess_point(p, i, bx, by, bz);
        p.staged[3 * i] = bx, p.staged[3 * i + 1] = by, p.staged[3 * i + 2] = bz;
        p.flags[i] = keep ? 1u : 0u;
    }
    block_count_store(keep, p.block_counts);
}

// order-preserving compaction: survivor i goes to block_offset + (number of survivors before it in its block)
static __global__ __launch_bounds__(256) void k_compact(const double *staged, const uint32_t *flags, const uint32_t *block_counts, int raw, uint32_t *total,
                                                 uint32_t n, double *out) {
    __shared__ uint32_t s_wave[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool keep = i < n && flags[i] != 0u;
    const unsigned long long ballot = __ballot(keep);
    if (lane == 0) s_wave[wave] = static_cast<uint32_t>(__popcll(ballot));
    const uint32_t offset = block_offset(block_counts, raw, total);  // (its barriers also publish s_wave)
    __syncthreads();
    if (!keep) return;
    uint32_t pos = offset + static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
    out[3 * pos] = staged[3 * i], out[3 * pos + 1] = staged[3 * i + 1], out[3 * pos + 2] = staged[3 * i + 2];
}

// ---- VoxelDownsample ----------------------------------------------------------------------------------------------------
// kiss_icp::VoxelDownsample (kiss-icp v1.2.0 core/VoxelUtils.cpp; call sites
// pipeline/KinematicICP.cpp:40,42) keeps the first point of every voxel and returns the survivors in the ITERATION ORDER of
// its tsl::robin_map<Voxel, Vector3d> after reserve(frame.size()).  That order decides which point of a coarser voxel the
// second downsample keeps and the order in which local_map_.Update inserts, so it is reproduced here, in parallel:
//   1. the device table has the reference's bucket count and the reference's ideal bucket (std::hash<Voxel> & mask).
//      Linear probing and robin-hood probing occupy the SAME set of buckets (an insertion always ends in the first free
//      bucket at or after the ideal one), so after k_downsample_claim the occupied slots are the reference's occupied
//      buckets, and every maximal run of occupied slots ("cluster") holds exactly the keys the reference holds there -
//      only their arrangement inside the run differs;
//   2. "first" = lowest input index (atomicMin per slot), which is also the order in which the reference inserted;
//   3. k_downsample_replay: the thread at the head of a run replays the reference's robin-hood insertions of that
//      run's keys, in insertion order, inside the run (insertions never leave their final cluster, so clusters are
//      independent).  Runs are short (load factor <= 0.5 by construction, typically < 0.2);
//   4. the survivors are gathered in ascending bucket index = the reference's iteration order.
constexpr unsigned long long kEmptyVoxelKey = ~0ull;
struct DownsampleParams {
    const double *in;
    uint32_t n;
    double voxel_size;
    unsigned long long *keys;  // [mask+1] packed voxel of the slot, kEmptyVoxelKey when free
    uint32_t *min_index;       // [mask+1] lowest input index seen for the slot's voxel, 0xFFFFFFFF initially
    uint32_t *order;           // [mask+1] after the replay: input index of the point the reference keeps in this bucket
    uint32_t *home_at;         // [mask+1] scratch of the replay: ideal bucket of order[]'s resident
    uint32_t mask;             // the reference's bucket count - 1
    uint32_t *block_counts;    // occupied buckets per 256-slot block
    uint32_t *error;           // set when a voxel coordinate leaves the 21-bit packable range
    uint32_t *probe_max;       // largest robin-hood displacement the replay saw (atomicMax; see replay_cluster)
    // chained pre-steps (kicp_pre_frame_*): the input count is the previous step's survivor count, still on the device; n and mask
    // above are then unused, the launch is sized for an upper bound and every kernel derives the reference's bucket count itself
    const uint32_t *n_dev;
    uint32_t *probe_max_sticky;  // nullable: the chain's second downsample must not reset the first one's figure
};
__device__ __forceinline__ uint32_t ds_count(const DownsampleParams &p) { return p.n_dev ? *p.n_dev : p.n; }
__device__ __forceinline__ uint32_t ds_mask(const DownsampleParams &p, uint32_t n) {
    if (!p.n_dev) return p.mask;
    const uint32_t buckets = reference_bucket_count_u32(n);
    return buckets ? buckets - 1u : 0u;
}

__device__ __forceinline__ unsigned long long pack_voxel21(int32_t x, int32_t y, int32_t z, bool &ok) {
    const int lim = 1 << 20;
    ok = x >= -lim && x < lim && y >= -lim && y < lim && z >= -lim && z < lim;
    return (static_cast<unsigned long long>(static_cast<uint32_t>(z + lim) & 0x1FFFFFu) << 42) |
           (static_cast<unsigned long long>(static_cast<uint32_t>(y + lim) & 0x1FFFFFu) << 21) |
           static_cast<unsigned long long>(static_cast<uint32_t>(x + lim) & 0x1FFFFFu);
}
// the voxel of a point and its key.  +-inf saturates in the conversion and fails the range test; a NaN coordinate converts to 0 and
// would pass for a point of voxel 0: it is out of range too (the reference puts it at INT_MIN, which no table here can hold)
__device__ __forceinline__ unsigned long long voxel_key_of(double x, double y, double z, double vs, bool &ok, int32_t &vx, int32_t &vy, int32_t &vz) {
    const double fx = floor(x / vs), fy = floor(y / vs), fz = floor(z / vs);
    vx = static_cast<int32_t>(fx), vy = static_cast<int32_t>(fy), vz = static_cast<int32_t>(fz);
    const unsigned long long key = pack_voxel21(vx, vy, vz, ok);
    if (fx != fx || fy != fy || fz != fz) ok = false;
    return key;
}
// One point's claim: `key` (kEmptyVoxelKey: this lane has no point) finds / takes its voxel's slot by linear probing from the
// reference's ideal bucket and lowers the slot's winner to `index`.  The lanes of a wave hold CONSECUTIVE, ASCENDING indices.
// `overflow` / `overflow_tag` (the fused chain's first level, whose table size is a guess): a probe longer than kClaimProbeLimit
// gives up and leaves the tag there - a table sized for fewer points than it gets would otherwise be probed for ever.
constexpr uint32_t kClaimProbeLimit = 1024;
__device__ __forceinline__ void claim_voxel(unsigned long long *keys, uint32_t *min_index, uint32_t mask, unsigned long long key, bool ok, int32_t vx, int32_t vy,
                                            int32_t vz, uint32_t index, uint32_t *error, uint32_t *overflow = nullptr, uint32_t overflow_tag = 0u) {
    // Consecutive points of a scan ring fall into the same voxel in long runs (hundreds of points per voxel close to the sensor),
    // and every one of them would hammer the same two words with atomics - the kernel's tail, up to 0.6 ms on some frames.  Only
    // the FIRST lane of a run inside a wave goes on: it has the lowest index of the run, which is all atomicMin would keep.
    const unsigned long long prev = __shfl_up(key, 1, 64);
    if (key == kEmptyVoxelKey) return;
    if (!ok) {  // (before the run test: pack_voxel21 masks, so a voxel 2^21 beyond an in-range one carries that one's key)
        *error = 1u;
        return;
    }
    if ((threadIdx.x & 63) != 0 && prev == key) return;
    uint32_t slot = reference_voxel_hash(vx, vy, vz) & mask;
    for (uint32_t probes = 0;; ++probes) {
        const unsigned long long seen = atomicCAS(keys + slot, kEmptyVoxelKey, key);
        if (seen == kEmptyVoxelKey || seen == key) break;
        if (overflow && probes >= kClaimProbeLimit) {
            *overflow = overflow_tag;
            return;
        }
        slot = (slot + 1) & mask;
    }
    atomicMin(min_index + slot, index);
}
// pass 1: every point claims / finds its voxel's slot (linear probing from the reference's ideal bucket) and lowers the
// slot's winner to its own index
static __global__ __launch_bounds__(256) void k_downsample_claim(const DownsampleParams p) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && !p.probe_max_sticky) *p.probe_max = 0u;  // (the replay kernel, which raises it, runs after this one: no separate memset per call)
    const uint32_t n = ds_count(p), mask = ds_mask(p, n);
    const bool in_range = i < n;
    int32_t vx = 0, vy = 0, vz = 0;
    bool ok = true;
    const unsigned long long key = in_range ? voxel_key_of(p.in[3 * i], p.in[3 * i + 1], p.in[3 * i + 2], p.voxel_size, ok, vx, vy, vz) : kEmptyVoxelKey;
    claim_voxel(p.keys, p.min_index, mask, key, ok, vx, vy, vz, i, p.error);
}

// pass 2: one thread per bucket; heads of clusters replay them; every thread counts its bucket for the compaction
static __global__ __launch_bounds__(256) void k_downsample_replay(const DownsampleParams p) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = ds_count(p), mask = ds_mask(p, n);
    bool occupied = false;
    if (n != 0u && s <= mask) {
        occupied = p.keys[s] != kEmptyVoxelKey;
        if (occupied && p.keys[(s - 1u) & mask] == kEmptyVoxelKey) {
            uint32_t len = 1u;
            while (p.keys[(s + len) & mask] != kEmptyVoxelKey) ++len;  // ends: at least half of the buckets are free
            const uint32_t probe = replay_cluster(p.keys, p.min_index, p.order, p.home_at, mask, s, len);
            if (probe >= 32u) atomicMax(p.probe_max, probe);  // (short probes are the rule: only the rare long one touches the counter)
        }
    }
    block_count_store(occupied, p.block_counts);
}
// pass 3: survivors in ascending bucket index (the reference's iteration order)
static __global__ __launch_bounds__(256) void k_downsample_gather(const DownsampleParams p, const uint32_t *block_counts, int raw, uint32_t *total, double *out) {
    __shared__ uint32_t s_wave[4];
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = ds_count(p), mask = ds_mask(p, n);
    const bool occupied = n != 0u && s <= mask && p.keys[s] != kEmptyVoxelKey;
    const unsigned long long ballot = __ballot(occupied);
    if (lane == 0) s_wave[wave] = static_cast<uint32_t>(__popcll(ballot));
    const uint32_t offset = block_offset(block_counts, raw, total);
    __syncthreads();
    if (!occupied) return;
    uint32_t pos = offset + static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
    const uint32_t i = p.order[s];
    out[3 * pos] = p.in[3 * i], out[3 * pos + 1] = p.in[3 * i + 1], out[3 * pos + 2] = p.in[3 * i + 2];
    // leave the bucket as the next call must find it (free slots were never written): the host clears the table only once
    p.keys[s] = kEmptyVoxelKey, p.min_index[s] = 0xFFFFFFFFu, p.order[s] = kFreeBucket, p.home_at[s] = 0xFFFFFFFFu;
}

// ---- the pre-steps of one frame in FIVE launches (round 6) ----------------------------------------------------------------
// pipeline/KinematicICP.cpp:54-62: Preprocess + transform_points, VoxelDownsample(0.5 vs), VoxelDownsample(1.5 vs).  The steps
// above as one chain were eight launches (preprocess, compact, 2 x {claim, replay, gather}) of 5-12 us each for a few MB of
// traffic: every one of them latency, not bandwidth (a dependent kernel boundary costs ~1.5 us, a kernel's fill and drain ~4).
// What really orders them are five grid-wide facts, and each launch below ends where the next such fact is needed:
//   k_frame_pre        point -> base frame, crop flag, tile counts; the survivor claims its voxel in table A
//                      [needs: nothing.  The table's size depends on the survivor count, which no workgroup knows yet: it is
//                       SPECULATED (f.spec_mask: what the previous frame had) and verified by the next launch]
//   k_frame_l1_replay  survivor count n0 (every workgroup adds the tile counts up itself) -> speculation right?; compaction into
//                      buffer 0; the clusters of table A replayed in the reference's insertion order; occupied-bucket counts
//                      [needs: all claims]
//   k_frame_l1_gather  n1; survivors of level 1 in table order -> buffer 1; each one claims its voxel in table B
//                      [needs: all replays, all counts]
//   k_frame_l2_replay  the clusters of table B                      [needs: all claims of level 2]
//   k_frame_l2_gather  n2; survivors of level 2 -> buffer 2; the LAST workgroup to finish hands the three counts to the host
//                      (tagged words in host memory the caller polls: no copy, no stream synchronisation)
// The claim uses the point's index in the raw frame instead of its position after the crop: the order is the same, which is all
// "first point of the voxel" and the replay's insertion order look at.  A wrong guess of the table size (the survivor count
// crossed a power of two since the last frame) is found by k_frame_l1_replay before anything depends on it: the later launches
// return at once and the host runs the unfused steps from buffer 0 on.  Results: those of the unfused chain, bit for bit.
// (store_through and the words of `misc` and `host_rec`: kicp_pre_shared.hpp)
struct DsTable {
    unsigned long long *keys;
    uint32_t *min_index, *order, *home_at;
};
// misc words of the chain (device): [1] range error (sticky until reported) [2] longest probe [3] ticket of the last launch
// [4] n0 [5] n1 [6] n2 [7] speculation failed [8] == seq: a claim of k_frame_pre gave up (table A too small for the frame)
struct FrameParams {
    PreprocessParams pre;  // block_counts: survivors per 256-point tile
    DsTable A, B;
    double voxel_a, voxel_b;
    uint32_t spec_mask;   // table A's mask (bucket count - 1) this chain assumes
    uint32_t tiles_pts;   // ceil(n / 256)
    uint32_t tiles_spec;  // 256-slot tiles of table A under spec_mask
    uint32_t *counts1, *counts2;  // occupied buckets per tile of table A / B
    uint32_t *misc;
    double *buf0, *buf1, *buf2;
    double *host_buf2;    // nullable: host-mapped pinned memory that receives buffer 2 as well (the registration source the pipeline returns)
    int32_t host_buf2_f32;  // 1: host_buf2 receives buffer 2 as x y z FLOAT32 records (kicp_pre_frame_f32) instead of doubles
    unsigned long long *host_rec;  // 5 words, each (seq << 32) | value: n0, n1, n2, longest probe, flags (1 range error, 2 speculation failed)
    uint32_t seq;
};
__device__ __forceinline__ uint32_t expected_mask(uint32_t n) {
    const uint32_t buckets = reference_bucket_count_u32(n);
    return buckets ? buckets - 1u : 0u;
}
// Every workgroup adds the per-tile counts up itself (a few loads per thread for the grids of a frame): offset = the tiles before
// `tile`, total = all `ntiles`.
__device__ __forceinline__ void tile_offset_total(const uint32_t *counts, uint32_t tile, uint32_t ntiles, uint32_t &offset, uint32_t &total) {
    __shared__ uint32_t s_before[4], s_all[4];
    uint32_t before = 0u, all = 0u;
    for (uint32_t i = threadIdx.x; i < ntiles; i += 256u) {
        const uint32_t c = counts[i];
        all += c, before += i < tile ? c : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64), all += __shfl_xor(all, off, 64);
    __syncthreads();  // (a caller that loops: the previous turn's readers are done)
    if ((threadIdx.x & 63) == 0) s_before[threadIdx.x >> 6] = before, s_all[threadIdx.x >> 6] = all;
    __syncthreads();
    offset = s_before[0] + s_before[1] + s_before[2] + s_before[3], total = s_all[0] + s_all[1] + s_all[2] + s_all[3];
}
// position of this thread's element among the workgroup's flagged ones, behind `offset` (all 256 threads call)
__device__ __forceinline__ uint32_t tile_position(bool flagged, uint32_t offset) {
    __shared__ uint32_t s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long ballot = __ballot(flagged);
    __syncthreads();
    if (lane == 0) s_wave[wave] = static_cast<uint32_t>(__popcll(ballot));
    __syncthreads();
    uint32_t pos = offset + static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
    return pos;
}

static __global__ __launch_bounds__(256) void k_frame_pre(const FrameParams f) {
    const PreprocessParams &p = f.pre;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) f.misc[2] = 0u, f.misc[3] = 0u, f.misc[7] = 0u, f.misc[9] = 0u;  // (raised / drawn / set by the launches behind this one)
    bool keep = false;
    double bx = 0.0, by = 0.0, bz = 0.0;
    if (i < p.n) {
        keep = preprocess_point(p, i, bx, by, bz);
        p.staged[3 * i] = bx, p.staged[3 * i + 1] = by, p.staged[3 * i + 2] = bz;
        p.flags[i] = keep ? 1u : 0u;
    }
    block_count_store(keep, p.block_counts);
    bool ok = true;
    int32_t vx = 0, vy = 0, vz = 0;
    const unsigned long long key = keep ? voxel_key_of(bx, by, bz, f.voxel_a, ok, vx, vy, vz) : kEmptyVoxelKey;
    claim_voxel(f.A.keys, f.A.min_index, f.spec_mask, key, ok, vx, vy, vz, i, f.misc + 1, f.misc + 8, f.seq);
}

// One 256-bucket tile of a claimed table: every cluster whose HEAD lies in the tile is put into the reference's order (replay_cluster's
// result, bit for bit) - with TWO round trips to memory instead of a chain of them.  The first version walked global memory: this
// bucket's key, then the one before it, then the ones behind it one by one, then replay_cluster's O(len^2) reloads of min_index and
// its read-modify-writes of order / home_at - 5 dependent accesses for a cluster of one, dozens for a cluster of four, each 2-4 us
// while the frame's push and the look-ahead decode load the memory system (the second-level replay: 10 us alone, 44 us in the drive).
// Here the tile's keys and input indices, kReplayHalo buckets behind it and the one before it are fetched at once into LDS; heads,
// lengths and the robin-hood replay work there (a cluster's LDS positions are its head thread's alone); the order goes back with one
// store per bucket.  home_at is not written (the gather resets it, nobody else reads it).  A cluster that leaves the window, and
// tables smaller than the window, take the global path.  Returns whether this thread's bucket is occupied.
constexpr uint32_t kReplayHalo = 32, kReplayWindow = 256 + kReplayHalo;
struct ReplayTile {
    unsigned long long key[kReplayWindow];
    uint32_t min[kReplayWindow], ord[kReplayWindow], home[kReplayWindow];
    uint32_t prev_occupied;
};
__device__ __forceinline__ bool replay_tile(const DsTable &T, uint32_t mask, uint32_t tile, ReplayTile &L, uint32_t *probe_max) {
    const uint32_t base = tile * 256u, i = threadIdx.x, s = base + i;
    if (mask + 1u < 2u * kReplayWindow) {  // (a small table: window positions would alias buckets)
        bool occupied = false;
        if (s <= mask) {
            occupied = T.keys[s] != kEmptyVoxelKey;
            if (occupied && T.keys[(s - 1u) & mask] == kEmptyVoxelKey) {
                uint32_t len = 1u;
                while (T.keys[(s + len) & mask] != kEmptyVoxelKey) ++len;  // ends: at least half of the buckets are free
                const uint32_t probe = replay_cluster(T.keys, T.min_index, T.order, T.home_at, mask, s, len);
                if (probe >= 32u) atomicMax(probe_max, probe);
            }
        }
        return occupied;
    }
    unsigned long long k = kEmptyVoxelKey, kh = kEmptyVoxelKey, kp = kEmptyVoxelKey;
    uint32_t m = 0xFFFFFFFFu, mh = 0xFFFFFFFFu;
    if (s <= mask) k = T.keys[s], m = T.min_index[s];
    if (i < kReplayHalo) kh = T.keys[(base + 256u + i) & mask], mh = T.min_index[(base + 256u + i) & mask];
    if (i == 255u) kp = T.keys[(base - 1u) & mask];
    __syncthreads();  // (a caller that loops over tiles: the previous tile's clusters are done with the window)
    L.key[i] = k, L.min[i] = m, L.ord[i] = kFreeBucket;
    if (i < kReplayHalo) L.key[256u + i] = kh, L.min[256u + i] = mh, L.ord[256u + i] = kFreeBucket;
    if (i == 255u) L.prev_occupied = kp != kEmptyVoxelKey ? 1u : 0u;
    __syncthreads();
    const bool occupied = k != kEmptyVoxelKey;
    const bool head = occupied && !(i ? L.key[i - 1u] != kEmptyVoxelKey : L.prev_occupied != 0u);
    if (!head) return occupied;
    uint32_t end = i + 1u;
    while (end < kReplayWindow && L.key[end] != kEmptyVoxelKey) ++end;
    uint32_t len = end - i;
    if (end == kReplayWindow) {  // the cluster leaves the window: the global walk (order / home_at of its buckets are still untouched)
        while (T.keys[(s + len) & mask] != kEmptyVoxelKey) ++len;
        const uint32_t probe = replay_cluster(T.keys, T.min_index, T.order, T.home_at, mask, s, len);
        if (probe >= 32u) atomicMax(probe_max, probe);
        return occupied;
    }
    if (len == 1u) {
        T.order[s] = m;
        return occupied;
    }
    // replay_cluster's result on window positions (kicp_table_order.hpp replay_window, CPU-tested against it): bucket (s + j) & mask <-> position i + j
    const uint32_t max_probe = replay_window(L.key, L.min, L.ord, L.home, i, end, s, mask);
    for (uint32_t j = i; j < end; ++j) T.order[(base + j) & mask] = L.ord[j];
    if (max_probe >= 32u) atomicMax(probe_max, max_probe);
    return occupied;
}

static __global__ __launch_bounds__(256) void k_frame_l1_replay(const FrameParams f) {
    const PreprocessParams &p = f.pre;
    // (this thread's point and its crop flag: fetched before the tile counts, not behind them - one round trip less)
    const uint32_t point = blockIdx.x * 256 + threadIdx.x;
    uint32_t flag = 0u;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (blockIdx.x < f.tiles_pts && point < p.n) flag = p.flags[point], sx = p.staged[3 * point], sy = p.staged[3 * point + 1], sz = p.staged[3 * point + 2];
    uint32_t offset, n0;
    tile_offset_total(p.block_counts, blockIdx.x, f.tiles_pts, offset, n0);
    const bool spec_ok = n0 == 0u || (expected_mask(n0) == f.spec_mask && f.misc[8] != f.seq);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        f.misc[4] = n0;
        if (!spec_ok) f.misc[7] = 1u;
    }
    if (blockIdx.x < f.tiles_pts) {  // order-preserving compaction of this tile's survivors: buffer 0, the frame the pipeline returns
        const bool keep = flag != 0u;
        const uint32_t pos = tile_position(keep, offset);
        if (keep) f.buf0[3 * pos] = sx, f.buf0[3 * pos + 1] = sy, f.buf0[3 * pos + 2] = sz;
    }
    if (!spec_ok || blockIdx.x >= f.tiles_spec) return;
    __shared__ ReplayTile s_tile;
    const bool occupied = n0 != 0u && replay_tile(f.A, f.spec_mask, blockIdx.x, s_tile, f.misc + 2);  // (n0: the same for every thread)
    block_count_store(occupied, f.counts1);
}

static __global__ __launch_bounds__(256) void k_frame_l1_gather(const FrameParams f) {
    // (the bucket's key and its place in the reference's order are fetched BEFORE the tile counts, not behind them: one round trip to
    //  memory less in a chain of five, each 2-8 us while the push and the look-ahead decode run)
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    unsigned long long bucket_key = kEmptyVoxelKey;
    uint32_t bucket_order = kFreeBucket;
    if (s <= f.spec_mask) bucket_key = f.A.keys[s], bucket_order = f.A.order[s];
    if (f.misc[7]) return;
    uint32_t offset, n1;
    tile_offset_total(f.counts1, blockIdx.x, f.tiles_spec, offset, n1);
    if (blockIdx.x == 0 && threadIdx.x == 0) f.misc[5] = n1;
    const bool occupied = f.misc[4] != 0u && bucket_key != kEmptyVoxelKey;
    const uint32_t pos = tile_position(occupied, offset);
    double x = 0.0, y = 0.0, z = 0.0;
    if (occupied) {
        const uint32_t i = bucket_order;
        x = f.pre.staged[3 * i], y = f.pre.staged[3 * i + 1], z = f.pre.staged[3 * i + 2];
        f.buf1[3 * pos] = x, f.buf1[3 * pos + 1] = y, f.buf1[3 * pos + 2] = z;
        // leave the bucket as the next frame must find it (free slots were never written)
        f.A.keys[s] = kEmptyVoxelKey, f.A.min_index[s] = 0xFFFFFFFFu, f.A.order[s] = kFreeBucket, f.A.home_at[s] = 0xFFFFFFFFu;
    }
    bool ok = true;
    int32_t vx = 0, vy = 0, vz = 0;
    const unsigned long long key = occupied ? voxel_key_of(x, y, z, f.voxel_b, ok, vx, vy, vz) : kEmptyVoxelKey;
    claim_voxel(f.B.keys, f.B.min_index, expected_mask(n1), key, ok, vx, vy, vz, pos, f.misc + 1);
}

// (table B's size is known on the device only: the launch covers an upper bound and walks the tiles there are)
static __global__ __launch_bounds__(256) void k_frame_l2_replay(const FrameParams f) {
    if (f.misc[7]) return;
    const uint32_t n1 = f.misc[5], mask = expected_mask(n1), tiles = n1 ? (mask >> 8) + 1u : 0u;
    __shared__ ReplayTile s_tile;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const bool occupied = replay_tile(f.B, mask, t, s_tile, f.misc + 2);
        block_count_store_at(occupied, f.counts2 + t);
    }
}

static __global__ __launch_bounds__(256) void k_frame_l2_gather(const FrameParams f) {
    __shared__ uint32_t s_last;
    const unsigned long long tag = static_cast<unsigned long long>(f.seq) << 32;
    auto publish = [&](int word, uint32_t v) { __hip_atomic_store(f.host_rec + word, tag | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    // (the first tile's bucket and its place in the order: fetched before anything that depends on the counts - k_frame_l1_gather;
    //  table B is never larger than table A, whose size the launch knows)
    unsigned long long first_key = kEmptyVoxelKey;
    uint32_t first_order = kFreeBucket;
    if (blockIdx.x * 256u + threadIdx.x <= f.spec_mask) first_key = f.B.keys[blockIdx.x * 256u + threadIdx.x], first_order = f.B.order[blockIdx.x * 256u + threadIdx.x];
    if (f.misc[7]) {  // the table-size guess was wrong: nothing behind buffer 0 was done; the host takes the unfused steps from there
        if (blockIdx.x == 0 && threadIdx.x == 0) publish(0, f.misc[4]), publish(1, 0u), publish(2, 0u), publish(3, 0u), publish(4, 2u | (f.misc[1] ? 1u : 0u));
        return;
    }
    const uint32_t n1 = f.misc[5], mask = expected_mask(n1), tiles = n1 ? (mask >> 8) + 1u : 0u;
    uint32_t n2_seen = 0xFFFFFFFFu;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t offset, n2;
        const uint32_t s = t * 256 + threadIdx.x;
        const bool mine = t == blockIdx.x;  // (this workgroup's first tile: fetched at the top of the kernel)
        const unsigned long long bucket_key = mine ? first_key : (s <= mask ? f.B.keys[s] : kEmptyVoxelKey);
        const uint32_t bucket_order = mine ? first_order : (s <= mask ? f.B.order[s] : kFreeBucket);
        tile_offset_total(f.counts2, t, tiles, offset, n2);
        n2_seen = n2;
        const bool occupied = s <= mask && bucket_key != kEmptyVoxelKey;
        const uint32_t pos = tile_position(occupied, offset);
        if (occupied) {
            const uint32_t i = bucket_order;
            const double x = f.buf1[3 * i], y = f.buf1[3 * i + 1], z = f.buf1[3 * i + 2];
            store_through(f.buf2 + 3 * pos, x), store_through(f.buf2 + 3 * pos + 1, y), store_through(f.buf2 + 3 * pos + 2, z);
            f.B.keys[s] = kEmptyVoxelKey, f.B.min_index[s] = 0xFFFFFFFFu, f.B.order[s] = kFreeBucket, f.B.home_at[s] = 0xFFFFFFFFu;
        }
    }
    // The workgroup that finishes LAST tells the host (which polls the record instead of synchronising the stream).  Buffer 2 goes
    // to a kernel on another queue next: its stores went through to memory (store_through) and every wave waits for them, then the
    // workgroup draws its ticket.  (The copy of buffer 2 in host memory is k_frame_src_host's: written here, its PCIe writes queued
    // up behind the frame push's and a system-scope release held the record back by ~10 us.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        s_last = __hip_atomic_fetch_add(f.misc + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    uint32_t offset, n2 = n2_seen;
    if (n2_seen == 0xFFFFFFFFu) tile_offset_total(f.counts2, 0u, tiles, offset, n2);  // (a workgroup without a tile of its own; n2_seen: the same for every thread)
    if (threadIdx.x == 0) {
        f.misc[6] = n2;
        publish(0, f.misc[4]), publish(1, n1), publish(2, n2), publish(3, f.misc[2]), publish(4, f.misc[1] ? 1u : 0u);
    }
}

// Buffer 2 - the registration source, ~1 300 points, the second cloud RegisterFrame returns - into host memory: a launch of its own
// behind the chain, announced by word 5 of the host record ((seq << 32) | points), which only kicp_pre_download(2) waits for.
// misc[9]: its ticket (reset by k_frame_pre).
static __global__ __launch_bounds__(256) void k_frame_src_host(const FrameParams f) {
    __shared__ uint32_t s_last;
    if (f.misc[7]) return;  // (the guess was wrong: the host takes the unfused steps and downloads buffer 2 itself)
    const uint32_t n2 = f.misc[6];
    if (f.host_buf2_f32) {  // (the published keypoints' PointCloud2 records: static_cast<float>, RosUtils.cpp:40-63)
        float *out = reinterpret_cast<float *>(f.host_buf2);
        for (uint32_t o = blockIdx.x * 256u + threadIdx.x; o < 3u * n2; o += gridDim.x * 256u) out[o] = static_cast<float>(f.buf2[o]);
    } else {
        for (uint32_t o = blockIdx.x * 256u + threadIdx.x; o < 3u * n2; o += gridDim.x * 256u) f.host_buf2[o] = f.buf2[o];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        // system scope: this workgroup's bytes are in host memory before its ticket - and so before the flag, whoever writes it
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = __hip_atomic_fetch_add(f.misc + 9, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
        if (s_last) __hip_atomic_store(f.host_rec + 5, (static_cast<unsigned long long>(f.seq) << 32) | n2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// (round 6 tried the second level in ONE workgroup - replay, ballot bitmap + scan in LDS, gather, as a fourth and last launch: its chains
//  of dependent loads - cluster walk, order -> point -> store - take as long on one CU as the two launches do on thirty, 100 vs 140 us
//  per frame with a contiguous bucket range per thread, no gain with coalesced rows; removed.)

}  // namespace kicp
