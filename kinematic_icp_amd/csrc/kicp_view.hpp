// kicp_view.hpp -- the kernels of the depth view and of the map sweep that reads it (kicp_view_*, kicp_map_remove_seen_through; C-ABI:
// kicp_view.hip, geometry and verdict: kicp_view_host.hpp).
//
// The image is 6 res^2 floats kept as their bit patterns (positive floats order like their bits):
//   k_view_render    one lane per frame point: transform, face, pixel, atomicMin of (float)m on the pixel's word; the image was filled
//                    with +inf beforehand.  A minimum over a SET: the result depends neither on the points' order nor on launch shape
//   k_view_classify  one lane per world point: the verdict as a byte
// The sweep is two launches on the map's stream:
//   k_view_list      over the packed-key side array, as k_up_remove walks it: every occupied voxel whose box can hold an in-range
//                    point is appended to a list (one atomic per wave and trip of 256 slots).  The cull - the Chebyshev distance from the
//                    sensor to the voxel's box, widened by a thousandth of a voxel on every side, against max_ray - only leaves
//                    voxels out whose points are all out of range, which the verdict would keep and not count anyway
//   k_view_sweep     one WAVE per listed voxel (launched for the host's voxel count, an upper bound of the list's length; the waves
//                    beyond the list leave): lanes take the points k = lane, lane + 64, ..; each forms its verdict - the window's
//                    loads are independent - and the survivors of a 64-point trip are compacted in order with a ballot and a prefix
//                    popcount.  A wave executes a trip's loads before its stores, and a trip only writes positions at or below its own,
//                    so no point is overwritten before it was read.  The fp64 pool and the 16-bit mirror move alike, the mirror's
//                    freed tail is marked empty, val gets the new count, and a voxel left empty is erased as k_up_remove erases one,
//                    one neighbour per lane
// Statistics are summed per wave and added with one atomic per wave and counter, the sweep's into one of kSweepShards sets that the
// host sums.  No kernel uses LDS or scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_devmap.hpp"  // DevMap, dev_find: all the view needs of the map's device code, and no kernel comes with it
#include "kicp_view_host.hpp"

namespace kicp {

constexpr uint32_t kViewBlock = 256;
constexpr int kSweepWaves = 4;  // voxels per workgroup of k_view_sweep
// The sweep's four statistics are kept kSweepShards times, a workgroup adding to the set blockIdx.x % kSweepShards, and summed by the
// host: tens of thousands of waves adding to ONE word serialise on it
constexpr uint32_t kSweepShards = 64;

// stats[0] += points used (the host derives the skipped ones)
static __global__ __launch_bounds__(kViewBlock) void k_view_render(const double *__restrict__ xyz, uint32_t n, ViewGeom g, ViewFrame f, uint32_t *__restrict__ depth,
                                                                   unsigned int *__restrict__ stats) {
    const uint32_t i = blockIdx.x * kViewBlock + threadIdx.x;
    bool used = false;
    if (i < n) {
        size_t pixel;
        uint32_t bits;
        used = view_render_point(g, f, xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2], pixel, bits);
        if (used) atomicMin(&depth[pixel], bits);
    }
    const unsigned long long b = __ballot(used);
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&stats[0], static_cast<unsigned int>(__popcll(b)));
}

static __global__ __launch_bounds__(kViewBlock) void k_view_classify(const double *__restrict__ xyz, uint32_t n, ViewGeom g, ViewFrame f,
                                                                     const uint32_t *__restrict__ depth, uint8_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * kViewBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = view_verdict(g, f, depth, xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2]);
}

// can the voxel (x, y, z) hold a point within max_ray (Chebyshev) of the sensor?  Conservative: the box is widened, a NaN sensor
// answers yes (the verdict then finds every point out of range)
__device__ __forceinline__ bool view_voxel_in_reach(const ViewGeom &g, const ViewFrame &f, double vs, int32_t x, int32_t y, int32_t z) {
    const double reach = g.max_ray + 0.001 * vs;
    const double c[3] = {f.cx, f.cy, f.cz};
    const int32_t v[3] = {x, y, z};
    bool out_of_reach = false;
    for (int a = 0; a < 3; ++a) {
        const double lo = (static_cast<double>(v[a]) - 0.001) * vs, hi = (static_cast<double>(v[a]) + 1.001) * vs;
        out_of_reach = out_of_reach || lo - c[a] > reach || c[a] - hi > reach;
    }
    return !out_of_reach;
}

// list[0 .. *n_list) = the slots of the occupied voxels within reach (room for every occupied voxel)
static __global__ __launch_bounds__(kViewBlock) void k_view_list(const DevMap m, ViewGeom g, ViewFrame f, uint32_t *__restrict__ list, unsigned int *__restrict__ n_list) {
    const uint32_t slots = m.mask + 1;
    const ulonglong2 *keys2 = reinterpret_cast<const ulonglong2 *>(m.keys64);
    const uint32_t lane = threadIdx.x & 63u;
    // (slots is a power of two >= 1024: slots / 4 is a multiple of the workgroup, so the lanes of a wave make the same trips)
    for (uint32_t q = blockIdx.x * kViewBlock + threadIdx.x; q < slots / 4; q += gridDim.x * kViewBlock) {
        const ulonglong2 ka = keys2[2 * q], kb = keys2[2 * q + 1];
        const unsigned long long key[4] = {ka.x, ka.y, kb.x, kb.y};
        bool want[4];
        unsigned long long b[4];
        uint32_t total = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            want[u] = false;
            if (key[u] != kEmptyKey64) {
                const Slot &e = m.table[4 * q + u];
                const uint32_t val = e.val;
                want[u] = val != kEmptyVal && val_count(val, m.cbits) != 0u && view_voxel_in_reach(g, f, m.voxel_size, e.x, e.y, e.z);
            }
            b[u] = __ballot(want[u]);
            total += static_cast<uint32_t>(__popcll(b[u]));
        }
        if (total == 0u) continue;  // (wave-uniform)
        uint32_t base = 0;
        if (lane == 0u) base = atomicAdd(n_list, total);  // one add per wave and trip, whatever the four columns hold
        base = __shfl(base, 0, 64);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (want[u]) list[base + static_cast<uint32_t>(__popcll(b[u] & ((1ull << lane) - 1ull)))] = 4 * q + u;
            base += static_cast<uint32_t>(__popcll(b[u]));
        }
    }
}

__device__ __forceinline__ uint32_t view_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// stats: kSweepShards sets of: points in range, points removed, voxels that lost at least one point, voxels erased
static __global__ __launch_bounds__(64 * kSweepWaves) void k_view_sweep(const DevMap m, ViewGeom g, ViewFrame f, const uint32_t *__restrict__ depth,
                                                                        const uint32_t *__restrict__ list, const unsigned int *__restrict__ n_list,
                                                                        unsigned int *__restrict__ all_stats) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned int *stats = all_stats + 4u * (blockIdx.x % kSweepShards);
    const uint32_t t = blockIdx.x * kSweepWaves + (threadIdx.x >> 6);
    if (t >= *n_list) return;  // (wave-uniform)
    const uint32_t h = list[t];
    Slot &e = m.table[h];
    const uint32_t val = e.val;
    const uint32_t count = val_count(val, m.cbits), bucket = val_bucket(val, m.cbits);
    double *b = m.pool + static_cast<size_t>(bucket) * m.cap * 3;
    MirrorPoint *b16 = m.pool16 + static_cast<size_t>(bucket) * mirror_stride(m.cap);
    uint32_t kept = 0, in_range = 0;
    for (uint32_t k0 = 0; k0 < count; k0 += 64u) {  // (count is wave-uniform)
        const uint32_t k = k0 + lane;
        const bool have = k < count;
        double px = 0.0, py = 0.0, pz = 0.0;
        MirrorPoint mp = mirror_empty();
        uint8_t verdict = 0u;
        if (have) {
            px = b[3 * k], py = b[3 * k + 1], pz = b[3 * k + 2], mp = b16[k];
            verdict = view_verdict(g, f, depth, px, py, pz);
        }
        in_range += (verdict & kViewInRange) ? 1u : 0u;
        const bool keep = have && !(verdict & kViewSeenThrough);
        const unsigned long long keeps = __ballot(keep);
        const uint32_t at = kept + static_cast<uint32_t>(__popcll(keeps & ((1ull << lane) - 1ull)));
        if (keep && at != k) b[3 * at] = px, b[3 * at + 1] = py, b[3 * at + 2] = pz, b16[at] = mp;
        kept += static_cast<uint32_t>(__popcll(keeps));
    }
    in_range = view_wave_sum(in_range);
    if (lane == 0u && in_range) atomicAdd(&stats[0], in_range);
    if (kept == count) return;
    for (uint32_t k = kept + lane; k < count; k += 64u) b16[k] = mirror_empty();
    if (lane == 0u) {
        atomicAdd(&stats[1], count - kept);
        atomicAdd(&stats[2], 1u);
        atomicAdd(&m.ctr->n_points, ~static_cast<unsigned long long>(count - kept) + 1ull);
        if (kept) {
            e.val = make_val(bucket, kept, m.cbits);
        } else {
            e.val = halo_val(m.cbits);
            m.free_list[atomicAdd(&m.ctr->free_count, 1u)] = bucket;
            atomicSub(&m.ctr->n_voxels, 1u);
            atomicAdd(&stats[3], 1u);
        }
    }
    if (kept == 0u && lane < 27u) {  // erased: the 27 voxels that see this one forget it (U + shift[s] == this  <=>  U = this - shift[s])
        const int s = static_cast<int>(lane);
        const uint32_t w = dev_find(m, e.x - shift_component(kShiftX, s), e.y - shift_component(kShiftY, s), e.z - shift_component(kShiftZ, s));
        if (w != kNoSlot) atomicAnd(&m.table[w].nbr, ~(1u << s));
    }
}

}  // namespace kicp
