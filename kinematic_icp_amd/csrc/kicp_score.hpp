// kicp_score.hpp -- k_score_poses: DataAssociation (Registration.cpp:62-81) of ONE frame at MANY poses in one launch.
//
// Per pose two numbers leave the device: how many source points found a correspondence within max_correspondence_distance, and
// the sum of their squared residuals |T s - nn|^2 - sums [6] and [5] of a pass kernel at that pose, bit for bit: the search, the
// exact fp64 resolution, the first-minimum tie rule and the acceptance test ARE the pass kernels' (gather32_pass ->
// resolve_and_accumulate, instantiated with ScoreAcc: kicp_kernels.hpp), the term is formed by the same expression on the same
// transformed point, rounded once by the same to_fixed and added as an integer.  What a pass kernel computes beyond that - the
// pose's basis, five more terms per correspondence, 28-limb rows, the hand-off to a waiting host - is not here.
//
// Decomposition: the work is the grid (tile of 256 source points) x (pose), numbered tile-major (item = tile * count + pose), so a
// workgroup that strides over the items stays on one tile of the frame while it walks the poses: the tile's source points are L1 /
// L2 hits from the second pose on, and poses that are neighbours in the caller's grid read neighbouring voxels of the map.  One
// thread per query, the four-waves register budget (with thousands of poses the device is full: the latency builds have nothing to
// offer), idle lanes take over voxels of loaded queries exactly as in the generic pass kernel.
//
// Reduction: a lane holds at most one correspondence per item - four 21-bit limbs and a flag.  Wave sums in int32 (DPP), the four
// waves through LDS, then ONE 64-bit integer atomic per workgroup, pose and word into the pose's accumulator row (relaxed, agent
// scope; no floating-point atomics anywhere).  Integer sums: the result cannot depend on how the items are cut into workgroups or
// launches.  A workgroup whose tile found nothing at a pose (most tiles of a wrong hypothesis) sends nothing.
#pragma once
#include "kicp_kernels.hpp"

namespace kicp {

constexpr int kScoreBlock = 256;
// a pose's accumulator row (64 bytes): the four limb sums of sum ||r||^2 (limb k at 2^(21 k), each < n 2^21), the count, padding.
// (A term beyond to_fixed's range adds zero and counts, as in the pass kernels; kicp_pass_sums does not report it either.)
constexpr int kScoreWords = 8;
constexpr int kScoreCountWord = kTermLimbs, kScoreUsedWords = kTermLimbs + 1;

struct ScoreParams {
    PassParams pass;               // src, n, map, tau, search; everything else unused (zero)
    const double *poses;           // device [count][7]: qx qy qz qw tx ty tz
    unsigned long long *acc;       // device [count][kScoreWords], zero before the first launch of a call
    uint32_t count;                // poses
    unsigned long long item0, items;  // this launch's share of the tiles x count items
};
static_assert(offsetof(ScoreParams, pass) == 0, "args_at_point_of_use reads the PassParams at offset 0 of the kernarg segment");

static __global__ __launch_bounds__(kScoreBlock, 4) void k_score_poses(const ScoreParams sp) {
    constexpr int kWaves = kScoreBlock / 64;
    __shared__ int s_lend[kWaves][kLendWords];
    __shared__ double s_park[kScoreBlock * kParkWords];
    __shared__ int s_sum[2][kWaves][kScoreUsedWords];  // two sets, alternating: one barrier per item
    const PassParams &p = sp.pass;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t set = 0u;
    for (unsigned long long e = blockIdx.x; e < sp.items; e += gridDim.x, set ^= 1u) {  // (the same trip count for every lane of the workgroup)
        const unsigned long long item = sp.item0 + e;
        const uint32_t tile = static_cast<uint32_t>(item / sp.count), k = static_cast<uint32_t>(item % sp.count);
        const double *__restrict__ pq = sp.poses + static_cast<size_t>(k) * 7;
        const Pose T{uniform_d(pq[0]), uniform_d(pq[1]), uniform_d(pq[2]), uniform_d(pq[3]), uniform_d(pq[4]), uniform_d(pq[5]), uniform_d(pq[6])};
        ScoreAcc acc{};
        gather32_pass<false, kScoreBlock, 1, false, false, true, false, ScoreAcc>(p, T, threadIdx.x, acc, p.src, p.n, tile, &s_lend[wave][0], s_park);
        const int hits = __popcll(__ballot(acc.hit != 0));
        int limb[kTermLimbs];
#pragma unroll
        for (int j = 0; j < kTermLimbs; ++j) limb[j] = hits ? wave_sum_to_lane63(acc.limb[j]) : 0;  // (wave-uniform branch; 64 limbs of 21 bits: int32)
        if (lane == 63) {
#pragma unroll
            for (int j = 0; j < kTermLimbs; ++j) s_sum[set][wave][j] = limb[j];
            s_sum[set][wave][kScoreCountWord] = hits;
        }
        __syncthreads();
        if (threadIdx.x < kScoreUsedWords) {
            long long v = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) v += s_sum[set][w][threadIdx.x];
            if (v != 0)
                __hip_atomic_fetch_add(sp.acc + static_cast<size_t>(k) * kScoreWords + threadIdx.x, static_cast<unsigned long long>(v), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace kicp
