// kicp_planar.hpp -- k_planar_poses: the sums of a planar 3-DoF Gauss-Newton step of ONE frame at MANY poses in one launch.
//
// Per accepted correspondence (s = source point, r = T s - nn, c0 = R UnitX, c1 = R UnitY) the Jacobian of a step that is free in the
// plane of the body frame is J = [c0 | c1 | R (-s.y, s.x, 0)], so with R orthogonal
//   J^T J = [ 1     0    -s.y          ]      J^T r = [ a = c0 . r    ]
//           [ 0     1     s.x          ]              [ b = c1 . r    ]
//           [-s.y   s.x   s.x^2 + s.y^2]              [ s.x b - s.y a ]
// and seven sums besides the count describe the step: sum s.x, sum -s.y, sum (s.x^2 + s.y^2), sum a, sum b, sum (s.x b - s.y a) and
// sum |r|^2.  Five of them are terms of a registration pass and come out of the pass kernels' own function (correspondence_terms, via
// gather32_pass -> resolve_and_accumulate instantiated with PlanarAcc: kicp_kernels.hpp) - the same doubles, rounded once by the same
// to_fixed and added as integers, so they equal kicp_pass_sums at that pose bit for bit; s.x and b are added next to them.
//
// Decomposition and reduction are k_score_poses' (kicp_score.hpp): items = (tile of 256 source points) x (pose), tile-major, a
// workgroup strides over the items, the pose is wave-uniform; per limb a wave sum in int32 (skipped for a wave without hits), the four
// waves through LDS, then ONE relaxed agent-scope 64-bit integer atomic per workgroup, pose and non-zero word into the pose's row.
// Integer sums: a pose's row cannot depend on which other poses share its launch, nor on how the items are cut into launches.
#pragma once
#include "kicp_kernels.hpp"
#include "kicp_score.hpp"

namespace kicp {

// a pose's accumulator row (256 bytes): 7 terms x 4 limb sums (limb k at 2^(21 k)) in PlanarAcc's order, the count, padding
constexpr int kPlanarLimbWords = kTermLimbs * kPlanarTerms;
constexpr int kPlanarCountWord = kPlanarLimbWords, kPlanarUsedWords = kPlanarLimbWords + 1;
constexpr int kPlanarWords = 32;
static_assert(kPlanarUsedWords <= kPlanarWords && kPlanarUsedWords <= 64, "one lane of the first wave per word of the row");

// (ScoreParams: `acc` is [count][kPlanarWords] here)
// Register budget: PlanarAcc is as large as a pass kernel's Acc, but seven terms are converted instead of five, and under the
// four-waves bound (128 VGPRs) the compiler spills 5 VGPRs to 24 bytes of scratch per lane.  Bound to three waves per SIMD it takes
// 137 VGPRs, no scratch and no VGPR spill: taken, rather than scratch traffic in the exact phase.
static __global__ __launch_bounds__(kScoreBlock, 3) void k_planar_poses(const ScoreParams sp) {
    constexpr int kWaves = kScoreBlock / 64;
    __shared__ int s_lend[kWaves][kLendWords];
    __shared__ double s_park[kScoreBlock * kParkWords];
    __shared__ int s_sum[2][kWaves][kPlanarUsedWords];  // two sets, alternating: one barrier per item
    const PassParams &p = sp.pass;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t set = 0u;
    for (unsigned long long e = blockIdx.x; e < sp.items; e += gridDim.x, set ^= 1u) {  // (the same trip count for every lane of the workgroup)
        const unsigned long long item = sp.item0 + e;
        const uint32_t tile = static_cast<uint32_t>(item / sp.count), k = static_cast<uint32_t>(item % sp.count);
        const double *__restrict__ pq = sp.poses + static_cast<size_t>(k) * 7;
        const Pose T{uniform_d(pq[0]), uniform_d(pq[1]), uniform_d(pq[2]), uniform_d(pq[3]), uniform_d(pq[4]), uniform_d(pq[5]), uniform_d(pq[6])};
        PlanarAcc acc{};
        gather32_pass<false, kScoreBlock, 1, false, false, true, false, PlanarAcc>(p, T, threadIdx.x, acc, p.src, p.n, tile, &s_lend[wave][0], s_park);
        const int hits = __popcll(__ballot(acc.hit != 0));
        if (hits) {  // (wave-uniform branch; 64 limbs of 21 bits: int32)
#pragma unroll
            for (int j = 0; j < kPlanarLimbWords; ++j) {
                const int v = wave_sum_to_lane63(acc.limb[j]);
                if (lane == 63) s_sum[set][wave][j] = v;
            }
        } else if (lane < kPlanarLimbWords) {
            s_sum[set][wave][lane] = 0;
        }
        if (lane == 63) s_sum[set][wave][kPlanarCountWord] = hits;
        __syncthreads();
        if (threadIdx.x < kPlanarUsedWords) {
            long long v = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) v += s_sum[set][w][threadIdx.x];
            if (v != 0)
                __hip_atomic_fetch_add(sp.acc + static_cast<size_t>(k) * kPlanarWords + threadIdx.x, static_cast<unsigned long long>(v), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace kicp
