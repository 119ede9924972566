// kicp_arcs.hpp -- the kernel that scores a fan of arc trajectories on the grid's plan (kicp_grid_score_arcs; C-ABI: kicp_grid_arcs.hip,
// arithmetic: kicp_arcs_host.hpp).  One launch on the grid's stream:
//   k_arcs_score  one wave per arc, four arcs per 256-lane workgroup.  Every lane rolls the arc's poses forward by the same recurrence
//                 (wave-uniform: a dozen fp64 operations a step, no lane waits for another), the lanes stride over the footprint's
//                 samples at each pose, a collision is a ballot, the pose's largest weight a butterfly of shuffles.  The step loop
//                 leaves at the first colliding pose - the ballot makes the branch wave-uniform.  Lane 0 stores the arc's four words
//                 with one 16-byte store.
// The weight bytes are gathers within a few metres of the robot and are left to L1 / L2; the footprint (two doubles a sample, read by
// every wave at every pose) likewise.  No LDS, no atomics, no workgroup barrier: the four waves of a workgroup share nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_arcs_host.hpp"

namespace kicp {

constexpr uint32_t kArcsBlock = 256, kArcsWave = 64, kArcsPerBlock = kArcsBlock / kArcsWave;

// arcs: n_arcs x 4 doubles; footprint_xy: n_samples x 2; out: n_arcs x 4 words, 16-byte aligned
static __global__ __launch_bounds__(kArcsBlock) void k_arcs_score(const uint8_t *__restrict__ q, const uint32_t *__restrict__ potential, ArcGeom g, ArcPose start,
                                                                  const double *__restrict__ arcs, uint32_t n_arcs, uint32_t n_steps,
                                                                  const double *__restrict__ footprint_xy, uint32_t n_samples, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x % kArcsWave, k = blockIdx.x * kArcsPerBlock + threadIdx.x / kArcsWave;
    if (k >= n_arcs) return;  // (a whole wave)
    uint32_t r[4];
    arc_score(g, potential, start, arcs + 4 * static_cast<size_t>(k), n_steps,
              [&](const ArcPose &p) {
                  uint32_t largest;
                  const bool collides = arc_pose_part(g, q, p, footprint_xy, n_samples, lane, kArcsWave, largest);
                  if (__ballot(collides) != 0ull) return 0u;
                  for (int o = 32; o > 0; o >>= 1) {
                      const uint32_t other = __shfl_xor(largest, o);
                      largest = other > largest ? other : largest;
                  }
                  return largest;
              },
              r);
    if (lane == 0u) reinterpret_cast<uint4 *>(out)[k] = make_uint4(r[0], r[1], r[2], r[3]);
}

}  // namespace kicp
