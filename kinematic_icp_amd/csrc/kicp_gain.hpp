// kicp_gain.hpp -- the kernels of the grid's information gain (kicp_grid_gain; C-ABI: kicp_grid_explore.hip, arithmetic: kicp_gain_host.hpp):
// what a sensor of R cells' range would see of the unknown cells from each candidate viewpoint.  Two launches on the grid's stream:
//   k_gain_classes  one lane per cell: the class of the cell from its counters (grid_readout, clear_class), one byte.  Once per call:
//                   the ray kernel then pays one byte load per visit instead of a readout's division, and neighbouring viewpoints
//                   share the plane through L2.
//   k_gain_rays     one 256-lane workgroup per viewpoint.  The bit plane of the viewpoint's (2 R + 1)^2 window lies in dynamic LDS
//                   behind four words of sums (16 + 4 ceil((2 R + 1)^2 / 32) bytes: 65 360 at R = 361, within the 64 KiB a launch
//                   gets without an attribute) and is zeroed first.  Each wave takes the rays wave, wave + 4, ..; its 64 lanes take the
//                   steps k = 1 + lane + 64 t of that ONE ray (k_grid_rays' mapping: the walk is in closed form, so every lane knows
//                   its cell without the steps before it, and the 64 byte loads are independent).  A ballot of "the ray ends at my
//                   step" finds the first ending lane; the lanes below it whose cell is UNKNOWN set their bit with an LDS atomicOr -
//                   bits share words and rays share cells, so a plain store will not do - and the first ending lane's reason bumps
//                   the wave's BLOCKED or LEFT count.  A non-zero ballot ends the ray's trips.  After a barrier the lanes count the
//                   plane's bits, the waves add their sums in LDS and one lane stores the row.
// A viewpoint that is not CLEAR leaves before the first barrier - the whole workgroup reads the same byte - with words 0 .. 2 zero.
// Nothing waits on another workgroup: there is no persistent kernel, no grid-wide barrier and no spin.  No scratch.
// For R well below 64 most lanes of a wave idle in the walk (R = 20: 20 of 64); rays are not packed into sub-wave groups - the bench
// (tools/bench_gain.py) has the small-R case.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_gain_host.hpp"

namespace kicp {

constexpr uint32_t kGainBlock = 256;
constexpr uint32_t kGainSumWords = 4;  // in front of the plane: SEEN, BLOCKED, LEFT and a word that keeps the plane 16-byte aligned
static_assert((kGainSumWords + (2u * kGainMaxRange + 1u) * (2u * kGainMaxRange + 1u) / 32u + 1u) * 4u <= 65536u, "the plane of the largest window fits 64 KiB of LDS");

inline size_t gain_lds_bytes(uint32_t R) { return (static_cast<size_t>(kGainSumWords) + gain_plane_words(R)) * sizeof(uint32_t); }

static __global__ __launch_bounds__(kGainBlock) void k_gain_classes(const uint16_t *__restrict__ counts, uint32_t cells, uint32_t min_observations, int32_t source_min,
                                                                    uint8_t *__restrict__ classes) {
    const uint32_t c = blockIdx.x * kGainBlock + threadIdx.x;
    if (c >= cells) return;
    const uint32_t pair = reinterpret_cast<const uint32_t *>(counts)[c];
    classes[c] = static_cast<uint8_t>(clear_class(grid_readout(pair & 0xFFFFu, pair >> 16, min_observations), source_min));
}

// views[blockIdx.x] < width * height (the entry has checked every one); out: gridDim.x rows of kGainWords
static __global__ __launch_bounds__(kGainBlock) void k_gain_rays(const uint8_t *__restrict__ classes, uint32_t width, uint32_t height, uint32_t R,
                                                                 const uint32_t *__restrict__ views, uint32_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_gain[];
    uint32_t *sums = s_gain, *plane = s_gain + kGainSumWords;
    const uint32_t view = views[blockIdx.x], view_class = classes[view];
    uint32_t *row = out + static_cast<size_t>(blockIdx.x) * kGainWords;
    if (view_class != kClearClear) {  // the same for every lane of the workgroup
        if (threadIdx.x == 0u) gain_row(row, 0u, 0u, 0u, view_class);
        return;
    }
    const uint32_t words = gain_plane_words(R);
    for (uint32_t i = threadIdx.x; i < words; i += kGainBlock) plane[i] = 0u;
    if (threadIdx.x < kGainSumWords) sums[threadIdx.x] = 0u;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u, vx = view % width, vy = view / width;
    auto class_of = [classes](size_t cell) { return static_cast<uint32_t>(classes[cell]); };
    uint32_t blocked = 0, left = 0;  // the same in every lane of a wave
    for (uint32_t ray = threadIdx.x / 64u; ray < gain_rays(R); ray += kGainBlock / 64u) {
        int32_t dx, dy;
        gain_ray(R, ray, dx, dy);
        for (uint32_t k0 = 1u; k0 <= R; k0 += 64u) {
            const uint32_t k = k0 + lane;
            uint32_t bit = 0, verdict = kGainOn;  // a lane past the ray's last step neither sees nor ends anything
            if (k <= R) verdict = gain_step(dx, dy, R, k, vx, vy, width, height, class_of, bit);
            const unsigned long long ends = __ballot(gain_ends(verdict));
            const uint32_t first = ends ? static_cast<uint32_t>(__ffsll(static_cast<long long>(ends))) - 1u : 64u;
            if (verdict == kGainSeen && lane < first) atomicOr(&plane[bit >> 5], 1u << (bit & 31u));
            if (ends) {
                const uint32_t reason = __shfl(verdict, static_cast<int>(first), 64);
                blocked += reason == kGainEndBlocked ? 1u : 0u, left += reason == kGainEndLeft ? 1u : 0u;
                break;
            }
        }
    }
    if (lane == 0u) {
        if (blocked) atomicAdd(&sums[1], blocked);
        if (left) atomicAdd(&sums[2], left);
    }
    __syncthreads();
    uint32_t seen = 0;
    for (uint32_t i = threadIdx.x; i < words; i += kGainBlock) seen += static_cast<uint32_t>(__popc(plane[i]));
    for (int o = 32; o > 0; o >>= 1) seen += __shfl_xor(seen, o, 64);
    if (lane == 0u && seen) atomicAdd(&sums[0], seen);
    __syncthreads();
    if (threadIdx.x == 0u) gain_row(row, sums[0], sums[1], sums[2], view_class);
}

}  // namespace kicp
