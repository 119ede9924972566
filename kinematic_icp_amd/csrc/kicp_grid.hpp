// kicp_grid.hpp -- the kernels of the 2-D occupancy grid (kicp_grid_*; C-ABI: kicp_grid.hip, geometry: kicp_grid_host.hpp).
//
// A frame touches only the window, the (2 reach + 1)^2 cells around the sensor's cell.  Two frame-local byte planes lie over it, one
// for HIT and one for MISS, and three launches on one stream make a frame:
//   k_grid_mark   one lane per point: a used point sets the byte of its endpoint cell in the hit plane with an atomic OR on the word
//                 around it; the lane that finds the byte clear appends the cell to the frame's ray list.  The plane thereby
//                 deduplicates the endpoints: rays are walked once per HIT cell, not once per point (a 128-beam cloud projects
//                 many returns into each cell), and the OR is contended only by the few points that share a cell
//   k_grid_rays   one wave per entry of the ray list: all 64 lanes take the steps k = lane, lane + 64, .. of that ONE ray (the walk
//                 is in closed form, so a ray of 4 cells and one of 4 000 cost what they are long, whatever mix a launch holds)
//                 and store 1 into the miss plane - relaxed, idempotent stores: every writer stores the same value, and hit and
//                 miss are separate planes, so nothing orders the stores but the end of the launch
//   k_grid_apply  one lane per 4 window cells: hit wins over miss, the counters of cells inside the grid saturate at 65 535, both
//                 planes are cleared for the next frame
// The counters are touched by exactly one lane per cell, without atomics.  The other atomics are the frame statistics and the list's
// length (one add per wave that has something to add).  No kernel uses LDS or scratch.
// Beside the frame: k_grid_readout, the occupancy byte of every cell, and k_grid_fill_unknown, which fills one grid's unknown cells
// from another grid's readout (kicp_grid_fill_unknown; described at the kernel).
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_grid_host.hpp"

namespace kicp {

constexpr uint32_t kGridBlock = 256;

static __device__ __forceinline__ void grid_plane_set(uint8_t *plane, size_t i) {
    __hip_atomic_store(plane + i, static_cast<uint8_t>(1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
static __device__ __forceinline__ uint32_t grid_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// stats[0] += points used (the host derives the skipped ones); stats[3] = entries of `rays`, the window cells that became HIT (room for
// n entries: at most one per point); hit_words: the hit plane as 32-bit words
static __global__ __launch_bounds__(kGridBlock) void k_grid_mark(const double *__restrict__ xyz, uint32_t n, GridGeom g, GridFrame f, uint32_t *__restrict__ hit_words,
                                                                 uint32_t *__restrict__ rays, unsigned int *__restrict__ stats) {
    const uint32_t i = blockIdx.x * kGridBlock + threadIdx.x;
    bool used = false, first = false;
    uint32_t cell = 0;
    if (i < n) {
        int32_t dx, dy;
        used = grid_endpoint(g, f, xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2], dx, dy);
        if (used) {
            const uint32_t side = 2u * static_cast<uint32_t>(g.reach) + 1u;
            cell = static_cast<uint32_t>(dy + g.reach) * side + static_cast<uint32_t>(dx + g.reach);  // < side^2 <= 8191^2 < 2^26
            const uint32_t bit = 1u << (8u * (cell & 3u));
            first = !(atomicOr(&hit_words[cell >> 2], bit) & bit);
        }
    }
    const unsigned long long b = __ballot(used), firsts = __ballot(first);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == 0u) {
        if (b) atomicAdd(&stats[0], static_cast<unsigned int>(__popcll(b)));
        if (firsts) base = atomicAdd(&stats[3], static_cast<unsigned int>(__popcll(firsts)));
    }
    base = __shfl(base, 0, 64);
    if (first) rays[base + static_cast<uint32_t>(__popcll(firsts & ((1ull << lane) - 1ull)))] = cell;
}

// rays[0 .. *n_rays): the window cells that are HIT this frame; one wave per ray, striding
static __global__ __launch_bounds__(kGridBlock) void k_grid_rays(const uint32_t *__restrict__ rays, const unsigned int *__restrict__ n_rays, int32_t reach,
                                                                 uint8_t *__restrict__ miss) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t side = 2u * static_cast<uint32_t>(reach) + 1u;
    const uint32_t waves = gridDim.x * (kGridBlock / 64u), count = *n_rays;
    for (uint32_t r = blockIdx.x * (kGridBlock / 64u) + threadIdx.x / 64u; r < count; r += waves) {
        const uint32_t cell = rays[r];
        const int32_t dx = static_cast<int32_t>(cell % side) - reach, dy = static_cast<int32_t>(cell / side) - reach;
        const uint32_t m = grid_walk_length(dx, dy);
        for (uint32_t k = lane; k < m; k += 64u) {
            int32_t ox, oy;
            grid_step(dx, dy, m, k, ox, oy);
            grid_plane_set(miss, static_cast<size_t>(oy + reach) * side + static_cast<size_t>(ox + reach));
        }
    }
}

// counts: cells x 2 (hits, misses).  stats[1] += cells HIT, stats[2] += cells MISS (cells inside the grid only).
static __global__ __launch_bounds__(kGridBlock) void k_grid_apply(uint32_t *__restrict__ hit_words, uint32_t *__restrict__ miss_words, uint32_t n_words, GridGeom g,
                                                                  GridFrame f, uint16_t *__restrict__ counts, unsigned int *__restrict__ stats) {
    const uint32_t i = blockIdx.x * kGridBlock + threadIdx.x;
    uint32_t n_hit = 0, n_miss = 0;
    if (i < n_words) {
        const uint32_t h = hit_words[i], m = miss_words[i];
        if (h | m) {
            const uint32_t side = 2u * static_cast<uint32_t>(g.reach) + 1u;
            for (uint32_t byte = 0; byte < 4u; ++byte) {
                const bool is_hit = (h >> (8u * byte)) & 0xFFu, is_miss = (m >> (8u * byte)) & 0xFFu;
                if (!(is_hit || is_miss)) continue;
                const uint32_t cell = 4u * i + byte;
                size_t c;
                if (!grid_inside(g, f, cell % side, cell / side, c)) continue;
                if (is_hit)
                    counts[2 * c] = grid_bump(counts[2 * c]), ++n_hit;
                else
                    counts[2 * c + 1] = grid_bump(counts[2 * c + 1]), ++n_miss;
            }
            if (h) hit_words[i] = 0u;
            if (m) miss_words[i] = 0u;
        }
    }
    const uint32_t packed = grid_wave_sum(n_hit | (n_miss << 16));  // (at most 4 per lane: 256 per wave and half)
    if ((threadIdx.x & 63u) == 0u) {
        if (packed & 0xFFFFu) atomicAdd(&stats[1], packed & 0xFFFFu);
        if (packed >> 16) atomicAdd(&stats[2], packed >> 16);
    }
}

// occupancy[i] = grid_readout(counts[i]); one lane per cell
static __global__ __launch_bounds__(kGridBlock) void k_grid_readout(const uint16_t *__restrict__ counts, size_t cells, uint32_t min_observations, int8_t *__restrict__ out) {
    const size_t i = static_cast<size_t>(blockIdx.x) * kGridBlock + threadIdx.x;
    if (i >= cells) return;
    const uint32_t pair = reinterpret_cast<const uint32_t *>(counts)[i];
    out[i] = grid_readout(pair & 0xFFFFu, pair >> 16, min_observations);
}

// ---- kicp_grid_fill_unknown: the unknown cells of one grid from the readout of another ------------------------------------------------
// A FIXED number of workgroups (at most kGridFillBlocks) stride over the cells: one 32-bit load per cell from each grid, a store only
// where the destination's pair changes.  Every lane keeps the seven tallies in registers over all its cells; at its end a wave sums
// each and its first lane adds what is not zero to the wave's shard of `counts` (nullable: kGridFillShards x kGridFillStride words, each
// shard on a 128-byte line of its own, summed on the host) - seven adds per wave whatever the grid's size, where an add per wave and
// 64 cells to one word queues for about 11 ns each.  cells <= 2^28 and the stride is 2^18, so i stays inside 32 bits.  No LDS, no scratch.
constexpr uint32_t kGridFillBlocks = 1024, kGridFillShards = 64, kGridFillStride = 32;
static __global__ __launch_bounds__(kGridBlock) void k_grid_fill_unknown(uint32_t *__restrict__ dst_pairs, const uint32_t *__restrict__ src_pairs, uint32_t cells,
                                                                         GridFillParams p, unsigned int *__restrict__ counts) {
    uint32_t tally[kGridFillCounts] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t i = blockIdx.x * kGridBlock + threadIdx.x; i < cells; i += gridDim.x * kGridBlock) {  // (every access is behind i < cells)
        const uint32_t d = dst_pairs[i];
        uint32_t which, disagree;
        const uint32_t after = grid_fill_pair(d, src_pairs[i], p, which, disagree);
        if (after != d) dst_pairs[i] = after;
#pragma unroll
        for (uint32_t k = 0; k < kGridFillCounts; ++k) tally[k] += (which == k || (k >= 5u && disagree == k)) ? 1u : 0u;  // (constant indices: registers)
    }
    if (!counts) return;
    unsigned int *shard = counts + ((blockIdx.x * (kGridBlock / 64u) + threadIdx.x / 64u) % kGridFillShards) * kGridFillStride;
#pragma unroll
    for (uint32_t k = 0; k < kGridFillCounts; ++k) {
        const uint32_t sum = grid_wave_sum(tally[k]);
        if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(&shard[k], sum);
    }
}

}  // namespace kicp
