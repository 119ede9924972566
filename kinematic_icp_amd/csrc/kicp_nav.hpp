// kicp_nav.hpp -- the kernels of the cost-to-go field over the grid's costmap (kicp_grid_potential, kicp_grid_potential_of_costmap;
// C-ABI: kicp_grid_plan.hip, arithmetic: kicp_nav_host.hpp).  The field is the least fixed point of a min-plus recurrence over integers, so
// any order of relaxation reaches the same values; the launches on the grid's stream are
//   k_nav_init   one lane per cell: q = weight[costmap] (a byte) and the potential "unreached".
//   k_nav_goals  one lane per goal: potential 0 on a passable goal, and the activity flag of its tile up.
//   k_nav_relax  one ROUND: a 256-lane workgroup per tile of 32 x 32 cells, four cells a lane.  A tile whose flag is down leaves at
//                once.  Otherwise it lowers its own flag, loads its potentials and weights with a halo of one cell into LDS (34 x 34
//                words and bytes), relaxes inside LDS until a sweep changes nothing (at most 1024 sweeps, the tile's cell count: a
//                tile that stops there raises its own flag again), stores the cells that fell, and raises the NEXT round's flag of
//                each of the eight neighbour tiles whose facing border cells fell.  The count of raised flags goes to the round's
//                counter with one atomic add per workgroup, the only atomic here.
//   k_nav_count  the cells below max_potential and equal to it, for the statistics.
// Rounds are separate launches; the host reads the counters after a batch of them and stops at the first round that raised nothing
// (kicp_grid_plan.hip).  The flags are bytes in two planes, used by round parity: round r reads plane r & 1 and writes plane (r + 1) & 1,
// which round r - 1 read and lowered.  No workgroup waits for another, no floating point.
//
// Why races do not matter.  Inside a sweep a lane reads LDS words that other lanes are storing to, and while a tile loads its halo the
// owner of those cells may be storing them.  A potential only ever falls, every stored value is the length of a real path (or the
// clamp), and 32-bit accesses do not tear: a stale read can delay a cell, never make it wrong.  A delayed cell is caught because the
// sweeps go on until one changes nothing after a barrier, and a halo read too early because its owner raises this tile's flag for the
// next round whenever a border cell fell.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_nav_host.hpp"

namespace kicp {

constexpr uint32_t kNavBlock = 256;
constexpr uint32_t kNavSpan = kNavTile + 2u;   // a tile with its halo
constexpr uint32_t kNavMaxSweeps = kNavTile * kNavTile;
constexpr uint32_t kNavBatch = 16;             // rounds between two looks at the counters: d_nav_ctr[0 .. 15], then the two cell counts
static_assert(kNavBlock * 4u == kNavTile * kNavTile, "four cells per lane");

static __global__ __launch_bounds__(kNavBlock) void k_nav_init(const uint8_t *__restrict__ costmap, const uint8_t *__restrict__ weight, uint32_t cells,
                                                               uint8_t *__restrict__ q, uint32_t *__restrict__ pot) {
    const uint32_t c = blockIdx.x * kNavBlock + threadIdx.x;
    if (c >= cells) return;
    q[c] = weight[costmap[c]];
    pot[c] = kNavUnreached;
}

// goals: n pairs (x, y), all inside the grid (checked on the host)
static __global__ __launch_bounds__(kNavBlock) void k_nav_goals(const uint32_t *__restrict__ goals, uint32_t n, uint32_t width, uint32_t tiles_x,
                                                                const uint8_t *__restrict__ q, uint32_t *pot, uint8_t *flags) {
    const uint32_t g = blockIdx.x * kNavBlock + threadIdx.x;
    if (g >= n) return;
    const uint32_t x = goals[2 * g], y = goals[2 * g + 1];
    const size_t c = static_cast<size_t>(y) * width + x;
    if (q[c] == 0u) return;
    pot[c] = 0u;
    flags[(y / kNavTile) * tiles_x + x / kNavTile] = 1u;
}

// blockIdx.x = tile_y * tiles_x + tile_x; flags_in / flags_out: this round's and the next round's plane; counter: this round's
static __global__ __launch_bounds__(kNavBlock) void k_nav_relax(uint32_t *pot, const uint8_t *__restrict__ q, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                uint32_t tiles_y, uint32_t max_potential, uint8_t *flags_in, uint8_t *flags_out, uint32_t *counter) {
    __shared__ uint32_t s_pot[kNavSpan * kNavSpan];
    __shared__ uint8_t s_q[kNavSpan * kNavSpan];
    __shared__ uint32_t s_raise[9];  // the neighbour tile at (dx, dy) is slot (dy + 1) * 3 + dx + 1; slot 4 is this tile
    const uint32_t tile = blockIdx.x;
    if (flags_in[tile] == 0u) return;  // (uniform: every lane reads the same byte, and nobody writes this plane during this round)
    const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
    const int64_t x0 = static_cast<int64_t>(tx) * kNavTile - 1, y0 = static_cast<int64_t>(ty) * kNavTile - 1;  // the halo's corner
    for (uint32_t i = threadIdx.x; i < kNavSpan * kNavSpan; i += kNavBlock) {
        const int64_t x = x0 + i % kNavSpan, y = y0 + i / kNavSpan;
        const bool inside = x >= 0 && y >= 0 && x < static_cast<int64_t>(width) && y < static_cast<int64_t>(height);
        const size_t c = inside ? static_cast<size_t>(y) * width + static_cast<size_t>(x) : 0u;
        s_q[i] = inside ? q[c] : static_cast<uint8_t>(0u);
        s_pot[i] = inside ? pot[c] : kNavUnreached;
    }
    if (threadIdx.x < 9u) s_raise[threadIdx.x] = 0u;
    __syncthreads();  // (also: every lane has read the flag)
    if (threadIdx.x == 0u) flags_in[tile] = 0u;

    // lane l owns the cells (l % 32, l / 32 + 8 j), j = 0 .. 3, of the tile: a wave reads two rows of 32 consecutive words
    const uint32_t lx = threadIdx.x % kNavTile, ly = threadIdx.x / kNavTile;
    uint32_t at[4], own_q[4], first[4];
    for (uint32_t j = 0; j < 4u; ++j) {
        at[j] = (ly + 8u * j + 1u) * kNavSpan + lx + 1u;
        own_q[j] = s_q[at[j]], first[j] = s_pot[at[j]];
    }
    volatile uint32_t *v_pot = s_pot;
    uint32_t sweeps = 0;
    int more;
    do {
        int changed = 0;
        for (uint32_t j = 0; j < 4u; ++j) {
            if (own_q[j] == 0u) continue;
            const uint32_t was = v_pot[at[j]];
            uint32_t best = was;
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {
                const uint32_t n = static_cast<uint32_t>(static_cast<int32_t>(at[j]) + nav_dy(k) * static_cast<int32_t>(kNavSpan) + nav_dx(k));
                best = nav_relax(best, own_q[j], s_q[n], v_pot[n], k, max_potential);
            }
            if (best < was) v_pot[at[j]] = best, changed = 1;
        }
        more = __syncthreads_or(changed);
    } while (more && ++sweeps < kNavMaxSweeps);

    // store what fell, and note which neighbour tiles now read a lower halo
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t cy = ly + 8u * j, now = s_pot[at[j]];
        if (now >= first[j]) continue;
        pot[static_cast<size_t>(y0 + 1 + cy) * width + static_cast<size_t>(x0 + 1 + lx)] = now;  // (own_q != 0: the cell lies inside the grid)
        const int32_t ex = lx == 0u ? -1 : lx == kNavTile - 1u ? 1 : 0, ey = cy == 0u ? -1 : cy == kNavTile - 1u ? 1 : 0;
        if (ex) s_raise[4 + ex] = 1u;
        if (ey) s_raise[4 + 3 * ey] = 1u;
        if (ex && ey) s_raise[4 + 3 * ey + ex] = 1u;
    }
    if (more && threadIdx.x == 0u) s_raise[4] = 1u;  // stopped at the sweep limit: this tile goes on in the next round
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t raised = 0;
        for (int32_t dy = -1; dy <= 1; ++dy)
            for (int32_t dx = -1; dx <= 1; ++dx) {
                const int64_t nx = static_cast<int64_t>(tx) + dx, ny = static_cast<int64_t>(ty) + dy;
                if (s_raise[(dy + 1) * 3 + dx + 1] == 0u || nx < 0 || ny < 0 || nx >= static_cast<int64_t>(tiles_x) || ny >= static_cast<int64_t>(tiles_y)) continue;
                flags_out[static_cast<size_t>(ny) * tiles_x + static_cast<size_t>(nx)] = 1u;
                ++raised;
            }
        if (raised) atomicAdd(counter, raised);
    }
}

// counts[0] += cells below max_potential, counts[1] += cells equal to it; the workgroups stride over the cells
static __global__ __launch_bounds__(kNavBlock) void k_nav_count(const uint32_t *__restrict__ pot, uint32_t cells, uint32_t max_potential, uint32_t *counts) {
    uint32_t below = 0, equal = 0;
    for (uint32_t c = blockIdx.x * kNavBlock + threadIdx.x; c < cells; c += gridDim.x * kNavBlock) {
        const uint32_t p = pot[c];
        below += p < max_potential ? 1u : 0u, equal += p == max_potential ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o), equal += __shfl_xor(equal, o);
    if (threadIdx.x % 64u == 0u) {
        if (below) atomicAdd(counts, below);
        if (equal) atomicAdd(counts + 1, equal);
    }
}

}  // namespace kicp
