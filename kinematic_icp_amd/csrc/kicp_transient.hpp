// kicp_transient.hpp -- the kernels of the grid's transient obstacles (kicp_grid_transients; C-ABI: kicp_grid_transient.hip, arithmetic:
// kicp_transient_host.hpp).  Three planes lie over the grid and are ZERO BETWEEN CALLS: a 32-bit count of returns per cell, a flag byte
// per cell, and - what a call leaves behind on purpose - the transient plane.  A frame touches few cells, so all but the components
// work on the TOUCHED LIST, the cells that received a return; the launches on the grid's stream are
//   k_transient_count   one lane per point: grid_endpoint and grid_inside give the global cell, one atomicAdd counts the return, and
//                       the lane that reads back 0 appends the cell to the touched list by ballot compaction (k_grid_mark's way with
//                       its ray list).  The used points, the points inside the grid and the list's length are one add per wave each.
//                       Lanes of a wave that share a cell are not combined before the atomic (not measured: DESIGN.md 5j).
//   k_transient_flag    one lane per touched entry: n(c) and the counter pair give the flag byte (transient_is_cell); only a 1 is
//                       stored.  The transient cells are counted, one add per wave.
//   k_front_local, k_front_border, k_front_flatten (kicp_front.hpp) over this flag plane: the frontiers' union-find, grid-wide.
//   k_transient_rows    (after the host has read the number of roots and the list's length) one lane per row: the empty row.
//   k_transient_sum     one lane per touched entry: a transient cell adds itself to its root's row, one 64-bit atomic per word: add
//                       for the size, the returns and the two sums, min and max for the box, min for the key.  All commute.
//   k_transient_finish  one lane per touched entry: the plane byte - flag and the root's size at least min_size - and the reset of the
//                       cell's count and flag.  The plane itself was cleared by a memset before the first launch.
// No LDS of their own, no scratch, no floating point after grid_endpoint.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_transient_host.hpp"

namespace kicp {

constexpr uint32_t kTransientBlock = 256;

// one add per wave of what its lanes vote for; returns the base the wave's first voter got (for a compaction)
static __device__ __forceinline__ uint32_t transient_wave_add(unsigned int *counter, unsigned long long votes, uint32_t lane) {
    uint32_t base = 0;
    if (lane == 0u && votes) base = atomicAdd(counter, static_cast<unsigned int>(__popcll(votes)));
    return __shfl(base, 0, 64);
}

// returns: a word per cell, zero on entry; touched: room for n entries (at most one per point); stats[0] += used points, stats[1] +=
// those inside the grid, stats[2] = entries of `touched`
static __global__ __launch_bounds__(kTransientBlock) void k_transient_count(const double *__restrict__ xyz, uint32_t n, GridGeom g, GridFrame f, uint32_t *returns,
                                                                             uint32_t *__restrict__ touched, unsigned int *stats) {
    const uint32_t i = blockIdx.x * kTransientBlock + threadIdx.x;
    bool used = false, inside = false, first = false;
    uint32_t cell = 0;
    if (i < n) {
        int32_t dx, dy;
        used = grid_endpoint(g, f, xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2], dx, dy);
        size_t c = 0;
        inside = used && grid_inside(g, f, static_cast<uint32_t>(dx + g.reach), static_cast<uint32_t>(dy + g.reach), c);  // c < width * height <= 2^28
        if (inside) cell = static_cast<uint32_t>(c), first = atomicAdd(&returns[c], 1u) == 0u;
    }
    const unsigned long long b_used = __ballot(used), b_inside = __ballot(inside), b_first = __ballot(first);
    const uint32_t lane = threadIdx.x & 63u;
    transient_wave_add(&stats[0], b_used, lane), transient_wave_add(&stats[1], b_inside, lane);
    const uint32_t base = transient_wave_add(&stats[2], b_first, lane);
    if (first) touched[base + static_cast<uint32_t>(__popcll(b_first & ((1ull << lane) - 1ull)))] = cell;
}

// lanes: the launch's (>= *n_touched); flags: a byte per cell, zero on entry; stats[3] += transient cells
static __global__ __launch_bounds__(kTransientBlock) void k_transient_flag(const uint32_t *__restrict__ touched, const unsigned int *__restrict__ n_touched,
                                                                            const uint32_t *__restrict__ returns, const uint16_t *__restrict__ counts, TransientParams p,
                                                                            uint8_t *__restrict__ flags, unsigned int *stats) {
    const uint32_t i = blockIdx.x * kTransientBlock + threadIdx.x;
    bool is = false;
    if (i < *n_touched) {
        const uint32_t c = touched[i];
        is = transient_is_cell(returns[c], reinterpret_cast<const uint32_t *>(counts)[c], p);
        if (is) flags[c] = 1u;
    }
    transient_wave_add(&stats[3], __ballot(is), threadIdx.x & 63u);
}

static __global__ __launch_bounds__(kTransientBlock) void k_transient_rows(unsigned long long *__restrict__ rows, uint32_t n_rows) {
    const uint32_t i = blockIdx.x * kTransientBlock + threadIdx.x;
    if (i < n_rows) transient_row_init(rows + static_cast<size_t>(i) * kTransientWords, 0u);
}

// labels, row_of: what k_front_flatten left; (sx, sy): the sensor's cell; rows: n_rows = the number of roots
static __global__ __launch_bounds__(kTransientBlock) void k_transient_sum(const uint32_t *__restrict__ touched, uint32_t n_touched, const uint32_t *__restrict__ returns,
                                                                           const uint8_t *__restrict__ flags, const uint32_t *__restrict__ labels,
                                                                           const uint32_t *__restrict__ row_of, uint32_t width, int64_t sx, int64_t sy, uint32_t n_rows,
                                                                           unsigned long long *rows) {
    const uint32_t i = blockIdx.x * kTransientBlock + threadIdx.x;
    if (i >= n_touched) return;
    const uint32_t c = touched[i];
    if (!flags[c]) return;
    const uint32_t root = labels[c], id = row_of[root];
    if (id >= n_rows) return;  // cannot happen: the roots were counted by the launch that numbered them
    unsigned long long *row = rows + static_cast<size_t>(id) * kTransientWords;
    const uint32_t x = c % width, y = c / width;
    const unsigned long long n = returns[c];
    if (root == c) row[0] = c;
    atomicAdd(row + 1, 1ull), atomicAdd(row + 2, n), atomicAdd(row + 3, n * x), atomicAdd(row + 4, n * y);
    atomicMin(row + 5, static_cast<unsigned long long>(x)), atomicMax(row + 6, static_cast<unsigned long long>(x));
    atomicMin(row + 7, static_cast<unsigned long long>(y)), atomicMax(row + 8, static_cast<unsigned long long>(y));
    atomicMin(row + 9, transient_key(x, y, sx, sy, c));
}

// plane: a byte per cell, zero on entry; rows: summed (read only where a cell is flagged: then n_rows >= 1)
static __global__ __launch_bounds__(kTransientBlock) void k_transient_finish(const uint32_t *__restrict__ touched, uint32_t n_touched, const uint32_t *__restrict__ labels,
                                                                              const uint32_t *__restrict__ row_of, const unsigned long long *__restrict__ rows, uint32_t n_rows,
                                                                              uint32_t min_size, uint32_t *__restrict__ returns, uint8_t *__restrict__ flags,
                                                                              uint8_t *__restrict__ plane) {
    const uint32_t i = blockIdx.x * kTransientBlock + threadIdx.x;
    if (i >= n_touched) return;
    const uint32_t c = touched[i];
    if (flags[c]) {
        const uint32_t id = row_of[labels[c]];
        if (id < n_rows && rows[static_cast<size_t>(id) * kTransientWords + 1u] >= min_size) plane[c] = 1u;
        flags[c] = 0u;
    }
    returns[c] = 0u;
}

}  // namespace kicp
