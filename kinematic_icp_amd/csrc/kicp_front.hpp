// kicp_front.hpp -- the kernels of the grid's exploration frontiers (kicp_grid_frontiers; C-ABI: kicp_grid_explore.hip, arithmetic:
// kicp_front_host.hpp).  A frontier is a connected component of the frontier cells, its label the least cell index in it.  The
// components are found by UNION-FIND, which needs no rounds and no look from the host; the launches on the grid's stream are
//   k_front_mark     one lane per cell: the classes of the cell and of its four edge neighbours straight from the counters
//                    (grid_readout, clear_class; the neighbours' pairs come from L1 and L2), and one byte: frontier cell or not.
//   k_front_local    a 256-lane workgroup per tile of 32 x 32 cells, four cells a lane (k_nav_relax's mapping).  The tile's flags and
//                    a parent word per cell go into LDS (5 KB), every cell its own parent.  A tile without a frontier cell - most
//                    are - stores "none" for its cells after one __syncthreads_or and leaves.  Otherwise every frontier cell is united
//                    with its frontier neighbours W, NW, N and NE inside the tile - each undirected pair once - and after a barrier
//                    every cell stores parent[c]: the GLOBAL index of its root in the tile, "none" (0xFFFFFFFF) off the frontier.
//   k_front_border   one lane per cell of a tile's first row (united in global memory with its neighbours N, NW, NE in the tiles
//                    above) and of a tile's first column (W, NW, SW): every pair of neighbours that two tiles part, the diagonal
//                    across a tile corner included.
//   k_front_flatten  one lane per cell: parent[c] = find(c), now the label; the roots - parent[c] == c - take a dense row number
//                    from a counter, one atomic add per wave.
//   k_front_rows     (after the host has read the counter and sized the rows) one lane per row: the empty row.
//   k_front_sum      one lane per cell: a frontier cell adds itself to its root's row, one 64-bit atomic per word: add for the size
//                    and the sums, min and max for the box, min for the key pot(c) * 2^32 + c.  All of them commute, so the rows do
//                    not depend on the order of arrival.  Lanes of a wave that share a root are not combined first: frontier cells
//                    are about one in a hundred, and a wave seldom holds more than a few of one frontier.
// k_front_local, k_front_border and k_front_flatten take any flag plane: kicp_grid_transient.hip runs them over its own (kicp_transient.hpp).
//
// THE INVARIANT that keeps the union-find safe where nothing may wait: parent[c] <= c ALWAYS, AND A STORED PARENT ONLY EVER FALLS.
// A cell starts as its own parent (or, in global memory, under its tile's root, which is the least index of its tile's component);
// the only store after that is atomicMin(&parent[a], b) with b < a, and k_front_flatten's store of an ancestor.  Hence every find
// walks strictly downward and ends at the latest at cell 0, and the union loop
//   loop: a = find(a); b = find(b); if a == b done; make a the larger; old = atomicMin(&parent[a], b); if old == a done; a = old;
// strictly lowers max(a, b) on each trip.  No lane waits for another lane, wave or workgroup: there is no spin wait, no grid-wide
// barrier and no persistent kernel.  A read that is stale - another lane lowered the word meanwhile - only sends the loop round once
// more: the atomic returns the word as it is, and when it was not `a` any more the loop goes on from what it held, to which `a` is
// joined already.  The root of a component is its least index: exactly the label include/kicp.h defines.  No path compression
// during the unions: a plain store could lift a word that an atomic has just lowered.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_front_host.hpp"

namespace kicp {

constexpr uint32_t kFrontBlock = 256;
constexpr uint32_t kFrontTile = 32;
static_assert(kFrontBlock * 4u == kFrontTile * kFrontTile, "four cells per lane");

static __device__ __forceinline__ uint32_t front_class_at(const uint32_t *__restrict__ pairs, size_t cell, const FrontParams &p) {
    const uint32_t pair = pairs[cell];
    return clear_class(grid_readout(pair & 0xFFFFu, pair >> 16, p.min_observations), p.source_min);
}

static __global__ __launch_bounds__(kFrontBlock) void k_front_mark(const uint16_t *__restrict__ counts, uint32_t width, uint32_t height, uint32_t cells, FrontParams p,
                                                                  uint8_t *__restrict__ flags) {
    const uint32_t c = blockIdx.x * kFrontBlock + threadIdx.x;
    if (c >= cells) return;
    const uint32_t *pairs = reinterpret_cast<const uint32_t *>(counts);
    const uint32_t x = c % width, y = c / width;
    const uint32_t own = front_class_at(pairs, c, p);
    bool frontier = false;
    if (own == kClearClear) {
        const uint32_t west = x > 0u ? front_class_at(pairs, c - 1u, p) : kFrontOutside, east = x + 1u < width ? front_class_at(pairs, c + 1u, p) : kFrontOutside;
        const uint32_t south = y > 0u ? front_class_at(pairs, c - width, p) : kFrontOutside, north = y + 1u < height ? front_class_at(pairs, c + width, p) : kFrontOutside;
        frontier = front_is_frontier(own, west, east, south, north);
    }
    flags[c] = frontier ? 1u : 0u;
}

// the union-find over the words of a tile in LDS: indices are ly * 32 + lx, whose order inside a tile is the cell indices' order
static __device__ __forceinline__ uint32_t front_find_lds(const volatile uint32_t *parent, uint32_t a) {
    for (uint32_t p; (p = parent[a]) != a;) a = p;
    return a;
}
static __device__ __forceinline__ void front_union_lds(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = front_find_lds(parent, a), b = front_find_lds(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b, b = t;
        }
        const uint32_t old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}
// the same over the parent plane in global memory; the loads are relaxed device-scope atomics, which no cache of this CU serves
static __device__ __forceinline__ uint32_t front_find(uint32_t *parent, uint32_t a) {
    for (uint32_t p; (p = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != a;) a = p;
    return a;
}
static __device__ __forceinline__ void front_union(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = front_find(parent, a), b = front_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b, b = t;
        }
        const uint32_t old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

// blockIdx.x = tile_y * tiles_x + tile_x
static __global__ __launch_bounds__(kFrontBlock) void k_front_local(const uint8_t *__restrict__ flags, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                   uint32_t *__restrict__ parent) {
    __shared__ uint8_t s_flag[kFrontTile * kFrontTile];
    __shared__ uint32_t s_parent[kFrontTile * kFrontTile];
    const uint32_t x0 = (blockIdx.x % tiles_x) * kFrontTile, y0 = (blockIdx.x / tiles_x) * kFrontTile;
    // lane l owns the cells (l % 32, l / 32 + 8 j), j = 0 .. 3, of the tile: a wave touches two rows of 32 consecutive words
    const uint32_t lx = threadIdx.x % kFrontTile, ly = threadIdx.x / kFrontTile, x = x0 + lx;
    uint32_t own[4];
    int any = 0;
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t cy = ly + 8u * j, y = y0 + cy, l = cy * kFrontTile + lx;
        own[j] = (x < width && y < height) ? flags[static_cast<size_t>(y) * width + x] : 0u;
        s_flag[l] = static_cast<uint8_t>(own[j]), s_parent[l] = l;
        any |= static_cast<int>(own[j]);
    }
    if (!__syncthreads_or(any)) {
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t y = y0 + ly + 8u * j;
            if (x < width && y < height) parent[static_cast<size_t>(y) * width + x] = kFrontNone;
        }
        return;
    }
    for (uint32_t j = 0; j < 4u; ++j) {
        if (!own[j]) continue;
        const uint32_t cy = ly + 8u * j, l = cy * kFrontTile + lx;
        if (lx > 0u && s_flag[l - 1u]) front_union_lds(s_parent, l, l - 1u);
        if (cy == 0u) continue;
        if (lx > 0u && s_flag[l - kFrontTile - 1u]) front_union_lds(s_parent, l, l - kFrontTile - 1u);
        if (s_flag[l - kFrontTile]) front_union_lds(s_parent, l, l - kFrontTile);
        if (lx + 1u < kFrontTile && s_flag[l - kFrontTile + 1u]) front_union_lds(s_parent, l, l - kFrontTile + 1u);
    }
    __syncthreads();
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t cy = ly + 8u * j, y = y0 + cy;
        if (!(x < width && y < height)) continue;
        uint32_t value = kFrontNone;
        if (own[j]) {
            const uint32_t root = front_find_lds(s_parent, cy * kFrontTile + lx);
            value = (y0 + root / kFrontTile) * width + x0 + root % kFrontTile;  // (a frontier cell's: inside the grid)
        }
        parent[static_cast<size_t>(y) * width + x] = value;
    }
}

// Lanes 0 .. row_lanes - 1: cell (i % width, 32 (i / width + 1)), a tile's first row; the others: cell (32 (j / height + 1), j % height)
// with j = i - row_lanes, a tile's first column.  A cell on both is visited twice, which does no harm.
static __global__ __launch_bounds__(kFrontBlock) void k_front_border(const uint8_t *__restrict__ flags, uint32_t width, uint32_t height, uint32_t row_lanes,
                                                                    uint32_t lanes, uint32_t *parent) {
    const uint32_t i = blockIdx.x * kFrontBlock + threadIdx.x;
    if (i >= lanes) return;
    if (i < row_lanes) {
        const uint32_t x = i % width, y = (i / width + 1u) * kFrontTile, c = y * width + x, below = c - width;  // y >= 32
        if (!flags[c]) return;
        if (x > 0u && flags[below - 1u]) front_union(parent, c, below - 1u);
        if (flags[below]) front_union(parent, c, below);
        if (x + 1u < width && flags[below + 1u]) front_union(parent, c, below + 1u);
    } else {
        const uint32_t j = i - row_lanes, x = (j / height + 1u) * kFrontTile, y = j % height, c = y * width + x;  // x >= 32
        if (!flags[c]) return;
        if (flags[c - 1u]) front_union(parent, c, c - 1u);
        if (y > 0u && flags[c - width - 1u]) front_union(parent, c, c - width - 1u);
        if (y + 1u < height && flags[c + width - 1u]) front_union(parent, c, c + width - 1u);
    }
}

// parent becomes the label plane; row_of[root] = the root's row number; *counter += the number of roots
static __global__ __launch_bounds__(kFrontBlock) void k_front_flatten(const uint8_t *__restrict__ flags, uint32_t cells, uint32_t *parent, uint32_t *__restrict__ row_of,
                                                                     uint32_t *counter) {
    const uint32_t c = blockIdx.x * kFrontBlock + threadIdx.x;
    bool is_root = false;
    if (c < cells && flags[c]) {
        const uint32_t root = front_find(parent, c);
        if (root != c) parent[c] = root;  // an ancestor: the word falls
        is_root = root == c;
    }
    const unsigned long long roots = __ballot(is_root);
    if (roots == 0ull) return;
    const uint32_t lane = threadIdx.x % 64u, leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(roots))) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, static_cast<uint32_t>(__popcll(roots)));
    base = __shfl(base, static_cast<int>(leader));
    if (is_root) row_of[c] = base + static_cast<uint32_t>(__popcll(roots & ((1ull << lane) - 1ull)));
}

static __global__ __launch_bounds__(kFrontBlock) void k_front_rows(unsigned long long *__restrict__ rows, uint32_t n_rows) {
    const uint32_t i = blockIdx.x * kFrontBlock + threadIdx.x;
    if (i < n_rows) front_row_init(rows + static_cast<size_t>(i) * kFrontWords, 0u);
}

// labels: what k_front_flatten left; pot: the plan's potential, or nullptr (pot(c) = 0xFFFFFFFF); rows: n_rows = the counter's value
static __global__ __launch_bounds__(kFrontBlock) void k_front_sum(const uint8_t *__restrict__ flags, const uint32_t *__restrict__ labels, const uint32_t *__restrict__ row_of,
                                                                 const uint32_t *__restrict__ pot, uint32_t width, uint32_t cells, uint32_t n_rows,
                                                                 unsigned long long *rows) {
    const uint32_t c = blockIdx.x * kFrontBlock + threadIdx.x;
    if (c >= cells || !flags[c]) return;
    const uint32_t root = labels[c], id = row_of[root];
    if (id >= n_rows) return;  // cannot happen: the roots were counted by the launch that numbered them
    unsigned long long *row = rows + static_cast<size_t>(id) * kFrontWords;
    const unsigned long long x = c % width, y = c / width;
    if (root == c) row[0] = c;
    atomicAdd(row + 1, 1ull), atomicAdd(row + 2, x), atomicAdd(row + 3, y);
    atomicMin(row + 4, x), atomicMax(row + 5, x), atomicMin(row + 6, y), atomicMax(row + 7, y);
    atomicMin(row + 8, front_key(pot ? pot[c] : kFrontNone, c));
}

}  // namespace kicp
