// kicp_search.hpp -- kernels of the whole-map relocalisation (kicp_occ_*, kicp_search_poses; host side: kicp_search.hip, traversal:
// kicp_search_host.hpp): the occupancy pyramid of a map as bits, and the scores of search nodes against one of its levels.
//
// Layout of a level (include/kicp.h): 32-bit words along x; cell (x, y, z) is bit (x & 31) of word (z * dims.y + y) * wx + (x >> 5),
// the bits of a row's last word beyond dims.x are zero.  Every level has level 0's resolution; the levels lie one behind the other.
#pragma once
#include "kicp_common.hpp"

namespace kicp {

struct OccGrid {
    double min[3];
    double cell;
    int32_t dims[3];
    uint32_t wx;                    // words per row
    unsigned long long level_words; // wx * dims.y * dims.z
};
// floor((v - min) / cell) as an int32, in the header's operation order; anything that is not a cell of a grid of < 2^24 cells per axis
// (far away, NaN) becomes kOccFar, which stays out of every grid after a node offset of up to 2^20 has been added
constexpr int32_t kOccFar = -(1 << 28);
KICP_HD int32_t occ_cell(double v, double mn, double cell) {
    const double c = floor((v - mn) / cell);
    return (c >= -16777216.0 && c <= 16777216.0) ? static_cast<int32_t>(c) : kOccFar;
}
// order-preserving image of a double in an unsigned 64-bit integer (for atomicMin / atomicMax)
KICP_HD unsigned long long occ_order_key(double v) {
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the map's bounding box: bounds[0..2] = min of the keys per axis, bounds[3..5] = max (initialised to ~0 / 0 by the host).
// One thread per table slot; occupied slots walk their bucket of the fp64 pool.
static __global__ __launch_bounds__(256) void k_occ_bounds(const Slot *table, uint32_t slots, const double *pool, uint32_t cap, uint32_t cbits,
                                                          unsigned long long *bounds) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    if (h < slots) {
        const uint32_t val = table[h].val;
        const uint32_t c = val == kEmptyVal ? 0u : val_count(val, cbits);
        const double *b = pool + static_cast<size_t>(val_bucket(val, cbits)) * cap * 3;
        for (uint32_t k = 0; k < c; ++k)
            for (int a = 0; a < 3; ++a) {
                const unsigned long long key = occ_order_key(b[3 * k + a]);
                lo[a] = key < lo[a] ? key : lo[a], hi[a] = key > hi[a] ? key : hi[a];
            }
    }
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long l = __shfl_down(lo[a], off, 64), u = __shfl_down(hi[a], off, 64);
            lo[a] = l < lo[a] ? l : lo[a], hi[a] = u > hi[a] ? u : hi[a];
        }
        if ((threadIdx.x & 63u) == 0u && lo[a] <= hi[a]) atomicMin(bounds + a, lo[a]), atomicMax(bounds + 3 + a, hi[a]);
    }
}

// level 0: every map point sets its own cell and every cell within `dilate` of it on all three axes (clipped to the grid, which by
// its geometry holds them all).  One thread per table slot, 32-bit atomicOr.
static __global__ __launch_bounds__(256) void k_occ_mark(const Slot *table, uint32_t slots, const double *pool, uint32_t cap, uint32_t cbits, const OccGrid g,
                                                        int dilate, uint32_t *bits) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= slots) return;
    const uint32_t val = table[h].val;
    if (val == kEmptyVal) return;
    const uint32_t c = val_count(val, cbits);
    const double *b = pool + static_cast<size_t>(val_bucket(val, cbits)) * cap * 3;
    for (uint32_t k = 0; k < c; ++k) {
        const int32_t cx = occ_cell(b[3 * k], g.min[0], g.cell), cy = occ_cell(b[3 * k + 1], g.min[1], g.cell), cz = occ_cell(b[3 * k + 2], g.min[2], g.cell);
        const int32_t x0 = max(cx - dilate, 0), x1 = min(cx + dilate, g.dims[0] - 1);
        if (x0 > x1) continue;
        for (int32_t z = max(cz - dilate, 0); z <= min(cz + dilate, g.dims[2] - 1); ++z)
            for (int32_t y = max(cy - dilate, 0); y <= min(cy + dilate, g.dims[1] - 1); ++y) {
                uint32_t *row = bits + (static_cast<size_t>(z) * g.dims[1] + y) * g.wx;
                // (2 dilate + 1 <= 9 bits: one word, or two when the run crosses a word boundary)
                const uint32_t w0 = static_cast<uint32_t>(x0) >> 5, w1 = static_cast<uint32_t>(x1) >> 5;
                const uint32_t from = 0xFFFFFFFFu << (x0 & 31), to = 0xFFFFFFFFu >> (31 - (x1 & 31));
                if (w0 == w1) atomicOr(row + w0, from & to);
                else atomicOr(row + w0, from), atomicOr(row + w1, to);
            }
    }
}

// the set bits of a level (level 0's count is kicp_occ_info's)
static __global__ __launch_bounds__(256) void k_occ_count(const uint32_t *bits, unsigned long long words, unsigned long long *out) {
    unsigned long long c = 0;
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < words; i += gridDim.x * 256ull) c += __popc(bits[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63u) == 0u && c) atomicAdd(out, c);
}

// level h from level h - 1: out(x, y) = in(x, y) | in(x + s, y) | in(x, y + s) | in(x + s, y + s), s = 2^(h - 1), cells beyond the grid
// empty.  One thread per output word; the shift by s crosses a word boundary for s < 32 and moves whole words from s = 32.
static __global__ __launch_bounds__(256) void k_occ_pool(const uint32_t *in, uint32_t *out, const OccGrid g, uint32_t s) {
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= g.level_words) return;
    const uint32_t w = static_cast<uint32_t>(i % g.wx);
    const unsigned long long row = i / g.wx;
    const uint32_t y = static_cast<uint32_t>(row % static_cast<uint32_t>(g.dims[1]));
    auto both = [&](const uint32_t *r) {  // r(x) | r(x + s) for the 32 cells of word w of row r
        uint32_t v = r[w];
        if (s < 32u) v |= (r[w] >> s) | (w + 1u < g.wx ? r[w + 1u] << (32u - s) : 0u);
        else if (w + (s >> 5) < g.wx) v |= r[w + (s >> 5)];
        return v;
    };
    const uint32_t *r0 = in + row * g.wx;
    uint32_t v = both(r0);
    if (y + s < static_cast<uint32_t>(g.dims[1])) v |= both(r0 + static_cast<size_t>(s) * g.wx);
    out[i] = v;
}

// ---- scoring -----------------------------------------------------------------------------------------------------------------
struct SearchWindowDev {
    double x0, y0, z;
    uint32_t nx, ny, nyaw;
};
// the cell of every frame point at every yaw (THE cell expression of include/kicp.h, written here once): cells[(3 j + axis) * n + i]
static __global__ __launch_bounds__(256) void k_search_cells(const double *frame, uint32_t n, const double *cs, const SearchWindowDev w, const OccGrid g,
                                                            int32_t *cells) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double px = frame[3 * i], py = frame[3 * i + 1], pz = frame[3 * i + 2];
    for (uint32_t j = blockIdx.y; j < w.nyaw; j += gridDim.y) {
        const double c = cs[2 * j], s = cs[2 * j + 1];
        int32_t *o = cells + static_cast<size_t>(3u * j) * n + i;
        o[0] = occ_cell((c * px - s * py) + w.x0, g.min[0], g.cell);
        o[n] = occ_cell((s * px + c * py) + w.y0, g.min[1], g.cell);
        o[2 * static_cast<size_t>(n)] = occ_cell(pz + w.z, g.min[2], g.cell);
    }
}

constexpr int kSearchBlock = 256;  // four waves, one node each at a time
// One wave per node: its lanes stride the node's yaw's cells (coalesced), each tests one bit per point (a gather into the level's
// bitset), the wave adds up and lane 0 stores the count - a node has one owner, nothing is atomic.  The waves of the launch stride
// over the nodes.  `level_bits` is level `level`: there a block that starts less than its size 2^level below the grid in x or y still
// covers cells of the grid, all of them inside the block that starts AT the edge - such a coordinate reads column / row 0, which
// keeps the score an upper bound of every node of the block (level 0: no such coordinate exists).
static __global__ __launch_bounds__(kSearchBlock) void k_search_score(const int32_t *cells, uint32_t n, const uint32_t *level_bits, const OccGrid g,
                                                                     const SearchWindowDev w, int level, const unsigned long long *nodes,
                                                                     unsigned long long count, uint32_t *hits) {
    const uint32_t lane = threadIdx.x & 63u;
    const int32_t lowest = -(1 << level);
    const unsigned long long waves = static_cast<unsigned long long>(gridDim.x) * (kSearchBlock / 64);
    for (unsigned long long k = static_cast<unsigned long long>(blockIdx.x) * (kSearchBlock / 64) + (threadIdx.x >> 6); k < count; k += waves) {
        const unsigned long long node = nodes[k];
        const int32_t ix = static_cast<int32_t>(node % w.nx);
        const unsigned long long row = node / w.nx;
        const int32_t iy = static_cast<int32_t>(row % w.ny);
        const uint32_t j = static_cast<uint32_t>(row / w.ny);
        const int32_t *cx = cells + static_cast<size_t>(3u * j) * n, *cy = cx + n, *cz = cy + n;
        uint32_t c = 0;
        for (uint32_t i = lane; i < n; i += 64u) {
            int32_t x = cx[i] + ix, y = cy[i] + iy;
            const int32_t z = cz[i];
            x = (x < 0 && x > lowest) ? 0 : x, y = (y < 0 && y > lowest) ? 0 : y;
            if (static_cast<uint32_t>(x) < static_cast<uint32_t>(g.dims[0]) && static_cast<uint32_t>(y) < static_cast<uint32_t>(g.dims[1]) &&
                static_cast<uint32_t>(z) < static_cast<uint32_t>(g.dims[2]))
                c += (level_bits[(static_cast<size_t>(z) * g.dims[1] + y) * g.wx + (static_cast<uint32_t>(x) >> 5)] >> (x & 31)) & 1u;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0u) hits[k] = c;
    }
}

}  // namespace kicp
