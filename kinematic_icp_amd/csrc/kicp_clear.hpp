// kicp_clear.hpp -- the kernels of the grid's clearance and costmap (kicp_grid_clearance, kicp_grid_costmap; C-ABI: kicp_grid_plan.hip,
// arithmetic: kicp_clear_host.hpp).  The squared distance to the nearest source within R cells is separable, so two launches on the
// grid's stream make a result for a rectangle of cells:
//   k_clear_columns  over the rectangle grown by R in x and clipped: one lane per column, so a wave reads 64 consecutive counter pairs
//                    of a row.  A workgroup owns 256 columns of a strip of rows and sweeps it twice, up from R rows below the strip
//                    and down from R rows above it, carrying the distance to the last source met.  The class of a cell comes straight
//                    from its counters (grid_readout, clear_class): no occupancy plane is written first.  The second sweep reads what
//                    the first stored - each lane its own bytes - and knows a source of the strip by its 0.  Output: a byte per cell,
//                    the column distance, 255 for none within R.
//   k_clear_rows     one workgroup per row and 256-cell segment: the column distances of the segment and R cells on either side go
//                    into LDS (at most 764 bytes), each lane scans outwards from its cell (clear_row_scan) and stores the clearance as
//                    16 bits, or - the costmap - looks its class up again from its counters, the cost in the caller's table (65 KB at
//                    most, read by every lane: it stays in cache) and stores a byte.
// THE TRANSIENT PLANE (kicp_grid_use_transients): both kernels take a bool template parameter kPlane and a pointer to a byte per cell.
// With kPlane a cell whose byte is 1 is a source in the columns' sweep and has the source's class in the costmap's lookup, whatever its
// counters say; without it the pointer is never read and the code is what it was before the plane existed.
// No atomics, no floating point, no scratch.  Both grids are one-dimensional: a column of 2^28 cells has more strips than a grid's y
// dimension admits.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_clear_host.hpp"

namespace kicp {

constexpr uint32_t kClearBlock = 256;
static_assert(kClearBlock == kClearSegment, "one lane per cell of a segment");

template <bool kPlane>
static __device__ __forceinline__ bool clear_source_at(const uint32_t *__restrict__ pairs, const uint8_t *__restrict__ plane, size_t cell, const ClearParams &p) {
    const uint32_t pair = pairs[cell];
    const bool source = clear_is_source(clear_class(grid_readout(pair & 0xFFFFu, pair >> 16, p.min_observations), p.source_min), p.unknown_is_obstacle);
    if constexpr (kPlane)
        return source || plane[cell] != 0u;
    else
        return source;
}

// coldist: r.h rows of cw bytes, column cx0 + i of the grid at byte i; blockIdx.x = strip * col_blocks + block of 256 columns;
// strip s holds the rows r.y0 + s * strip_rows .. of the rectangle
template <bool kPlane>
static __global__ __launch_bounds__(kClearBlock) void k_clear_columns(const uint16_t *__restrict__ counts, uint32_t width, uint32_t height, ClearParams p, ClearRect r,
                                                                      uint32_t cx0, uint32_t cw, uint32_t strip_rows, uint32_t col_blocks, uint8_t *coldist,
                                                                      const uint8_t *__restrict__ plane) {
    const uint32_t col = (blockIdx.x % col_blocks) * kClearBlock + threadIdx.x;
    if (col >= cw) return;
    const uint32_t *pairs = reinterpret_cast<const uint32_t *>(counts);
    const uint32_t x = cx0 + col, end = r.y0 + r.h;  // <= height <= 2^28
    const uint32_t ys = r.y0 + (blockIdx.x / col_blocks) * strip_rows, ye = ys + strip_rows < end ? ys + strip_rows : end;
    const uint32_t lo = ys > p.radius ? ys - p.radius : 0u, hi = ye + p.radius < height ? ye + p.radius : height;
    uint32_t d = kClearNone;
    for (uint32_t y = lo; y < ye; ++y) {
        d = clear_sweep(d, clear_source_at<kPlane>(pairs, plane, static_cast<size_t>(y) * width + x, p));
        if (y >= ys) coldist[static_cast<size_t>(y - r.y0) * cw + col] = static_cast<uint8_t>(d);
    }
    d = kClearNone;
    for (uint32_t y = hi; y-- > ys;) {
        if (y >= ye) {
            d = clear_sweep(d, clear_source_at<kPlane>(pairs, plane, static_cast<size_t>(y) * width + x, p));
            continue;
        }
        uint8_t *o = coldist + static_cast<size_t>(y - r.y0) * cw + col;
        const uint32_t down = *o;
        d = clear_sweep(d, down == 0u);
        const uint32_t m = down < d ? down : d;
        *o = static_cast<uint8_t>(m > p.radius ? kClearNone : m);
    }
}

// blockIdx.x = row * segments + segment; out: r.h rows of r.w values, 16 bits each (the clearance) or 8 (kCost: the cost)
template <bool kCost, bool kPlane>
static __global__ __launch_bounds__(kClearBlock) void k_clear_rows(const uint8_t *__restrict__ coldist, uint32_t cx0, uint32_t cw, const uint16_t *__restrict__ counts,
                                                                   uint32_t width, ClearParams p, ClearRect r, uint32_t segments, const uint8_t *__restrict__ table,
                                                                   uint32_t inflate_unknown, void *__restrict__ out, const uint8_t *__restrict__ plane) {
    __shared__ uint8_t g[kClearSegment + 2 * kClearMaxRadius];
    const uint32_t row = blockIdx.x / segments, first = r.x0 + (blockIdx.x % segments) * kClearSegment;  // the segment's first cell
    const uint8_t *line = coldist + static_cast<size_t>(row) * cw;
    for (uint32_t i = threadIdx.x; i < kClearSegment + 2u * p.radius; i += kClearBlock) {
        const int64_t c = static_cast<int64_t>(first) + i - p.radius - cx0;  // the column's byte in `line`
        g[i] = (c >= 0 && c < static_cast<int64_t>(cw)) ? line[c] : static_cast<uint8_t>(kClearNone);
    }
    __syncthreads();
    const uint32_t x = first + threadIdx.x;
    if (x >= r.x0 + r.w) return;
    const uint32_t c = clear_row_scan(g + p.radius + threadIdx.x, p.radius);
    const size_t at = static_cast<size_t>(row) * r.w + (x - r.x0);
    if constexpr (kCost) {
        const size_t cell = static_cast<size_t>(r.y0 + row) * width + x;
        const uint32_t pair = reinterpret_cast<const uint32_t *>(counts)[cell];
        uint32_t cls = clear_class(grid_readout(pair & 0xFFFFu, pair >> 16, p.min_observations), p.source_min);
        if constexpr (kPlane) cls = plane[cell] != 0u ? static_cast<uint32_t>(kClearSource) : cls;
        static_cast<uint8_t *>(out)[at] = clear_cost(cls, p.unknown_is_obstacle, table[c], inflate_unknown);
    } else {
        static_cast<uint16_t *>(out)[at] = static_cast<uint16_t>(c);
    }
}

}  // namespace kicp
