// kicp_map_kernels.hpp -- the two kernels of kicp_map.hip, neither of them map maintenance (that is kicp_mapdev.hpp, kicp_map_update.hip): the scatter of a delta
// upload's staged rows and the batch GetClosestNeighbor.  `static __global__`: a unit that includes this header emits both, so only
// kicp_map.hip, which launches them, does.
#pragma once
#include <cfloat>

#include "kicp_common.hpp"
#include "kicp_nn_exact.hpp"

namespace kicp {

// ------------------------------------------------------------------------------------------------------------
// delta upload of the map mirror: scatter staged rows (8-byte words) to their places
//   row r of `staged` (row_words uint2 each) goes to dst + index[r] * row_words
// ------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_scatter_rows(const uint2 *__restrict__ staged, const uint32_t *__restrict__ index, uint32_t rows,
                                                      uint32_t row_words, uint2 *__restrict__ dst) {
    const size_t total = static_cast<size_t>(rows) * row_words;
    for (size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; e < total; e += static_cast<size_t>(gridDim.x) * 256) {
        const uint32_t r = static_cast<uint32_t>(e / row_words), w = static_cast<uint32_t>(e % row_words);
        dst[static_cast<size_t>(index[r]) * row_words + w] = staged[e];
    }
}

// ------------------------------------------------------------------------------------------------------------
// GetClosestNeighbor for a batch (API parity; same search code as the fused kernel, no acceptance bound)
// ------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_closest(const double *__restrict__ queries, uint32_t n, const MapView m,
                                                 double *__restrict__ out_nn, double *__restrict__ out_dist) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Query q;
    make_query(q, queries[3 * i], queries[3 * i + 1], queries[3 * i + 2], m.voxel_size);
    double best = DBL_MAX;
    uint32_t best_idx = 0xFFFFFFFFu;
    search_global(m, q, best, best_idx);
    if (best_idx == 0xFFFFFFFFu) {
        out_nn[3 * i] = out_nn[3 * i + 1] = out_nn[3 * i + 2] = 0.0;
        out_dist[i] = DBL_MAX;
    } else {
        const double *t = m.pool + static_cast<size_t>(best_idx) * 3;
        out_nn[3 * i] = t[0], out_nn[3 * i + 1] = t[1], out_nn[3 * i + 2] = t[2];
        out_dist[i] = sqrt(best);
    }
}

}  // namespace kicp
