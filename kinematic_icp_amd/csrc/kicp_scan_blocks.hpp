// kicp_scan_blocks.hpp -- the exclusive scan of per-workgroup counts that order-preserving compactions share: as a launch of its
// own (k_scan_blocks) or folded into the consumer (block_offset).  Included by the pre-steps (kicp_pre.hip) and by the map's
// Pointcloud() (kicp_map_cloud.hip): the one kernel header that two translation units include, so k_scan_blocks is emitted twice.
#pragma once
#include "kicp_common.hpp"

namespace kicp {

// exclusive scan of the per-block counts (one workgroup; up to 1024 * 64 blocks = 16.7M points)
static __global__ __launch_bounds__(1024) void k_scan_blocks(uint32_t *block_counts, uint32_t nblocks, uint32_t *total) {
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nblocks; b0 += 1024) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t c = b < nblocks ? block_counts[b] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (b < nblocks) block_counts[b] = before + incl - c;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}

// Offset of this workgroup's survivors = the sum of the counts of the workgroups before it, added up by the workgroup itself
// (256 threads, a strided share each): for the grids of a frame (<= kFusedScanBlocks workgroups) that is a few loads per thread
// and saves the separate scan kernel - a launch of one workgroup whose ~5 us were pure latency, three times per frame.  The last
// workgroup also leaves the grand total in *total.  `raw` == 0: the counts have been scanned already (k_scan_blocks: larger grids).
constexpr uint32_t kFusedScanBlocks = 4096;
__device__ __forceinline__ uint32_t block_offset(const uint32_t *counts, int raw, uint32_t *total) {
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_offset;
    const uint32_t b = blockIdx.x;
    if (!raw) return counts[b];
    uint32_t sum = 0u;
    for (uint32_t i = threadIdx.x; i < b; i += 256u) sum += counts[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        s_offset = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (total && b == gridDim.x - 1u) *total = s_offset + counts[b];
    }
    __syncthreads();
    return s_offset;
}

}  // namespace kicp
