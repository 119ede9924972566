// kicp_scroll.hpp -- the kernel that shifts a plane of cells (kicp_grid_scroll: the counter pairs and the transient plane,
// kicp_elev_scroll: the height columns; arithmetic: kicp_scroll_host.hpp).  Included by kicp_grid.hip and kicp_elev.hip.
//
// k_scroll_plane<T> copies from the live buffer into a spare one of the same size; the handle swaps the two afterwards.  Not in
// place: workgroups have no order, and for a small |dy| the source rows of one workgroup are the destination rows of another.  It is a
// copy and is built like one: a lane owns a CHUNK, 16 bytes of the destination at a 16-byte boundary - 4 counter pairs, 2 columns or
// 16 plane bytes - and stores it with one 16-byte store; lanes are consecutive along the flat index, so a wave writes 1 KiB in one
// piece, and the lanes stride over the chunks.  Flat indices, byte offsets and the loop are 64-bit: 2^28 columns are 2 GiB.
//   The source of a chunk is as contiguous as the chunk but only element-aligned (dx elements off).  A chunk that lies in one row and
//   whose sources all lie inside the plane reads its 16 bytes at once; one that lies in a row without sources stores zeros; every other
//   one - across a row end, at the plane's end, over the edge of the valid columns - resolves element by element, and the plane's
//   last chunk, where width * height is no multiple of the chunk, stores element by element too.
// No LDS, no scratch, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_common.hpp"
#include "kicp_scroll_host.hpp"

namespace kicp {

constexpr uint32_t kScrollBlock = 256;
constexpr uint32_t kScrollMaxBlocks = 1024;  // 4 MiB of destination per turn of the loop
constexpr uint32_t kScrollChunkBytes = 16;

// element k of a chunk's four words
template <class T>
static __device__ __forceinline__ void scroll_put(uint32_t (&w)[4], uint32_t k, T v) {
    static_assert(sizeof(T) == 1 || sizeof(T) == 4 || sizeof(T) == 8, "a plane byte, a counter pair or a column");
    if constexpr (sizeof(T) == 1) w[k >> 2] |= static_cast<uint32_t>(v) << (8u * (k & 3u));
    else if constexpr (sizeof(T) == 4) w[k] = static_cast<uint32_t>(v);
    else w[2u * k] = static_cast<uint32_t>(v), w[2u * k + 1u] = static_cast<uint32_t>(static_cast<unsigned long long>(v) >> 32);
}

template <class T>
static __global__ __launch_bounds__(kScrollBlock) void k_scroll_plane(const T *__restrict__ in, T *__restrict__ out, uint32_t width, uint32_t height, int32_t dx,
                                                                      int32_t dy) {
    constexpr uint32_t kPer = kScrollChunkBytes / sizeof(T);
    const uint64_t n = static_cast<uint64_t>(width) * height, chunks = (n + kPer - 1u) / kPer;
    const ScrollValid v = scroll_valid(width, height, dx, dy);
    const int64_t off = static_cast<int64_t>(dy) * static_cast<int64_t>(width) + dx;  // a destination's flat index + off = its source's
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kScrollBlock;
    for (uint64_t c = static_cast<uint64_t>(blockIdx.x) * kScrollBlock + threadIdx.x; c < chunks; c += stride) {
        const uint64_t e0 = c * kPer;
        const uint64_t iy = e0 / width, ix = e0 - iy * width;
        const bool full = e0 + kPer <= n, one_row = ix + kPer <= width;
        const bool row_valid = static_cast<int64_t>(iy) >= v.y0 && static_cast<int64_t>(iy) < v.y1;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (full && one_row && row_valid && static_cast<int64_t>(ix) >= v.x0 && static_cast<int64_t>(ix + kPer) <= v.x1) {
            const T *src = in + (static_cast<int64_t>(e0) + off);
            __builtin_memcpy(w, src, kScrollChunkBytes);  // aligned as T is, no more: one global_load_dwordx4 (element loads measured slower)
        } else if (!(full && one_row && !row_valid)) {  // (a full chunk in a row without sources keeps its zeros)
            uint64_t x = ix, y = iy;
#pragma unroll
            for (uint32_t k = 0; k < kPer; ++k) {
                const uint64_t e = e0 + k;
                if (e < n) {
                    const bool valid = static_cast<int64_t>(y) >= v.y0 && static_cast<int64_t>(y) < v.y1 && static_cast<int64_t>(x) >= v.x0 && static_cast<int64_t>(x) < v.x1;
                    const T value = valid ? in[static_cast<int64_t>(e) + off] : T(0);
                    if (full) scroll_put<T>(w, k, value);
                    else out[e] = value;
                }
                if (++x == width) x = 0, ++y;
            }
        }
        if (full) *reinterpret_cast<uint4 *>(out + e0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// how many workgroups a plane of n elements of T gets
template <class T>
inline uint32_t scroll_blocks(uint64_t n) {
    const uint64_t chunks = (n + kScrollChunkBytes / sizeof(T) - 1u) / (kScrollChunkBytes / sizeof(T));
    const uint64_t blocks = (chunks + kScrollBlock - 1u) / kScrollBlock;
    return static_cast<uint32_t>(blocks < kScrollMaxBlocks ? blocks : kScrollMaxBlocks);
}

}  // namespace kicp
