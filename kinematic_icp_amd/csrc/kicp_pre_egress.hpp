// kicp_pre_egress.hpp -- the kernels that bring the pre-steps' results back to the caller; included by kicp_pre_egress.hip alone.
#pragma once
#include "kicp_common.hpp"
#include "kicp_pre_shared.hpp"

namespace kicp {

// ---- the preprocessed frame on its way back to the caller (pipeline/KinematicICP.cpp:84 returns it) ------------------------
// 3 MB that nothing on the device waits for.  A kernel on a stream of its own PUSHES buffer 0 into host-mapped pinned memory, 16 bytes
// per lane (PCIe writes: ~46 GB/s with 64 workgroups, tools/micro/d2h.hip; the DMA engine reaches that only in ONE piece, and every
// piece it is cut into costs ~10 us of API calls and engine start-up), piece by piece: the workgroup that completes a piece says so
// in host memory - (seq << 32) | bytes of the piece -, and the handle's helper thread copies that piece into the caller's vector
// while the next ones are still crossing PCIe.  The point count is read on the device (the launch is queued before the host knows it).
// (kPushPieces: kicp_pre_shared.hpp)
struct PushParams {
    const unsigned char *src;       // buffer 0
    unsigned char *dst;             // pinned landing area as the device sees it
    const uint32_t *n_points;       // the chain's survivor count (misc[4])
    uint32_t piece_bytes;           // a multiple of 16; kPushPieces pieces cover the largest frame the handle holds
    unsigned long long *tickets;    // [kPushPieces] device counters, never reset
    unsigned long long ticket_done; // their value once this launch's last workgroup has drawn
    unsigned long long *host_flags; // [kPushPieces] pinned
    uint32_t seq;
};
static __global__ __launch_bounds__(256) void k_push_frame(const PushParams q) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __shared__ uint32_t s_last;
    const size_t bytes = static_cast<size_t>(*q.n_points) * 24u;
    for (int piece = 0; piece < kPushPieces; ++piece) {
        const size_t lo = static_cast<size_t>(piece) * q.piece_bytes, hi = lo + q.piece_bytes < bytes ? lo + q.piece_bytes : bytes;
        const size_t len = hi > lo ? hi - lo : 0u;
        for (size_t o = (static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x) * 16u; o < len; o += static_cast<size_t>(gridDim.x) * 4096u) {
            if (o + 16u <= len) *reinterpret_cast<u32x4 *>(q.dst + lo + o) = *reinterpret_cast<const u32x4 *>(q.src + lo + o);
            else
                for (size_t k = o; k < len; ++k) q.dst[lo + k] = q.src[lo + k];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            // system scope: this workgroup's bytes are in host memory before its ticket - and so before the flag, whoever writes it
            // (without the fence the flag of another workgroup overtook the bytes: measured)
            // (a timing run WITHOUT this fence left the launches beside the push as slow as with it: the fence is not what they pay for)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            s_last = __hip_atomic_fetch_add(q.tickets + piece, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == q.ticket_done ? 1u : 0u;
            if (s_last) __hip_atomic_store(q.host_flags + piece, (static_cast<unsigned long long>(q.seq) << 32) | static_cast<unsigned long long>(len), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
    }
}
// The same push with the frame narrowed on the way out (kicp_pre_frame_f32: the PointCloud2 `data` of the published frame,
// RosUtils.cpp:40-63).  x y z FLOAT32 records of 12 bytes are the fp64 frame's doubles one by one as floats, so a lane reads 32
// bytes (four doubles), narrows them with static_cast<float> (round to nearest even, subnormals kept, +-inf beyond the float
// range, signed zeros kept) and stores one 16-byte unit: half the bytes of k_push_frame cross PCIe.  piece_bytes counts
// record bytes; the flag protocol is k_push_frame's.
static __global__ __launch_bounds__(256) void k_push_frame_f32(const PushParams q) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    __shared__ uint32_t s_last;
    const size_t bytes = static_cast<size_t>(*q.n_points) * 12u;
    const double *src = reinterpret_cast<const double *>(q.src);
    float *dst = reinterpret_cast<float *>(q.dst);
    for (int piece = 0; piece < kPushPieces; ++piece) {
        const size_t lo = static_cast<size_t>(piece) * q.piece_bytes, hi = lo + q.piece_bytes < bytes ? lo + q.piece_bytes : bytes;
        const size_t len = hi > lo ? hi - lo : 0u;
        for (size_t o = (static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x) * 16u; o < len; o += static_cast<size_t>(gridDim.x) * 4096u) {
            const size_t w = (lo + o) / 4u;  // first word of the unit = index of its first double
            if (o + 16u <= len) {
                const f64x2 a = *reinterpret_cast<const f64x2 *>(src + w), b = *reinterpret_cast<const f64x2 *>(src + w + 2);
                *reinterpret_cast<f32x4 *>(dst + w) = f32x4{static_cast<float>(a.x), static_cast<float>(a.y), static_cast<float>(b.x), static_cast<float>(b.y)};
            } else {
                for (size_t k = w; k < (lo + len) / 4u; ++k) dst[k] = static_cast<float>(src[k]);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            // system scope: this workgroup's bytes are in host memory before its ticket - and so before the flag, whoever writes it
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            s_last = __hip_atomic_fetch_add(q.tickets + piece, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == q.ticket_done ? 1u : 0u;
            if (s_last) __hip_atomic_store(q.host_flags + piece, (static_cast<unsigned long long>(q.seq) << 32) | static_cast<unsigned long long>(len), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
    }
}
// kicp_pre_download_f32 of a buffer that has no copy in host memory: its doubles narrowed into HBM, then downloaded
static __global__ __launch_bounds__(256) void k_narrow_f32(const double *src, size_t words, float *dst) {
    for (size_t k = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; k < words; k += static_cast<size_t>(gridDim.x) * 256u) dst[k] = static_cast<float>(src[k]);
}

}  // namespace kicp
