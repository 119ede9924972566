// kicp_pre_shared.hpp -- what the pre-steps' kernel headers (kicp_pre.hpp, kicp_pre_ingest.hpp, kicp_pre_egress.hpp) and the host
// code behind them (kicp_pre_internal.hpp) agree on: the store that hands results to other queues, the number of pieces the frame
// travels back in, and the words of the two small records every kernel of a frame reports through.  No kernels.
#pragma once
#include "kicp_common.hpp"

namespace kicp {

// A store that goes THROUGH the L2 to memory (relaxed, device scope: an sc1 store on gfx950).  What a workgroup hands to kernels of
// other queues - or to the host - before its launch has ended is written this way, followed by `s_waitcnt vmcnt(0)` and the
// workgroup's ticket: no release fence.  A fence writes the whole L2 back, and a few hundred of them per frame - one per workgroup
// of the ingest, the push and the last gather - slowed every kernel running beside them two- to fourfold (profiles/r06: the
// second-level replay 14 -> 48 us).
__device__ __forceinline__ void store_through(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_through(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

constexpr int kPushPieces = 8;  // pieces of the frame's way back (kicp_pre_egress.hpp): a ticket in HBM and a flag in host memory each

// THE WORDS OF d_misc (kicp_pre::d_misc, uint32 in HBM; the kernels index it with these numbers)
//   [0] survivor count of a single step (k_compact, k_downsample_gather)   [1] range error, sticky until the host has reported it
//   [2] longest robin-hood probe of the last downsample                   [3] ticket of the chain's last launch
//   [4] [5] [6] the chain's three counts n0, n1, n2                       [7] the chain's table-size guess was wrong
//   [8] == the chain's seq: a claim of k_frame_pre gave up (table A too small for the frame)
constexpr int kMiscTotal = 0, kMiscError = 1, kMiscProbe = 2, kMiscCounts = 4, kMiscWords = 16;
// THE WORDS OF h_rec (kicp_pre::h_rec, uint64 in host-coherent pinned memory; kernels write, the host polls)
//   [0..4]   the chain's record, each (seq << 32) | value: n0, n1, n2, longest probe, flags (1 range error, 2 guess wrong)
//   [5]      (seq << 32) | n2 once buffer 2's copy in host memory is complete (k_frame_src_host)
//   [8..10]  this call's ingest record: min key, max key, seq; [11] a scan's kept beams (k_ingest_scan)
//   [12..14] the look-ahead's ingest record
//   [16..23] the pushed frame's piece flags, each (seq << 32) | bytes of the piece (k_push_frame*)
constexpr int kRecChain = 0, kRecSrcHost = 5, kRecIngest = 8, kRecIngestStride = 4, kRecPush = 16, kRecWords = 32;
static_assert(kRecPush + kPushPieces <= kRecWords, "the piece flags fit the record");

}  // namespace kicp
