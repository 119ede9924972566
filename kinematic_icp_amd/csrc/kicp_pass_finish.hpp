// kicp_pass_finish.hpp -- the epilogue every pass kernel ends in: the exact wave / workgroup reduction of a lane's limbs and one of the
// four hand-offs (HandOff, kicp_pass_params.hpp) - finish_pass with its helpers, and the LDS it works in (KICP_PASS_SHARED).  Nothing
// here searches: it shares no code with the visit (kicp_pass_visit.hpp) or the fp64 search (kicp_nn_exact.hpp).
#pragma once
#include "kicp_common.hpp"
#include "kicp_pass_fixed.hpp"
#include "kicp_pass_params.hpp"
#include "kicp_pass_tiles.hpp"

namespace kicp {

// (The solve + pose update - Registration.cpp:119-125, 159-167, 181-184 - is the host's: kicp_reg_internal.hpp HostLoop::step.  The device-side
//  twin that round 1 to 5 carried - the launch's last workgroup solving on one lane - lost every A/B and went in round 6.)
// Workgroup epilogue of every pass kernel: exact workgroup sum, then a last-arriver tree.  Default (HandOff::GroupRows): ONE level -
// the last workgroup of every group of kGroup sends the group's row, tagged, to the host.  Totals, PeerSingleRow: two levels, the
// last workgroup of the launch finishes the iteration.  Inter-workgroup traffic follows cdna_hip_programming.md
// Guideline 16 (form R1): payload as 8-byte write-through (sc1) stores, ONE relaxed agent-scope ticket atomic per
// workgroup, readers use sc1 loads; no fences, no same-line atomic fan-in (tickets live on separate 128-B lines).  The
// two-level hand-offs order payload before ticket with `s_waitcnt vmcnt(0)`; tagged rows need no ordering.
// (kGroup, kTicketStride, kAcc*, kGaveUpUnit, kLostRowUnit, kRowWaitTicks: kicp_pass_params.hpp - the host lays its buffers out by them)

__device__ __forceinline__ unsigned long long ld_sc1(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// lanes 0..47 cooperatively sum `count` <= kGroup rows of kReduceWords words; the totals end up in lanes 0..23.
// All loads of a lane are issued before the first is consumed (one round trip, not count/2 of them).
__device__ __forceinline__ long long sum_rows(const unsigned long long *rows, uint32_t count, int lane) {
    long long v = 0;
    if (lane < 2 * kReduceWords) {
        const int word = lane % kReduceWords;
        const uint32_t first = lane / kReduceWords;
        unsigned long long t[kGroup / 2];
#pragma unroll
        for (int u = 0; u < kGroup / 2; ++u) {
            const uint32_t j = first + 2 * u;
            t[u] = (j < count) ? ld_sc1(rows + static_cast<size_t>(j) * kReduceWords + word) : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kGroup / 2; ++u) v += static_cast<long long>(t[u]);
    }
    return v + __shfl_down(v, kReduceWords, 64);
}

// the same fold over tagged rows (word = value << 16 | tag).  Returns the sum of the values; `ok` tells whether
// every word carried `tag`, i.e. whether every row had landed (the caller retries otherwise).
__device__ __forceinline__ long long sum_rows_tagged(const unsigned long long *rows, uint32_t count, int lane, uint32_t tag, bool &ok) {
    long long v = 0;
    ok = true;
    if (lane < 2 * kReduceWords) {
        const int word = lane % kReduceWords;
        const uint32_t first = lane / kReduceWords;
        unsigned long long t[kGroup / 2];
#pragma unroll
        for (int u = 0; u < kGroup / 2; ++u) {
            const uint32_t j = first + 2 * u;
            t[u] = (j < count) ? ld_sc1(rows + static_cast<size_t>(j) * kReduceWords + word) : static_cast<unsigned long long>(tag);
        }
#pragma unroll
        for (int u = 0; u < kGroup / 2; ++u) {
            ok = ok && (static_cast<uint32_t>(t[u]) & 0xFFFFu) == tag;
            v += static_cast<long long>(t[u]) >> 16;
        }
    }
    return v + __shfl_down(v, kReduceWords, 64);
}

// HandOff::PeerGroupRows and PeerSingleRow, the collecting workgroup (wave 0): add every rank's group rows out of this rank's mailbox.  Lanes r < nranks first
// learn rank r's group count (word kP2pCountWord of its row 0); then all rows are fetched the way sum_rows_tagged does it - 48
// lanes, 16 loads each in flight, 32 rows per round over the flattened (rank, group) index - and re-fetched until every word
// carries the tag.  Returns the node-wide totals in lanes 0..23; lane kNumLimbs + 1 is set to 1 when a row did not arrive in time.
__device__ __forceinline__ long long p2p_collect_rows(const SolveParams &f, int lane) {
    const uint32_t nr = static_cast<uint32_t>(f.p2p_nranks), tag = f.p2p_tag;
    const unsigned long long *box = f.p2p_peers[f.p2p_rank] + p2p_rows_offset(f.p2p_nranks) +
                                    static_cast<size_t>(f.p2p_parity) * nr * kP2pMaxGroups * kReduceWords;
    const long long t0 = wall_clock64();
    int late = 0;
    uint32_t count = 0;
    if (static_cast<uint32_t>(lane) < nr) {
        for (;;) {
            const unsigned long long got = __hip_atomic_load(box + static_cast<size_t>(lane) * kP2pMaxGroups * kReduceWords + kP2pCountWord, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_SYSTEM);
            if ((static_cast<uint32_t>(got) & 0xFFFFu) == tag) {
                count = min(static_cast<uint32_t>(got >> 16), static_cast<uint32_t>(kP2pMaxGroups));
                break;
            }
            if (wall_clock64() - t0 > f.p2p_timeout_ticks) {
                late = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    late = __any(late) ? 1 : 0;
    uint32_t widest = count;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) widest = max(widest, static_cast<uint32_t>(__shfl_xor(static_cast<int>(widest), off, 64)));
    long long sum = 0;
    const int word = lane % kReduceWords;
    const uint32_t phase = static_cast<uint32_t>(lane / kReduceWords);  // lanes 0..23 take the even rows of a round, 24..47 the odd ones
    for (uint32_t v0 = 0; v0 < nr * widest && !late; v0 += kGroup) {
        for (;;) {
            bool ok = true;
            long long part = 0;
            unsigned long long t[kGroup / 2];
#pragma unroll
            for (int u = 0; u < kGroup / 2; ++u) {
                const uint32_t v = v0 + phase + 2 * u, r = v / widest, j = v % widest;  // (widest >= 1 here)
                const uint32_t rows_of_r = static_cast<uint32_t>(__shfl(static_cast<int>(count), static_cast<int>(min(r, nr - 1u)), 64));  // (every lane takes part)
                const bool want = lane < 2 * kReduceWords && r < nr && j < rows_of_r;
                t[u] = want ? __hip_atomic_load(box + (static_cast<size_t>(r) * kP2pMaxGroups + j) * kReduceWords + word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                            : static_cast<unsigned long long>(tag);
            }
#pragma unroll
            for (int u = 0; u < kGroup / 2; ++u) {
                ok = ok && (static_cast<uint32_t>(t[u]) & 0xFFFFu) == tag;
                part += static_cast<long long>(t[u]) >> 16;
            }
            if (__all(ok)) {
                sum += part;
                break;
            }
            if (wall_clock64() - t0 > f.p2p_timeout_ticks) {
                late = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    sum += __shfl_down(sum, kReduceWords, 64);
    if (lane == kP2pCountWord) sum = 0;  // (the counts are not part of the payload)
    if (lane == kNumLimbs + 1) sum = late;
    return sum;
}

// Sum of a 32-bit value over the wave with DPP adds only (no LDS crossbar): inclusive scan inside each row of 16 lanes
// (row_shr 1, 2, 4, 8; lanes shifted in from outside the row read 0), then lane 15 of row 0 / 2 is added to every lane of
// row 1 / 3 (row_bcast:15) and lane 31 to rows 2 and 3 (row_bcast:31).  LANE 63 holds the wave total.
__device__ __forceinline__ int wave_sum_to_lane63(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);
    return v;
}

// The hand-over of a workgroup's exact sums through its group's COUNTING ACCUMULATORS (wave 0; lanes 0..6 hold the row words
// of the seven sums): ONE round trip to the L2 and no reader.  Lane w < kReduceWords adds word w of the workgroup's row - biased to be
// non-negative, with a 1 in the count field above it - to word w of the group's accumulator.  The addition that finds the count at
// group size - 1 is the last one for that word: old value + own = the group's sum, which that lane hands to the host (and clears
// the word for the set's next turn).  Every word is completed by whichever workgroup happened to add to it last - not necessarily
// the same one for all 24 - and carries the pass tag, which is how the host tells a complete row anyway (wait_rows).
// `acc_set` / `row_set`: which of the launch's sets of accumulators / of host rows the pass uses (resident kernels: the pass's slot
// for both; an ordinary launch: the tag's parity for the accumulators, row set 0).  Round 4: the resident generic kernel; round 5:
// every launch whose group rows go to the host, and the small-scan kernels (kicp_small.hpp), whose every workgroup used to send a
// row of its own across PCIe.
// `nblocks`: the workgroups of the pass - the launch's (gridDim.x), or the job's where a launch serves several (k_pass_gather32_jobs).
// `l` (lanes 0..6): the three row words of the lane's sum - the canonical limbs of its 128-bit total (i128_to_limbs) or any other
// three words of magnitude below 2^40 with the same weighted sum (limb_sums_to_words).
__device__ __forceinline__ void counting_hand_over(const long long (&l)[3], int range_error, int gave_up, const PassParams &p, uint32_t row_tag, uint32_t acc_set,
                                                   uint32_t row_set, int lane, uint32_t nblocks = gridDim.x) {
    const uint32_t b = blockIdx.x, g = b / kGroup, ngroups = (nblocks + kGroup - 1) / kGroup;
    const int from = min(lane, kNumLimbs - 1) / 3;
    const long long a0 = __shfl(l[0], from, 64), a1 = __shfl(l[1], from, 64), a2 = __shfl(l[2], from, 64);
    long long word = lane % 3 == 0 ? a0 : (lane % 3 == 1 ? a1 : a2);
    if (lane >= kNumLimbs) word = lane == kNumLimbs ? static_cast<long long>(range_error) + (gave_up ? static_cast<long long>(kGaveUpUnit) : 0ll) : 0ll;
    if (lane < kReduceWords) {
        const uint32_t group_size = min(static_cast<uint32_t>(kGroup), nblocks - g * kGroup);
        unsigned long long *acc = p.group_acc + (static_cast<size_t>(acc_set) * ngroups + g) * kAccStride + lane;
        const unsigned long long mine = static_cast<unsigned long long>(word + kAccBias);  // |word| < 2^40: (0, 2^42)
        const unsigned long long old = __hip_atomic_fetch_add(acc, (1ull << kAccCountShift) + mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((old >> kAccCountShift) == group_size - 1u) {
            const long long total = static_cast<long long>((old & ((1ull << kAccCountShift) - 1ull)) + mine) - static_cast<long long>(group_size) * kAccBias;
            __hip_atomic_store(acc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.sol.pub_rows + (static_cast<size_t>(row_set) * ngroups + g) * kReduceWords + lane,
                               (static_cast<unsigned long long>(total) << 16) | static_cast<unsigned long long>(row_tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// the same for a caller that holds 128-bit totals (k_pass_wave: its lanes convert whole terms, there are no limb sums)
__device__ __forceinline__ void counting_hand_over(const I128 &t, int range_error, int gave_up, const PassParams &p, uint32_t row_tag, uint32_t acc_set,
                                                   uint32_t row_set, int lane, uint32_t nblocks = gridDim.x) {
    long long l[3] = {0ll, 0ll, 0ll};
    if (lane < kNumSums) i128_to_limbs(t, l);
    counting_hand_over(l, range_error, gave_up, p, row_tag, acc_set, row_set, lane, nblocks);
}
// Wave 0 after the workgroup's barrier: lane i < 7 adds the waves' sums of the four limbs of sum i (64-bit additions of int32
// values) and cuts them into the three row words (limb_sums_to_words).  No 128-bit arithmetic: the chain every workgroup's last
// wave runs alone is a dozen 64-bit operations.
template <int WAVES>
__device__ __forceinline__ void workgroup_row_words(const int (*s_red)[kWaveLimbs], int lane, long long (&l)[3]) {
    l[0] = l[1] = l[2] = 0ll;
    if (lane < kNumSums) {
        long long s[kTermLimbs] = {0ll, 0ll, 0ll, 0ll};
#pragma unroll
        for (int w = 0; w < WAVES; ++w)
#pragma unroll
            for (int k = 0; k < kTermLimbs; ++k) s[k] += s_red[w][kTermLimbs * lane + k];
        limb_sums_to_words(s[0], s[1], s[2], s[3], l);
    }
}

// ROWS_ONLY: the caller only ever hands over group rows (the resident kernel): none of the other hand-offs is compiled in.
// `parity` (resident kernel: pass & 1): workgroup rows, tickets and the groups' host rows are double-buffered by pass parity, so
// that what a workgroup writes for pass k + 1 - in particular the marked empty row of a workgroup that gave up waiting for the
// command of pass k + 1 - can never land on a row of pass k that its reader (the group's last workgroup, the host) has not
// consumed yet.  The buffer of parity (k + 1) & 1 last held pass k - 1, whose rows the host had added before it sent the command
// that started pass k.
// TILED (the kernels whose workgroups serve several tiles, pass_tiles_loop): `a` holds the lane's limb sums over its tiles,
// `holders` the number of correspondences the WAVE found in all of them (wave-uniform) and `jtj` the four limbs of |R UnitX|^2
// (PassBasis::jtj00, wave-uniform) - a lane may hold several correspondences, so the two shortcuts below take these instead of a ballot.
template <int BLOCK, bool ROWS_ONLY = false, bool TILED = false>
__device__ __forceinline__ void finish_pass(Acc &a, const PassParams &p, int (*s_red)[kWaveLimbs], int *s_flag, uint32_t row_tag, int gave_up = 0,
                                            uint32_t parity = 0u, uint32_t nblocks = gridDim.x, int holders = 0, const int *jtj = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    IcpState *st = p.st;
    if (!ROWS_ONLY && dbg_is(p, 8)) {  // ablation (tools/gpu_dbg.py): no reduction at all, workgroup 0 hands over zeros
        if (p.sol.mode == HandOff::GroupRows && wave == 0 && blockIdx.x % kGroup == 0 && lane < kReduceWords)
            __hip_atomic_store(p.sol.pub_rows + static_cast<size_t>(blockIdx.x / kGroup) * kReduceWords + lane, static_cast<unsigned long long>(p.sol.tag),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    // Every lane contributes at most ONE correspondence per tile and serves at most kMaxPassTiles of them, so each of its seven
    // sums is at most four terms (to_fixed): limbs of 21 bits each, below 2^23 per lane, and a wave's 64 values of a limb add up in int32.
    int range_error = a.range_error;
    int limb[kWaveLimbs];
    if (dbg_is(p, 10) || dbg_is(p, 12)) {  // (10, the census: the count's limbs carry something else; 12: the in-process A/B switch of what follows)
#pragma unroll
        for (int k = 0; k < kWaveLimbs; ++k) limb[k] = wave_sum_to_lane63(a.limb[k]);
    } else {
        // Two of the seven sums need no reduction.  The count: every correspondence adds 2^40 = limb 1 at 2^19, so the wave's sum is
        // the number of lanes that hold one.  |J.col(0)|^2 = |R UnitX|^2 depends on the pose alone: every correspondence adds the SAME
        // four limbs, so the wave's sum is that number times the limbs of any lane that holds one.  (Sums of identical integers:
        // exactly what the additions would give.)  TILED: the number is the caller's count over the wave's tiles, the limbs the basis'.
        int n_holders;
        if constexpr (TILED) {
            n_holders = holders;
#pragma unroll
            for (int k = 0; k < kTermLimbs; ++k) limb[k] = n_holders * jtj[k];
        } else {
            const unsigned long long held = __ballot(a.limb[6 * kTermLimbs + 1] != 0);
            n_holders = __popcll(held);
            const int some = held ? static_cast<int>(__ffsll(static_cast<long long>(held))) - 1 : 0;
#pragma unroll
            for (int k = 0; k < kTermLimbs; ++k) limb[k] = n_holders * __builtin_amdgcn_readlane(a.limb[k], some);
        }
        limb[6 * kTermLimbs] = 0, limb[6 * kTermLimbs + 1] = n_holders << 19, limb[6 * kTermLimbs + 2] = 0, limb[6 * kTermLimbs + 3] = 0;
        // The other twenty limbs: a reduction that HALVES the number of values a lane carries with every step it can - the lanes of a
        // pair keep one half each and take the partner's share of it (quad_perm), twice; then the quads of a row (row_shr 4, 8) and the
        // four rows (ds_bpermute) are added for the five values a lane is left with.  ~65 instead of 120 DPP additions; lane 60 + q
        // ends up with the wave's sums of limbs 4 j + q (j = 0 .. 4).
        int w10[10], x5[5];
        const bool p0 = (lane & 1) != 0, p1 = (lane & 2) != 0;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const int lo = a.limb[kTermLimbs + 2 * j], hi = a.limb[kTermLimbs + 2 * j + 1];
            w10[j] = (p0 ? hi : lo) + __builtin_amdgcn_update_dpp(0, p0 ? lo : hi, 0xB1, 0xF, 0xF, true);  // quad_perm [1, 0, 3, 2]
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int lo = w10[2 * j], hi = w10[2 * j + 1];
            x5[j] = (p1 ? hi : lo) + __builtin_amdgcn_update_dpp(0, p1 ? lo : hi, 0x4E, 0xF, 0xF, true);  // quad_perm [2, 3, 0, 1]
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) x5[j] += __builtin_amdgcn_update_dpp(0, x5[j], 0x114, 0xF, 0xF, true);  // row_shr 4
#pragma unroll
        for (int j = 0; j < 5; ++j) x5[j] += __builtin_amdgcn_update_dpp(0, x5[j], 0x118, 0xF, 0xF, true);  // row_shr 8: lanes 12 .. 15 of a row hold its sums
#pragma unroll
        for (int j = 0; j < 5; ++j) x5[j] += __shfl_up(x5[j], 16, 64);
#pragma unroll
        for (int j = 0; j < 5; ++j) x5[j] += __shfl_up(x5[j], 32, 64);
        range_error = __any(range_error) ? 1 : 0;
        if (lane >= 60) {
#pragma unroll
            for (int j = 0; j < 5; ++j) s_red[wave][kTermLimbs + 4 * j + (lane & 3)] = x5[j];
        }
        if (lane == 63) {
#pragma unroll
            for (int k = 0; k < kTermLimbs; ++k) s_red[wave][k] = limb[k], s_red[wave][6 * kTermLimbs + k] = limb[6 * kTermLimbs + k];
            if (range_error) atomicOr(s_flag, 2);
        }
    }
    if (dbg_is(p, 10) || dbg_is(p, 12)) {
        range_error = __any(range_error) ? 1 : 0;
        if (lane == 63) {
#pragma unroll
            for (int k = 0; k < kWaveLimbs; ++k) s_red[wave][k] = limb[k];
            if (range_error) atomicOr(s_flag, 2);
        }
    }
    __syncthreads();
    if (wave != 0) return;
    range_error = (*s_flag & 2) ? 1 : 0;
    // wave 0 only from here.
    const uint32_t b = blockIdx.x, g = b / kGroup, ngroups = (nblocks + kGroup - 1) / kGroup;
    // (an ordinary launch of HandOff::GroupRows - round 5: the accumulators alternate with the pass tag's parity, the host's row of group g stays
    //  where it was; dbg 14: round 4's rows -> ticket -> reload, for the in-process A/B)
    const bool counting = ROWS_ONLY || (p.sol.mode == HandOff::GroupRows && dbg_not(p, 14));
    if (!ROWS_ONLY && counting) parity = row_tag & 1u;
    if (counting) {  // lane i < 7: the three row words of sum i straight from the waves' limb sums
        long long l[3];
        workgroup_row_words<BLOCK / 64>(s_red, lane, l);
        counting_hand_over(l, range_error, gave_up, p, row_tag, parity, ROWS_ONLY ? parity : 0u, lane, nblocks);
        return;
    }
    // The other hand-offs: lane i < 7 takes the workgroup total of sum i (as a 128-bit integer) and publishes its three 40-bit limbs.
    I128 t{0ull, 0ll};
    if (lane < kNumSums) {
        for (int w = 0; w < BLOCK / 64; ++w)
            i128_add_limb_sums(t, s_red[w][kTermLimbs * lane], s_red[w][kTermLimbs * lane + 1], s_red[w][kTermLimbs * lane + 2], s_red[w][kTermLimbs * lane + 3]);
    }
    unsigned long long *const rows0 = p.partials + (ROWS_ONLY ? static_cast<size_t>(parity) * nblocks * kReduceWords : 0u);
    unsigned int *const tickets0 = p.tickets + (ROWS_ONLY ? static_cast<size_t>(parity) * ngroups * kTicketStride : 0u);
    unsigned long long *row = rows0 + static_cast<size_t>(b) * kReduceWords;
    if (ROWS_ONLY || p.sol.mode == HandOff::GroupRows || p.sol.mode == HandOff::PeerGroupRows) {
        // Tagged rows: no store acknowledgement is awaited anywhere.  The ticket only elects the group's reader; whether
        // a row has landed is visible in the row itself.  Values: limbs < 2^40 (the top limb is a small signed number
        // within the documented range), so value << 16 | tag fits a word, and so does the sum of a group's 32 rows.
        const unsigned long long tag = row_tag;
        if (lane < kNumSums) {
            long long l[3];
            i128_to_limbs(t, l);
#pragma unroll
            for (int j = 0; j < 3; ++j) st_sc1(row + 3 * lane + j, (static_cast<unsigned long long>(l[j]) << 16) | tag);
        } else if (lane < kNumSums + 3) {
            st_sc1(row + kNumLimbs + (lane - kNumSums),
                   ((lane == kNumSums ? static_cast<unsigned long long>(range_error) + (gave_up ? kGaveUpUnit : 0ull) : 0ull) << 16) | tag);
        }
        unsigned int ticket = 0;
        if (lane == 0) ticket = __hip_atomic_fetch_add(tickets0 + static_cast<size_t>(g) * kTicketStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ticket = __shfl(ticket, 0, 64);
        const uint32_t group_size = min(static_cast<uint32_t>(kGroup), nblocks - g * kGroup);
        if (ticket != group_size - 1) return;
        if (lane == 0) __hip_atomic_store(tickets0 + static_cast<size_t>(g) * kTicketStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long long total;
        bool ok;
        total = sum_rows_tagged(rows0 + static_cast<size_t>(g) * kGroup * kReduceWords, group_size, lane, static_cast<uint32_t>(tag), ok);
        if (!__all(ok)) {  // (rare: a row still on its way) re-read, bounded by wall-clock time
            const long long t0 = wall_clock64();
            bool lost = false;
            do {
                __builtin_amdgcn_s_sleep(1);
                total = sum_rows_tagged(rows0 + static_cast<size_t>(g) * kGroup * kReduceWords, group_size, lane, static_cast<uint32_t>(tag), ok);
                lost = wall_clock64() - t0 > kRowWaitTicks;
            } while (!__all(ok) && !lost);
            if (!__all(ok)) total = lane == kNumLimbs ? static_cast<long long>(kLostRowUnit) : 0ll;  // nothing of an incomplete sum is handed on
        }
        if (ROWS_ONLY || p.sol.mode == HandOff::GroupRows) {
            if (lane < kReduceWords)
                __hip_atomic_store(p.sol.pub_rows + (static_cast<size_t>(ROWS_ONLY ? parity * ngroups : 0u) + g) * kReduceWords + lane,
                                   (static_cast<unsigned long long>(total) << 16) | tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        // PeerGroupRows: the group's row goes into EVERY rank's mailbox (over xGMI for the peers'), tagged with the step
        const SolveParams &f = p.sol;
        if (lane < kReduceWords) {
            const unsigned long long value = lane == kP2pCountWord ? static_cast<unsigned long long>(ngroups) : static_cast<unsigned long long>(total);
            const unsigned long long w = (value << 16) | f.p2p_tag;
            const size_t at = p2p_rows_offset(f.p2p_nranks) + ((static_cast<size_t>(f.p2p_parity) * f.p2p_nranks + f.p2p_rank) * kP2pMaxGroups + g) * kReduceWords + lane;
            for (int r = 0; r < f.p2p_nranks; ++r) __hip_atomic_store(f.p2p_peers[r] + at, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (g != 0) return;
        // group 0's last workgroup collects for this rank and hands the node-wide totals to its host
        const long long all = p2p_collect_rows(f, lane);
        if (lane < kReduceWords) __hip_atomic_store(f.pub_words + lane, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(f.pub_seq, f.pub_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (lane < kNumSums) {
        long long l[3];
        i128_to_limbs(t, l);
#pragma unroll
        for (int j = 0; j < 3; ++j) st_sc1(row + 3 * lane + j, static_cast<unsigned long long>(l[j]));
    } else if (lane < kNumSums + 3) {
        st_sc1(row + kNumLimbs + (lane - kNumSums), lane == kNumSums ? static_cast<unsigned long long>(range_error) : 0ull);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned int ticket = 0;
    if (lane == 0) ticket = __hip_atomic_fetch_add(p.tickets + static_cast<size_t>(g) * kTicketStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __shfl(ticket, 0, 64);
    const uint32_t group_size = min(static_cast<uint32_t>(kGroup), nblocks - g * kGroup);
    if (ticket != group_size - 1) return;
    // ---- last workgroup of its group: fold the group's rows into one ---------------------------------------
    if (lane == 0) __hip_atomic_store(p.tickets + static_cast<size_t>(g) * kTicketStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long long total = sum_rows(p.partials + static_cast<size_t>(g) * kGroup * kReduceWords, group_size, lane);
    if (ngroups > 1) {
        unsigned long long *grow = p.partials + (static_cast<size_t>(nblocks) + g) * kReduceWords;
        if (lane < kReduceWords) st_sc1(grow + lane, static_cast<unsigned long long>(total));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) ticket = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ticket = __shfl(ticket, 0, 64);
        if (ticket != ngroups - 1) return;
        if (lane == 0) __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        total = 0;
        for (uint32_t base = 0; base < ngroups; base += kGroup)
            total += sum_rows(p.partials + (static_cast<size_t>(nblocks) + base) * kReduceWords, min(static_cast<uint32_t>(kGroup), ngroups - base), lane);
    }
    // ---- last workgroup of the launch ------------------------------------------------------------------------
    if (p.sol.mode == HandOff::PeerSingleRow) {
        // Group rows are what the ranks exchange (PeerGroupRows), but this launch has more groups than a rank's share of the mailbox
        // holds: its total travels as ONE row.  A row's words carry 48 bits, so the limb sums are brought back into limb range
        // first (lane 3i + j: limb j of sum i).
        const SolveParams &f = p.sol;
        const int i3 = 3 * (min(lane, kNumLimbs - 1) / 3);
        const unsigned long long a = static_cast<unsigned long long>(__shfl(total, i3, 64)), b = static_cast<unsigned long long>(__shfl(total, i3 + 1, 64));
        const long long c = __shfl(total, i3 + 2, 64);
        I128 t{a, 0ll};
        i128_add(t, I128{b << 40, static_cast<long long>(b >> 24)});  // (the two lower limb sums are non-negative)
        t.hi += c << 16;
        long long l[3];
        i128_to_limbs(t, l);
        const int j = lane % 3;
        long long word = j == 0 ? l[0] : (j == 1 ? l[1] : l[2]);
        if (lane >= kNumLimbs) word = lane == kNumLimbs ? (total != 0 ? 1 : 0) : 0;  // the range flag as 0 / 1
        if (lane < kReduceWords) {
            const unsigned long long value = lane == kP2pCountWord ? 1ull : static_cast<unsigned long long>(word);
            const unsigned long long w = (value << 16) | f.p2p_tag;
            const size_t at = p2p_rows_offset(f.p2p_nranks) + ((static_cast<size_t>(f.p2p_parity) * f.p2p_nranks + f.p2p_rank) * kP2pMaxGroups) * kReduceWords + lane;
            for (int r = 0; r < f.p2p_nranks; ++r) __hip_atomic_store(f.p2p_peers[r] + at, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        total = p2p_collect_rows(f, lane);
    }
    if (lane < kReduceWords) st->reduce[lane] = total;
    if (p.sol.mode == HandOff::PeerSingleRow) {  // hand the totals to the host: write-through stores, one wait, then the sequence word
        if (lane < kReduceWords) __hip_atomic_store(p.sol.pub_words + lane, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(p.sol.pub_seq, p.sol.pub_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// wave-uniform values belong in SGPRs: tell the compiler explicitly
__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uniform_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane(static_cast<int>(b)), hi = __builtin_amdgcn_readfirstlane(static_cast<int>(b >> 32));
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}
#define KICP_PASS_SHARED(BLOCK)                       \
    __shared__ int s_red[(BLOCK) / 64][kWaveLimbs];   \
    __shared__ int s_flag;                            \
    if (threadIdx.x == 0) s_flag = 0;

}  // namespace kicp
