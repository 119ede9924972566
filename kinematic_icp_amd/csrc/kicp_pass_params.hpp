// kicp_pass_params.hpp -- what the host fills in for a pass kernel and what it reads back: the kernel arguments (PassParams with its
// SolveParams and SearchParams, JobsParams), the records and rows of the hand-offs (HostRecord, IcpState, the peer mailboxes' layout, the
// groups' accumulators) and the constants both sides share.  No kernel and no search or reduction code: a host unit that only fills in
// or reads these includes this header alone.  (The only device functions here are dbg_is / dbg_not, the two one-line readers of the
// kDbgBuild switch that sit next to it.)  The pass kernels themselves: kicp_kernels.hpp, which says which header holds what.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kicp_common.hpp"
#include "kicp_se3.hpp"

namespace kicp {

constexpr int kNumSums = 7;           // JTJ00 JTJ01 JTJ11 JTr0 JTr1 ssq count
constexpr int kNumLimbs = 3 * kNumSums;
constexpr int kReduceWords = 24;      // all-reduce payload: 21 limb sums + padding (int64)
constexpr double kFixScale = 1099511627776.0;  // 2^40
constexpr double kFixLimit = 8796093022208.0;  // 2^43: |term| must stay below this (source points within ~2900 km of the base frame)

// Result record in host-mapped pinned memory, polled by the host: the totals of a pass that does not hand over group rows.
struct HostRecord {
    unsigned long long seq;  // (call id << 16) | (0x8000: kicp_pass_sums) | passes completed; written last, behind the payload
    double sums[kNumSums];   // k_publish_sums, for kicp_pass_sums
    uint32_t gave_up;        // set by a resident workgroup that left without a command: counts of a round that never completed may be
                             // left in the groups' accumulators (clear_stale_tickets)
    long long words[kReduceWords];  // limb totals of the last pass (k_publish_words, the peer hand-offs)
};

// What a handle keeps on the device between the kernels of a pass.  (At least 24 bytes, whatever is in them: an empty scan's idle
// lanes read "point 0" out of this block - flight_launch, run_batch_resident.)
struct IcpState {
    long long reduce[kReduceWords];      // limb totals of the last pass (HandOff::Totals; multi-GPU: all-reduced in place)
    unsigned int pad_[16];
    unsigned int ticket;                 // second-level arrival counter (own cache line)
    unsigned int pad2_[31];
};
static_assert(sizeof(IcpState) >= 24 && offsetof(IcpState, ticket) % 128 == 0 && sizeof(IcpState) - offsetof(IcpState, ticket) == 128, "see above");

// What the per-correspondence terms need of the pose (Registration.cpp:86-93,108-113), the same for every
// correspondence of a pass: J.col(0) = R UnitX = c0 and J.col(1) = R (-s.y, s.x, 0) = -s.y c0 + s.x c1 with c1 = R UnitY, and the
// fixed-point term of JTJ(0,0) = |c0|^2, which every correspondence adds unchanged.  Computed ONCE per pass - by the host, next to
// the pose it sends (set_pose), or by the kernel where the pose comes from the device (resident kernels: the command line; pose
// lists) - by this one function, so that every kernel and the host see the same doubles.
struct PassBasis {
    double c0x, c0y, c0z, c1x, c1y, c1z;
    int jtj00[4];  // to_fixed(|c0|^2): four signed 21-bit limbs (= 2^40 exactly for any unit quaternion)
};
// How a pass hands its exact sums on (finish_pass).  The host adds what it gets and solves; the pose of EVERY launched pass is the
// host's and travels in the kernel arguments (pose0, basis) - resident kernels take later poses from their command line.
// (The values are the ones finish_pass has always compared against, so that its code stays instruction for instruction what
// it was: profiles/solve_residue_census.txt.  Every launch sets the member; a zero-initialised PassParams names no hand-off.)
enum class HandOff : int32_t {
    // Default (single GPU, shared segment, job lists): the reduction stops at the first-level groups of kGroup workgroups, whose
    // tagged rows go straight to the host (pub_rows), which adds them - two dependent device-scope round trips instead of six.
    // (Sending every workgroup's row was tried and is far slower: writes into host memory cost ~130 ns per transaction.)
    GroupRows = 4,
    // Two reduction levels; the last workgroup of the launch leaves the limb totals in st->reduce for what follows on the stream: a
    // collective (RCCL, caller's all-reduce) and k_publish_words, or k_publish_sums (kicp_pass_sums / kicp_pass_words).
    Totals = 3,
    // Peer mailboxes (multi-GPU without a collective library), launches of at most kP2pMaxGroups groups: the
    // last workgroup of every first-level group writes the group's row - tagged - into slot `p2p_rank` of EVERY rank's mailbox
    // (its own included; the peers' are IPC mappings of their HBM, reached over xGMI), and the last workgroup of group 0 adds ALL
    // ranks' group rows, in rank and group order, as they arrive and hands the node-wide totals to its host (pub_words, pub_seq).
    PeerGroupRows = 6,
    // Peer mailboxes, larger launches: two reduction levels as for Totals, then the launch's total travels as a SINGLE row of the
    // same format, so ranks on either side of the limit still pair up.
    PeerSingleRow = 7,
};
struct SolveParams {
    Pose pose0;
    PassBasis basis;  // of pose0 (set_pose)
    HandOff mode;
    HostRecord *rec;  // device pointer to the host-mapped record (the small-scan kernels set its gave_up word)
    // where the peer hand-offs put the node-wide totals (host-mapped memory: the handle's own record): 24 limb words, then the
    // sequence word set to pub_value
    long long *pub_words;
    unsigned long long *pub_seq;
    unsigned long long pub_value;
    // GroupRows: every first-level group's row, each word carrying the 16-bit tag of this pass; the host adds the rows as they arrive
    unsigned long long *pub_rows;  // host-mapped [groups][kReduceWords]
    uint32_t tag;                  // 1..65535, unique per pass within an epoch (the buffers are cleared when it wraps)
    // the peer hand-offs
    unsigned long long *const *p2p_peers;  // device array [p2p_nranks]: every rank's mailbox as seen from this GPU
    int32_t p2p_nranks, p2p_rank;
    uint32_t p2p_tag;     // 1..65535 (step % 65535 + 1); double-buffered by p2p_parity, so a stale slot can never match
    uint32_t p2p_parity;  // step & 1
    long long p2p_timeout_ticks;  // 100 MHz ticks a rank waits for its peers' slots (derived from the host's KICP_WAIT_TIMEOUT_S)
};
// a rank's mailbox: first [2 parities][nranks][kP2pWords] words that no kernel of this version touches (an earlier wire format's
// totals as tagged halves; the area stays so that the rows below are where every build expects them)
constexpr int kP2pWords = 2 * 24;
constexpr int kP2pMaxRanks = 16;
// ... followed by the rows of the peer hand-offs: [2 parities][nranks][kP2pMaxGroups] rows of 24 tagged words (value << 16 | tag,
// like the host's group rows) - the first-level GROUP rows of every rank, written by the groups' last workgroups themselves
constexpr int kP2pMaxGroups = 32;  // <= 1024 workgroups per rank and launch; larger launches send their total as one row (PeerSingleRow)
constexpr int kP2pCountWord = 23;  // word of a row that carries the sender's group count (padding in the single-GPU layout)
KICP_HD size_t p2p_rows_offset(int nranks) { return 2 * static_cast<size_t>(nranks) * kP2pWords; }
KICP_HD size_t p2p_box_words(int nranks) { return p2p_rows_offset(nranks) + 2 * static_cast<size_t>(nranks) * kP2pMaxGroups * 24; }

// Wave-uniform numbers of the pre-selection over the 16-bit mirror, computed once per call on the host (search_params()).
struct SearchParams {
    double bound;    // tau^2 (1 + 9.1e-13): acceptance bound on exact squared distances
    double upm;      // mirror units per metre = 65536 / voxel_size
    double inv_vs;   // 1 / voxel_size (voxel_coord's fast path)
    float bound_u;   // the bound in units^2, widened by the margin
    float margin_u;  // error margin of one decision between two mirror distances, units^2
    double tau2_lo, tau2_hi;  // tau^2 (1 -+ 2^-49): below / above, `sqrt(d2) < tau` is decided without taking the root (accepted_by_norm)
};
KICP_HD SearchParams search_params(double tau, double vs) {
    SearchParams sp;
    sp.bound = tau * tau * (1.0 + 9.1e-13);
    sp.upm = mirror_units_per_metre(vs);
    sp.inv_vs = 1.0 / vs;
    sp.tau2_lo = tau * tau * (1.0 - 1.7763568394002505e-15), sp.tau2_hi = tau * tau * (1.0 + 1.7763568394002505e-15);
    // error model in metres (k_pass_gather32): |delta| <= sqrt(3) * 1.05 units = 2.78e-5 vs; D off by <= 2 sqrt(D) |delta| +
    // |delta|^2 + 4.2e-6 D; both candidates of a decision, 10 % spare; D <= min(bound, 12 vs^2)
    const double bcap = fmin(sp.bound, 12.0 * vs * vs);
    const double margin = 2.2 * (5.55e-5 * sqrt(bcap) * vs + 4.2e-6 * bcap + 7.7e-10 * vs * vs);
    sp.margin_u = static_cast<float>(margin * sp.upm * sp.upm) * 1.00001f;
    sp.bound_u = static_cast<float>(sp.bound * sp.upm * sp.upm) * 1.00001f + sp.margin_u;
    return sp;
}

struct PassParams {
    const double *src;  // scan points, base frame, AoS xyz fp64 (device)
    uint32_t n;
    MapView map;
    double tau;
    SearchParams search;  // = search_params(tau, map.voxel_size)
    IcpState *st;
    unsigned long long *partials;  // [(grid + ceil(grid/32)) * 24] limb rows of the workgroups, then of the groups
    unsigned int *tickets;         // first-level arrival counters, one per group, 128 B apart, zero between launches
    unsigned long long *group_acc; // resident kernels: the groups' counting accumulators (finish_pass, ROWS_ONLY), zero between passes
    SolveParams sol;
    int32_t dbg;          // ablation switches for tools/dbg_census.py (0 = normal operation); read by the DBG build only (dbg_is)
    // blocks of 256 queries a workgroup of the one-lane-per-query four-waves build serves before its ONE epilogue (0 and 1: one block;
    // at most kMaxPassTiles; the grid is then ceil(blocks / tiles) workgroups).  Read by that build only (pass_tiles_loop).
    uint32_t tiles;
    // kicp_pass_correspondences (the EXPORT instantiations of the pass kernels only; nullptr otherwise): what DataAssociation appends
    // for query i (Registration.cpp:73-77) - the chosen map point's index in the pool (-1: no correspondence), its squared distance
    // to T * source[i] and its coordinates
    int32_t *corr_index;
    double *corr_d2, *corr_nn;
};
// The ablation / attribution switches (`dbg`, tools/gpu_dbg.py, tools/ab_option.py, bench.py's floor and rounds census) exist in
// libkicp_amd_dbg.so only (make dbg: -DKICP_DBG_BUILD).  In the production library every test below is a compile-time constant:
// the pass kernels carry no branch, no scalar load and no register for them (round 6; they cost the issue-bound kernel SALU work).
#ifdef KICP_DBG_BUILD
constexpr bool kDbgBuild = true;
#else
constexpr bool kDbgBuild = false;
#endif
__device__ __forceinline__ bool dbg_is(const PassParams &p, int v) { return kDbgBuild && p.dbg == v; }
__device__ __forceinline__ bool dbg_not(const PassParams &p, int v) { return !kDbgBuild || p.dbg != v; }

// The reduction's layout as both sides see it (finish_pass, kicp_pass_finish.hpp; the host's buffers and waits, kicp_reg_launch.hip)
constexpr int kGroup = 32;        // workgroups per first-level group
constexpr int kTicketStride = 32; // uint32 words between group tickets (128 B)
constexpr int kAccStride = 32;                // 64-bit words between the groups' counting accumulators (256 B: one memory channel)
constexpr int kAccCountShift = 56;            // a word of an accumulator: contributions so far << 56 | sum of the biased words
constexpr long long kAccBias = 1ll << 41;     // makes a row word (|value| < 2^40) non-negative; 32 of them stay below 2^47

// `row_tag` (tagged rows): the tag of this pass - p.sol.tag for a kernel that runs one pass, tag0 + pass for the resident
// kernel.  `gave_up` (resident kernel): this workgroup saw no command in time and hands over empty sums; the group row's flag
// word counts such workgroups in its upper half (kGaveUpUnit each) so that the host repeats the pass in a fresh launch.
constexpr unsigned long long kGaveUpUnit = 1ull << 16;
// A group's reader gives a row this long to land (100 MHz ticks = 2 s: rows arrive within microseconds of the ticket that
// announced them; anything longer is a lost workgroup).  It then hands over what it has, marked kLostRowUnit in the flag word, and
// the host repeats the pass (resident kernel) or fails the call - instead of a wave spinning on the device for ever.
constexpr unsigned long long kLostRowUnit = 1ull << 8;
constexpr long long kRowWaitTicks = 200000000ll;

// k_pass_gather32_jobs: ONE launch serves the passes of up to kMaxJobs scans (the batch path, run_batch_groups) on a 2-D grid -
// blockIdx.y is the job, blockIdx.x the workgroup inside that job's scan.  Every job brings its whole PassParams (scan, pose and
// basis, pass, tag, its own accumulators and host rows; map, search numbers and tau are the same in all of them), read from the
// kernarg segment with scalar loads where they are used, exactly as a single launch reads its one block; nblocks[j] = the
// workgroups of job j (gridDim.x is the largest of them).
constexpr int kMaxJobs = 8;
struct JobsParams {
    uint32_t nblocks[kMaxJobs];
    PassParams job[kMaxJobs];
};
static_assert(offsetof(JobsParams, job) == kMaxJobs * sizeof(uint32_t), "job_args: the jobs follow the counts without padding");

}  // namespace kicp
