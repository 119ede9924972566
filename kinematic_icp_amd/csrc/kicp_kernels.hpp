// kicp_kernels.hpp -- gfx950 (CDNA4, wave64) kernels of the registration hot path.
//
//   k_pass_*    : fused DataAssociation + ComputePerturbation reduction (+ the pass-0 sum of
//                 ComputeOdometryRegularization): registration/Registration.cpp:62-81, 83-118, 48-55, with
//                 kiss_icp::VoxelHashMap::GetClosestNeighbor (kiss-icp v1.2.0) inlined as ONE table
//                 probe + the scan of the neighbour buckets that can matter.  No correspondence list is materialised.
//                 One launch = one ICP iteration; every variant ends in finish_pass (exact reduction + hand-off).
//       k_pass_gather32 variant 3 (default): thread (or 2 / 4 sub-lanes) per query; the 16-bit mirror pre-selects (packed
//                      fp32 arithmetic, integer-key tournament), the winner and anything within the error margin of it
//                      are resolved in fp64.
//                      (Removed after losing every A/B: round 1's variants with the neighbourhoods staged in LDS per wave, and - in
//                      round 6 - the plain fp64 gather that served as the ablation's baseline; k_closest still runs the plain
//                      fp64 search, search_global, which is also the exact fallback of the mirror search.)
//   finish_pass : wave / workgroup reduction of the exact sums, then one of the four hand-offs (HandOff): tagged rows of the
//                 first-level groups for the host (default), the launch's totals left on the device for a collective or a
//                 publishing kernel, or the exchange over peer mailboxes.  The HOST adds what it gets and solves
//                 (Registration.cpp:119-125,159-167,181-184; HostLoop::step): no kernel solves or updates a pose.
//   k_closest   : GetClosestNeighbor for a batch of queries (API parity / tests; kicp_map_kernels.hpp).
//
// Roofline: gather + reduction, ~0.02 flop/B -> memory bound, no MFMA.
// Numerics: per-point arithmetic is fp64 in the reference's operation order (TU compiled with -ffp-contract=off),
// so NN decisions and per-correspondence terms equal the fp64 reference's.  The sums are accumulated EXACTLY:
// each term is rounded once to a multiple of 2^-40 and added as a 128-bit integer, so the result does not depend
// on summation order, kernel variant, binning order or the number of GPUs (bit-reproducible).
//
// Which header holds what (all in namespace kicp; this one includes the five and holds the pass kernels proper):
//   kicp_pass_params.hpp : what the host fills in and reads - PassParams, SolveParams, SearchParams, JobsParams, HandOff, HostRecord,
//                          IcpState, the mailbox layout, the reduction's constants, the kDbgBuild switch.  No search or reduction code.
//   kicp_pass_fixed.hpp  : the exact accumulation (I128, to_fixed, terms_to_fixed, Acc / ScoreAcc / PlanarAcc) and the
//                          per-correspondence terms (correspondence_terms, accumulate, basis_of)
//   kicp_nn_exact.hpp    : the plain fp64 search (Query, table_lookup*, scan_points, search_global, closer_by_norm, accepted_by_norm)
//   kicp_pass_finish.hpp : finish_pass and its helpers (sum_rows*, p2p_collect_rows, counting_hand_over), KICP_PASS_SHARED
//   kicp_pass_visit.hpp  : the mirror search (Best3, voxel_coord*, Probe, Lane, start_lane, cull_todo, the trips, query_from, visit_*)
//   here                 : the kernarg views, resolve_and_accumulate, gather32_pass, pass_tiles_loop, k_pass_gather32, k_pass_gather32_jobs
// The kernels that have nothing to do with a pass live with the one unit that launches them: k_closest and k_scatter_rows in
// kicp_map_kernels.hpp (kicp_map.hip), k_publish_words and k_publish_sums in kicp_reg_launch.hip, behind publish_words / publish_sums.
#pragma once
#include <cfloat>

#include "kicp_common.hpp"
#include "kicp_nn_exact.hpp"
#include "kicp_pass_finish.hpp"
#include "kicp_pass_fixed.hpp"
#include "kicp_pass_params.hpp"
#include "kicp_pass_tiles.hpp"
#include "kicp_pass_visit.hpp"
#include "kicp_se3.hpp"

namespace kicp {

// The kernel arguments as they lie in the kernarg segment, through an opaque copy of its address: what is read through this view is
// fetched (scalar loads, scalar cache) WHERE it is used instead of being loaded at the kernel's start and kept in scalar registers
// through the search - the pass kernels' sixteen words of basis pushed as many other values out into vector registers, and the
// four-waves build spilled.  Every pass kernel's first (or only) argument is its PassParams, at offset 0 (asserted next to SmallParams
// and ScoreParams, whose first member it is).
typedef const PassParams __attribute__((address_space(4))) *PassKernarg;
__device__ __forceinline__ const PassParams &args_at_point_of_use() {
    PassKernarg q = (PassKernarg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("; kernel arguments, re-read at the point of use" : "+s"(q));
    return *(const PassParams *)q;
}
// (k_pass_gather32_jobs reads its list of jobs, JobsParams - kicp_pass_params.hpp -, the same way)
typedef const JobsParams __attribute__((address_space(4))) *JobsKernarg;
__device__ __forceinline__ const PassParams &job_args(uint32_t job) {
    JobsKernarg q = (JobsKernarg)__builtin_amdgcn_kernarg_segment_ptr();
    return *(const PassParams *)&q->job[job];
}
__device__ __forceinline__ const PassParams &job_args_at_point_of_use(uint32_t job) {
    JobsKernarg q = (JobsKernarg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("; kernel arguments, re-read at the point of use" : "+s"(q));
    return *(const PassParams *)&q->job[job];
}
// exact resolution of a finished search: the winner (and whatever lies within the margin of it) re-evaluated in fp64, the
// reference's tie rule, the acceptance test and the per-correspondence terms (Registration.cpp:74-77, 86-93)
// HOST_POSE: T is the host's pose and the kernel arguments carry its basis (the launched passes: k_pass_gather32, k_pass_gather32_jobs);
// otherwise the kernel got T from the device (resident and small-scan kernels, the pose lists of k_score_poses / k_planar_poses) and the
// basis is formed here, from T
// EXPORT (kicp_pass_correspondences): the decision is also written out per query - index, squared distance, coordinates
__device__ __forceinline__ void export_correspondence(const PassParams &p, uint32_t i, uint32_t idx, double d2, double x, double y, double z) {
    p.corr_index[i] = idx == kNoIndex32 ? -1 : static_cast<int32_t>(idx);
    p.corr_d2[i] = idx == kNoIndex32 ? DBL_MAX : d2;
    p.corr_nn[3 * i] = x, p.corr_nn[3 * i + 1] = y, p.corr_nn[3 * i + 2] = z;
}
// ACC = ScoreAcc (k_score_poses): the same search result, resolution, tie rule and acceptance test; only what is kept of an accepted
// correspondence differs (its squared residual and the count - no basis, no Jacobian terms)
// ACC = PlanarAcc (k_planar_poses): likewise; the basis is formed here from T, as for a pass whose pose is the device's
// JOBS: the kernel arguments are a list of jobs and this workgroup's are those of job blockIdx.y (k_pass_gather32_jobs)
template <bool HOST_POSE, bool EXPORT = false, class ACC = Acc, bool JOBS = false>
__device__ __forceinline__ void resolve_and_accumulate(ACC &acc, const PassParams &p, const double *__restrict__ src, const Pose &T, uint32_t i,
                                                       const Best3 &t, const KeptQuery *kept = nullptr) {
    if (EXPORT && i != kNoIndex32) export_correspondence(p, i, kNoIndex32, 0.0, 0.0, 0.0, 0.0);  // (overwritten below when the query has a correspondence)
    if (i == kNoIndex32 || t.i1 == kNoIndex32 || (kDbgBuild && p.dbg != 0 && p.dbg != 9 && p.dbg != 11 && p.dbg != 12 && p.dbg != 13 && p.dbg != 14)) return;
    const MapView &m = p.map;
    const float margin = p.search.margin_u;
    Query q;
    if (kept) q = kept->q;
    else make_query_of(q, p, src, T, i);
    const double bound = p.search.bound;
    double best = bound;
    uint32_t best_idx = kNoIndex32;
    double wx = 0.0, wy = 0.0, wz = 0.0;  // the winner's coordinates, as far as they have passed through registers already
    bool have_winner = false;
    if (t.b3 - t.b1 <= margin && dbg_not(p, 9)) {  // three near-equal candidates: leave it to the exact fp64 search (dbg 9: experiment without it)
        // (which needs to look no farther than the pre-selected winner's exact distance)
        if (kept && !kept->voxel) {
            const double vs = m.voxel_size;
            q.vx = voxel_coord(q.x, vs, p.search.inv_vs), q.vy = voxel_coord(q.y, vs, p.search.inv_vs), q.vz = voxel_coord(q.z, vs, p.search.inv_vs);
        }
        const double *c1 = m.pool + static_cast<size_t>(t.i1) * 3;
        search_global(m, q, best, best_idx, exact_d2_of(c1[0], c1[1], c1[2], q));
    } else {
        const double *c1 = m.pool + static_cast<size_t>(t.i1) * 3;
        const double x1 = c1[0], y1 = c1[1], z1 = c1[2];
        const double d1 = exact_d2_of(x1, y1, z1, q);
        if (d1 < best) best = d1, best_idx = t.i1, wx = x1, wy = y1, wz = z1, have_winner = true;
        if (t.b2 - t.b1 <= margin && t.i2 != kNoIndex32) {
            const double *c2 = m.pool + static_cast<size_t>(t.i2) * 3;
            const double x2 = c2[0], y2 = c2[1], z2 = c2[2];
            const double d2 = exact_d2_of(x2, y2, z2, q);
            // the reference keeps the FIRST candidate (in visiting order) whose NORM attains the strict minimum: the later of
            // the two only replaces the earlier when its rounded square root is smaller (closer_by_norm)
            if (d2 < bound) {
                if (best_idx == kNoIndex32 || (t.o2 < t.o1 ? !closer_by_norm(d1, d2) : closer_by_norm(d2, d1)))
                    best = d2, best_idx = t.i2, wx = x2, wy = y2, wz = z2, have_winner = true;
            }
        }
    }
    if (best_idx != kNoIndex32 && accepted_by_norm(best, p.tau, p.search)) {  // `distance < max_correspondance_distance`, Registration.cpp:75
        if (!have_winner) {  // (found by the exact search)
            const double *tp = m.pool + static_cast<size_t>(best_idx) * 3;
            wx = tp[0], wy = tp[1], wz = tp[2];
        }
        if (EXPORT) export_correspondence(p, i, best_idx, best, wx, wy, wz);
        if constexpr (ACC::kKind == AccKind::Score) {
            accumulate(acc, q.x, q.y, q.z, wx, wy, wz);
        } else if constexpr (ACC::kKind == AccKind::Planar) {
            accumulate(acc, basis_of(T), kept ? kept->sx : src[3 * i], kept ? kept->sy : src[3 * i + 1], q.x, q.y, q.z, wx, wy, wz);
        } else {
            // The basis is taken up HERE, not carried through the search and the exact phase (sixteen registers: the four-waves build
            // spilled them).  HOST_POSE: `from_args` is the constant 1 and the basis is read from the kernarg segment at this point
            // rather than at the kernel's start (args_at_point_of_use).  Otherwise it is 0 behind an opaque scalar: the branch on it
            // is never taken and is what keeps the compiler from forming basis_of(T) ahead of the exact phase (without it
            // k_pass_small<256, 4, true> goes from 124 to 130 VGPRs and from four waves per SIMD to three).
            if (dbg_is(p, 13)) return;  // (attribution, tools/valu_attribution.sh: the exact phase without the terms)
            int from_args = __builtin_amdgcn_readfirstlane(HOST_POSE ? 1 : 0);
            if constexpr (!HOST_POSE) asm volatile("; the basis is taken up here" : "+s"(from_args));
            PassBasis B;
            if (from_args) B = JOBS ? job_args_at_point_of_use(blockIdx.y).sol.basis : args_at_point_of_use().sol.basis;
            else B = basis_of(T);
            // the untransformed source point again (L1 / L2 hit) unless the build kept it: cheaper than registers kept live through the search
            accumulate<!EXPORT>(acc, B, kept ? kept->sx : src[3 * i], kept ? kept->sy : src[3 * i + 1], q.x, q.y, q.z, wx, wy, wz);
        }
    }
}

// G consecutive lanes serve one query: the occupied neighbour voxels are dealt round-robin to the G sub-lanes, which
// halves/quarters each lane's dependent chain and multiplies the resident waves; the sub-lanes share their running
// minimum for culling and merge their records with shuffles at the end.  (Small scans: few waves, latency bound.)
// OCC = waves per SIMD the register allocation aims for: 4 (<= 128 VGPRs; what scans larger than the machine want) or 3
// (<= 168: the compiler keeps more values instead of recomputing them; for scans that do not fill three waves per SIMD).
// SPLIT (G == 2): the two sub-lanes of a query do not deal the neighbour voxels between them but share every bucket, ten
// points each.
// LAT (G == 1, built at two waves per SIMD): the latency-oriented build for scans that do not fill the machine beyond that
// (<= 131 072 points on 256 CUs) - two neighbour voxels per round (visit_two).
// the search and the exact phase of one pass for lane `tid` of workgroup blockIdx.x; `acc` receives the lane's terms
// (`src`, `n`: the scan - p.src / p.n for a kernel that serves one call, the current scan of a resident kernel that serves a batch)
// `park` (the four-waves build): BLOCK x kParkWords doubles of LDS in which a lane parks its transformed point and the two source
// coordinates the terms need while it searches - that build has no registers to keep them (128 VGPRs) and used to transform the
// source point a second time for the exact phase (~70 fp64 instructions and three loads per lane).
constexpr int kParkWords = 5;
constexpr int kLendJobs = 32;                     // voxels a wave's loaded queries can give away per round (gather32_pass)
constexpr int kLendWords = kLendJobs * (1 + 7 + 7);  // per wave: the jobs, the lent lanes' own records, the records they hand back
// HOST_POSE: T is the host's pose (kernel arguments) and p.sol.basis its basis; where the kernel got T from the device the basis
// is formed right before the exact phase, not kept through the search (resolve_and_accumulate).
template <bool HOST_POSE, int BLOCK, int G, bool SPLIT, bool LAT, bool PARK = false, bool EXPORT = false, class ACC = Acc, bool JOBS = false>
__device__ __forceinline__ void gather32_pass(const PassParams &p, const Pose &T, uint32_t tid, ACC &acc, const double *__restrict__ src, uint32_t n,
                                              uint32_t block, int *lend = nullptr, double *park = nullptr) {
    const MapView &m = p.map;
    const float margin = p.search.margin_u;
    const uint32_t gt = block * BLOCK + tid;  // (`block`: which BLOCK points of the scan this workgroup takes - blockIdx.x, or a resident kernel's turn)
    const uint32_t i = gt / G;
    const int sub = static_cast<int>(gt % G);
    const bool valid = i < n && dbg_not(p, 7) && dbg_not(p, 8);
    Lane L;
    KeptQuery kept;
    static_assert(!(LAT && PARK), "the latency-oriented build keeps the query in registers");
    // (the pass kernels' one-lane-per-query build whose idle lanes take over voxels has a first round of its own, see below; the
    // kernels that score poses through ACC share that build's register budget and have none to spare for it)
    constexpr bool kFirstRound = G == 1 && !LAT && PARK && ACC::kKind == AccKind::Pass;
    const bool first_round = kFirstRound && lend != nullptr && dbg_not(p, 11) && dbg_not(p, 15);
    uint32_t own_val = 0u;
    start_lane<kFirstRound>(L, p, src, T, i, valid, own_val, (LAT || PARK) ? &kept : nullptr);
    if (PARK) {
        park[0 * BLOCK + tid] = kept.q.x, park[1 * BLOCK + tid] = kept.q.y, park[2 * BLOCK + tid] = kept.q.z;
        park[3 * BLOCK + tid] = kept.sx, park[4 * BLOCK + tid] = kept.sy;
    }
    if (G > 1 && !SPLIT) {  // deal the set bits round-robin: the r-th occupied voxel goes to sub-lane r % G
        uint32_t rest = L.todo, mine = 0u;
        for (int r = 0; rest; ++r) {
            const uint32_t low = rest & (0u - rest);
            rest ^= low;
            if (r % G == sub) mine |= low;
        }
        L.todo = mine;
    }
    float cull = L.t.b1;  // running minimum shared by the G sub-lanes (culling only)
    uint32_t rounds = 0u;  // (wave-uniform; read by the dbg 10 census only)
    // THE FIRST ROUND of the lending build.  Every lane that visits anything in it does so with the record start_lane left, most
    // of them at their own voxel (bit 0: the first shift of the order), and nobody lends before round 2 - so the round is written
    // out for that case (visit_first) and skips what the generic round pays for nothing: cull_todo, the load of nb[0] behind the
    // probe, the merge into a record that holds nothing, and the lending round's copies of record and probe.
    // Without the cull a lane takes the first OCCUPIED voxel of the order: its own wherever that holds points (bit 0 is always
    // alive), else - a third of a 64-beam scan's queries: the own voxel empty, a halo entry - the first occupied neighbour, even
    // one that lies beyond the acceptance bound and that the cull would have dropped.  Such a visit is wasted but harmless: a culled
    // voxel can never hold the winner, a voxel visited needlessly cannot change the outcome, and the visiting order travels with
    // every candidate.  Every other bit is culled at the top of round 2 against a minimum that can only be sharper than the bound.
    // (Letting those lanes sit the round out instead costs a round for a third of the lanes: +14 % instructions, measured.)
    // (dbg 15: the in-process A/B switch of this round.)
    if (first_round && __any(L.todo != 0u)) {
        ++rounds;
        if (L.todo) {
            const int s = __ffs(L.todo) - 1;
            L.todo &= L.todo - 1u;
            visit_first(L.q, L.t, m, s, own_val, margin);
        }
        cull = L.t.b1;
    }
    while (__any(L.todo != 0u)) {
        ++rounds;
        // which of the 27 neighbours could still hold something within the margin of the current minimum
        L.todo = cull_todo(L, cull, margin);
        if (LAT) {
            if (L.todo) {
                const int s1 = __ffs(L.todo) - 1;
                L.todo &= L.todo - 1u;
                const bool has2 = L.todo != 0u;
                const int s2 = has2 ? __ffs(L.todo) - 1 : s1;
                L.todo &= L.todo - 1u;  // (0 stays 0; a second voxel that the first one's result rules out is dropped here - cull_todo would)
                visit_two(L.q, L.t, m, s1, s2, has2, has2 ? voxel_lower_bound(L.q, s2, margin) : 0.f, margin);
            }
        } else if (G == 1 && lend != nullptr && dbg_not(p, 11)) {  // (dbg 11: the in-process A/B switch of this, tools/ab_option.py)
            // One lane per query, one neighbour voxel per round - and every round costs the WAVE its ~430 instructions however few
            // lanes still have a voxel to see (cfg2: 100 % of the lanes in round 1, 42 % in round 2, 7 % in round 3, 5 % in round 4;
            // 3.0 rounds per wave).  So from the second round on, lanes with nothing to do take over voxels of the queries that
            // have more than one left: such a query gives away up to two voxels beyond the one it visits itself, job j goes to the
            // j-th idle lane (dealt through a few words of LDS), which fetches the query's probe by ds_bpermute, parks its own
            // record in LDS, visits the voxel with a fresh record and hands that record back through LDS to be merged.  The visiting
            // order travels with every candidate (Best3::o1 / o2), so the reference's first-minimum rule holds whoever did the
            // visiting; a voxel that a sharper minimum would have culled is visited needlessly but cannot change the outcome.
            const bool busy = L.todo != 0u;
            int s = 0;
            if (busy) s = __ffs(L.todo) - 1, L.todo &= L.todo - 1u;
            bool helps = false;
            int jobs = 0, job0 = 0, slot = 0;
            if (rounds > 1u) {
                // (every minimum of this round between operands cast to `int`: mixed int / unsigned arguments pick min(double, double))
                const int spare = min(2, static_cast<int>(__popc(L.todo)));
                const unsigned long long give1 = __ballot(spare >= 1), give2 = __ballot(spare >= 2), idle = __ballot(!busy);
                if (give1 != 0ull && idle != 0ull) {  // (wave-uniform)
                    const int lane = static_cast<int>(tid & 63u);
                    const unsigned long long below = (1ull << lane) - 1ull;
                    job0 = __popcll(give1 & below) + __popcll(give2 & below);
                    const int pairs = min(min(static_cast<int>(__popcll(give1) + __popcll(give2)), static_cast<int>(__popcll(idle))), kLendJobs);
                    slot = __popcll(idle & below);
                    helps = !busy && slot < pairs;
                    jobs = max(0, min(spare, pairs - job0));
                    for (int j = 0; j < jobs; ++j) {
                        const int sj = __ffs(L.todo) - 1;
                        L.todo &= L.todo - 1u;
                        lend[job0 + j] = lane | (sj << 8);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    int from = lane;
                    if (helps) {
                        const int e = lend[slot];
                        from = e & 63, s = e >> 8;
                    }
                    // every lane takes the probe the shuffle returns - its own from `from == lane`, the lender's where it helps: no select
                    // per word (all 64 lanes are active here: every condition around this block is wave-uniform)
                    L.q = Probe{__shfl(L.q.lx, from, 64), __shfl(L.q.ly, from, 64), __shfl(L.q.lz, from, 64), __shfl(L.q.slot0, from, 64)};
                    if (helps) {  // (a lane with nothing to do never needs its own probe again; its record waits in LDS)
                        int *keep = lend + kLendJobs + 7 * slot;
                        keep[0] = __float_as_int(L.t.b1), keep[1] = __float_as_int(L.t.b2), keep[2] = __float_as_int(L.t.b3);
                        keep[3] = static_cast<int>(L.t.i1), keep[4] = static_cast<int>(L.t.i2), keep[5] = static_cast<int>(L.t.o1), keep[6] = static_cast<int>(L.t.o2);
                        L.t = Best3{p.search.bound_u, p.search.bound_u, p.search.bound_u, kNoIndex32, kNoIndex32, 0u, 0u};
                    }
                }
            }
            if (busy || helps) visit_bucket<1, ACC::kKind != AccKind::Pass>(L.q, L.t, m, s, margin, 0);
            if (__any(helps)) {  // (wave-uniform) the lent lanes' records go home
                if (helps) {
                    int *back = lend + kLendJobs + 7 * kLendJobs + 7 * slot;
                    back[0] = __float_as_int(L.t.b1), back[1] = __float_as_int(L.t.b2), back[2] = __float_as_int(L.t.b3);
                    back[3] = static_cast<int>(L.t.i1), back[4] = static_cast<int>(L.t.i2), back[5] = static_cast<int>(L.t.o1), back[6] = static_cast<int>(L.t.o2);
                    const int *keep = lend + kLendJobs + 7 * slot;
                    L.t = Best3{__int_as_float(keep[0]), __int_as_float(keep[1]), __int_as_float(keep[2]), static_cast<uint32_t>(keep[3]), static_cast<uint32_t>(keep[4]),
                                static_cast<uint32_t>(keep[5]), static_cast<uint32_t>(keep[6])};
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (int j = 0; j < jobs; ++j) {
                    const int *back = lend + kLendJobs + 7 * kLendJobs + 7 * (job0 + j);
                    const Best3 o{__int_as_float(back[0]), __int_as_float(back[1]), __int_as_float(back[2]), static_cast<uint32_t>(back[3]), static_cast<uint32_t>(back[4]),
                                  static_cast<uint32_t>(back[5]), static_cast<uint32_t>(back[6])};
                    if (o.i1 != kNoIndex32) best3_merge(L.t, o);
                }
            }
        } else if (L.todo) {
            const int s = __ffs(L.todo) - 1;
            L.todo &= L.todo - 1u;
            visit_bucket<SPLIT ? 2 : 1, ACC::kKind != AccKind::Pass>(L.q, L.t, m, s, margin, SPLIT ? sub : 0);
        }
        cull = L.t.b1;
#pragma unroll
        for (int off = 1; off < G; off <<= 1) cull = fminf(cull, __shfl_xor(cull, off, 64));
    }
    // ---- merge the sub-lanes' records (butterfly: every sub-lane ends up with the query's record) ------------------------
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
        Best3 o;
        o.b1 = __shfl_xor(L.t.b1, off, 64), o.b2 = __shfl_xor(L.t.b2, off, 64), o.b3 = __shfl_xor(L.t.b3, off, 64);
        o.i1 = __shfl_xor(L.t.i1, off, 64), o.i2 = __shfl_xor(L.t.i2, off, 64), o.o1 = __shfl_xor(L.t.o1, off, 64), o.o2 = __shfl_xor(L.t.o2, off, 64);
        best3_merge(L.t, o);
    }
    // ---- exact resolution (one sub-lane per query) ----------------------------------------------------------------------
    if (PARK) {  // (a lane reads back what it wrote itself: no barrier)
        kept.q.x = park[0 * BLOCK + tid], kept.q.y = park[1 * BLOCK + tid], kept.q.z = park[2 * BLOCK + tid];
        kept.sx = park[3 * BLOCK + tid], kept.sy = park[4 * BLOCK + tid], kept.voxel = false;
    }
    if (sub == 0) {
        resolve_and_accumulate<HOST_POSE, EXPORT, ACC, JOBS>(acc, p, src, T, L.i, L.t, (LAT || PARK) ? &kept : nullptr);
    }
    // dbg 10 (bench.py's latency model): no correspondences are formed; the "count" sum carries the number of visiting rounds
    // this WAVE ran - its chain of dependent bucket visits - from lane 0 (as rounds x 2^40: limb 1 holds bits 21..41, limb 2 the rest)
    if constexpr (ACC::kKind == AccKind::Pass)
        if (dbg_is(p, 10) && (tid & 63u) == 0u) acc.limb[6 * kTermLimbs + 1] = static_cast<int>(rounds & 3u) << 19, acc.limb[6 * kTermLimbs + 2] = static_cast<int>(rounds >> 2);
}
// SEVERAL TILES PER WORKGROUP (the one-lane-per-query four-waves build: k_pass_gather32<256, 1, 4, false, false>, its EXPORT twin,
// k_pass_gather32_jobs).  The epilogue - the wave reduction of twenty limbs, the barrier, wave 0's section alone on its SIMD, 24
// atomics and a share of a group row the host collects - costs a workgroup the same however many queries it served, and the sums
// are exact integers: any dealing of the queries to workgroups gives the same 24 words.  So a workgroup searches p.tiles blocks of
// BLOCK queries, one after the other, and finishes ONCE.  Workgroup b of `nwg` takes blocks b, b + nwg, b + 2 nwg, ...: strided by
// the grid, so that (workgroups being dealt round-robin to the XCDs) a block stays on the XCD it ran on with one tile wherever nwg
// is a multiple of 8, and every workgroup's first tile is a full one.  The waves of a workgroup pass from tile to tile on their
// own: what a tile uses of the LDS is private to a wave (s_lend) or a lane (s_park, s_tile), so no barrier separates the tiles.
// Between tiles a lane's terms wait in LDS, `tile` = [20][BLOCK] ints: the limbs of the five sums that need a reduction are added
// there by ds_add_u32 (column `tid`: no bank conflict, no VALU instruction, no register held through the next search) and read back
// once for the single reduction.  The two other sums travel as the wave's number of correspondences (`holders`).  With one tile the
// terms stay in registers and the LDS array is not touched.
// Returns the wave's number of correspondences; `acc` holds the lane's limb sums (limbs 4 .. 23) and its range flag, OR-ed over the tiles.
constexpr int kTileLimbs = kWaveLimbs - 2 * kTermLimbs;  // (|R UnitX|^2 and the count need no per-lane sums: finish_pass, TILED)
template <int BLOCK, bool EXPORT, bool JOBS>
__device__ __forceinline__ int pass_tiles_loop(Acc &acc, int (*lend)[kLendWords], double *park, int (*tile)[BLOCK]) {
    const uint32_t tid = threadIdx.x;
    // (the wave's count and the lane's range flag wait in vector registers: the search leaves a few of those free and no scalar one)
    int holders = 0, range_error = 0;
    uint32_t block = blockIdx.x;
    for (;;) {
        asm volatile("; kept in vector registers through the tile" : "+v"(holders), "+v"(range_error));
        // Nothing of a tile's set-up may be carried from tile to tile in registers (the build has none to spare, scalar ones
        // included): the arguments and the pose are re-read from the kernarg segment and the lane index is taken up afresh, so
        // that the compiler cannot hoist what depends on them out of the loop and hold it through the search.
        const PassParams &pt = JOBS ? job_args_at_point_of_use(blockIdx.y) : args_at_point_of_use();
        const Pose T = pt.sol.pose0;
        uint32_t lane_id = tid;
        asm volatile("; a tile starts here" : "+v"(lane_id));
        Acc one{};
        gather32_pass<true, BLOCK, 1, false, false, true, EXPORT, Acc, JOBS>(pt, T, lane_id, one, pt.src, pt.n, block, &lend[lane_id / 64u][0], park);
        holders += __popcll(__ballot(one.limb[6 * kTermLimbs + 1] != 0));
        range_error |= one.range_error;
        // (all wave-uniform from here, and read where they are used: the job's or the launch's workgroups, the tiles of each, the scan's blocks)
        const PassParams &pe = JOBS ? job_args_at_point_of_use(blockIdx.y) : args_at_point_of_use();
        const uint32_t tiles = min(pe.tiles, static_cast<uint32_t>(kMaxPassTiles));
        if (tiles <= 1u) {  // the terms never leave the registers
            acc = one;
            break;
        }
        if (block == blockIdx.x) {
#pragma unroll
            for (int k = 0; k < kTileLimbs; ++k) tile[k][tid] = one.limb[kTermLimbs + k];
        } else {
#pragma unroll
            for (int k = 0; k < kTileLimbs; ++k) (void)__hip_atomic_fetch_add(&tile[k][tid], one.limb[kTermLimbs + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        const uint32_t nwg = JOBS ? ((JobsKernarg)__builtin_amdgcn_kernarg_segment_ptr())->nblocks[blockIdx.y] : gridDim.x;
        const uint32_t end = min((pe.n + BLOCK - 1) / BLOCK, blockIdx.x + tiles * nwg);
        block += nwg;
        if (block >= end) {  // (a lane reads back what it wrote itself: no barrier)
#pragma unroll
            for (int k = 0; k < kTileLimbs; ++k) acc.limb[kTermLimbs + k] = tile[k][tid];
            break;
        }
    }
    acc.range_error = range_error;
    return __builtin_amdgcn_readfirstlane(holders);
}
// the limbs of |R UnitX|^2 every correspondence of the pass adds (accumulate takes them from the same place)
template <bool JOBS>
__device__ __forceinline__ void pass_jtj00(int (&jtj)[kTermLimbs]) {
    const PassParams &p = JOBS ? job_args_at_point_of_use(blockIdx.y) : args_at_point_of_use();
#pragma unroll
    for (int k = 0; k < kTermLimbs; ++k) jtj[k] = p.sol.basis.jtj00[k];
}
template <int BLOCK, int G, int OCC, bool SPLIT, bool LAT = false, bool EXPORT = false>
__global__ __launch_bounds__(BLOCK, OCC) void k_pass_gather32(const PassParams p) {
    static_assert(!SPLIT || G == 2, "bucket sharing is written for pairs of lanes");
    static_assert(!LAT || G == 1, "the latency-oriented build serves one lane per query");
    KICP_PASS_SHARED(BLOCK)
    constexpr bool kLends = G == 1 && !SPLIT && !LAT;  // idle lanes take over voxels of loaded queries (gather32_pass)
    __shared__ int s_lend[kLends ? BLOCK / 64 : 1][kLendWords];
    __shared__ double s_park[kLends ? BLOCK * kParkWords : 1];
    Acc acc{};
    if constexpr (kLends) {  // the four-waves build: p.tiles blocks per workgroup
        __shared__ int s_tile[kTileLimbs][BLOCK];
        const int holders = pass_tiles_loop<BLOCK, EXPORT, false>(acc, s_lend, s_park, s_tile);
        int jtj[kTermLimbs];
        pass_jtj00<false>(jtj);
        __syncthreads();
        const PassParams &pf = args_at_point_of_use();  // (not `p`: its loads would be issued ahead of the loop and held through it)
        finish_pass<BLOCK, false, true>(acc, pf, s_red, &s_flag, pf.sol.tag, 0, 0u, gridDim.x, holders, jtj);
    } else {
        gather32_pass<true, BLOCK, G, SPLIT, LAT, kLends, EXPORT>(p, p.sol.pose0, threadIdx.x, acc, p.src, p.n, blockIdx.x, nullptr, s_park);
        if (BLOCK > 64) __syncthreads();
        finish_pass<BLOCK>(acc, p, s_red, &s_flag, p.sol.tag);
    }
}
// the four-waves build with one lane per query, for a list of jobs (JobsParams): every job's pose is its host's and its rows go to
// that host as group rows (HandOff::GroupRows), group by group, through the job's own accumulators.  A launch's grid is as wide as its largest job: the
// workgroups beyond a smaller job's end leave at once.
template <int BLOCK, int G, int OCC>
__global__ __launch_bounds__(BLOCK, OCC) void k_pass_gather32_jobs(const JobsParams) {
    static_assert(G == 1, "the job list serves the one-lane-per-query build");
    const uint32_t job = blockIdx.y;
    const uint32_t nblocks = ((JobsKernarg)__builtin_amdgcn_kernarg_segment_ptr())->nblocks[job];
    if (blockIdx.x >= nblocks) return;
    const PassParams &p = job_args(job);
    KICP_PASS_SHARED(BLOCK)
    __shared__ int s_lend[BLOCK / 64][kLendWords];
    __shared__ double s_park[BLOCK * kParkWords];
    __shared__ int s_tile[kTileLimbs][BLOCK];
    Acc acc{};
    // (`nblocks`: the job's workgroups, each of p.tiles blocks - a job list may mix tile counts)
    const int holders = pass_tiles_loop<BLOCK, false, true>(acc, s_lend, s_park, s_tile);
    int jtj[kTermLimbs];
    pass_jtj00<true>(jtj);
    __syncthreads();
    finish_pass<BLOCK, false, true>(acc, p, s_red, &s_flag, p.sol.tag, 0, 0u, nblocks, holders, jtj);
}

}  // namespace kicp
