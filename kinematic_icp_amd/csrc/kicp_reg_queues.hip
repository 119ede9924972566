// kicp_reg_queues.hip -- batches with several scans in flight on queues of their own, sharded or not (see kicp_reg_internal.hpp)
#include "kicp_reg_internal.hpp"
#include "kicp_batch_groups.hpp"
#include "kicp_small.hpp"  // kCmd*, kPipeSlots, SmallParams

using namespace kicp;
using namespace kicp::host;

namespace kicp {
namespace host {
// kicp_register_device_batch, large scans: SEVERAL SCANS IN FLIGHT ON SEVERAL QUEUES, one host thread.  The scans of a batch do
// not depend on each other - every one starts from its own pose, the map does not change - so the call keeps option
// "batch_queues" of them going at a time (four while the option is at its default) - here, with a launch per scan and pass (what
// sharded, short and mostly-small batches and "batch_group" 1 run; run_batch_groups below is the same with several scans per
// launch) - each on a handle of its own (clones of the caller's, made on first use and
// kept): own HSA queue, own reduction scratch and rows.  Every pass is an ordinary launch of the pass kernel in its
// four-waves-per-SIMD build (the latency-oriented build fills the register file with ONE scan's waves and leaves no room for a
// second scan's next to them); the device takes workgroups from all queues as wave slots fall free, so a pass's slow workgroups
// no longer hold anything up - the next scan's workgroups fill the slots the fast ones have left - and the host's answer to one
// scan's rows (add, solve, next launch: ~2 us) is hidden behind the other scans' searches.  This thread goes round the scans in
// flight: rows complete -> Registration.cpp:119-125, 159-167, 184 on the host -> next pass or next scan.
// What kicp_register_device_concurrent does with a host thread per lane, done by one thread that never sleeps on a lane.
// Returns 1 when the batch is not one for this path (the caller goes on to run_batch_resident / the plain loop), else a kicp
// status; *done = scans completed from the front.
static_assert(kMaxBatchQueues == kicp_reg::kShmLanes, "a lane of a sharded batch call owns one area of the shared segment");
struct BatchFlight {
    kicp_reg *h = nullptr;
    HostLoop loop;
    PassParams pp{};     // large scans: the pass kernel's arguments
    SmallParams sp{};    // small scans (kicp_small.hpp): a launch that serves ONE pass and leaves
    SmallPlan pl;
    bool small = false;    // a small-scan kernel's launch ...
    bool own_rows = false; // ... whose workgroups send rows of their own ("small_group_rows" 0)
    size_t k = 0, rows = 0, row_next = 0;  // rows of the pass in flight: the groups' (large) / the workgroups' (small); how many are in
    uint32_t tag = 0;
    bool active = false;
    unsigned polls = 0;
    long long words[kReduceWords] = {};            // sums of the rows that are in (large scans: the reduce payload's layout)
    __int128 total[kNumSums] = {};                 // (small scans: two 48-bit halves per sum and row)
    unsigned long long flags = 0;
    Deadline since;
    // sharded batches: this lane's next scan (static deal), and - once this rank's rows are in - the hand-off it waits for
    size_t next = 0;
    bool at_peers = false;
    unsigned long long shm_value = 0;
    // sharded over RCCL: the pass ends in the device-side tree + ncclAllReduce + k_publish_words on the lane's stream; the record's
    // sequence word the host polls for
    bool via_comm = false;
    unsigned long long comm_seq = 0;
};
// the rows of a flight's pass that have arrived since the last look: 1 all in (sums in out_words), 0 not yet, < 0 error
int flight_rows(BatchFlight &f, long long out_words[kReduceWords]) {
    kicp_reg *h = f.h;
    if (f.via_comm) {  // the all-reduced totals arrive as ONE record behind the collective (k_publish_words)
        if (__atomic_load_n(&h->rec.get()->seq, __ATOMIC_ACQUIRE) != f.comm_seq) {
            if (++f.polls % 256u == 0u) {
                const hipError_t q = hipStreamQuery(h->stream);
                if (q != hipSuccess && q != hipErrorNotReady) return fail(KICP_ERR_HIP, std::string("stream fault: ") + hipGetErrorString(q));
                if (f.since.passed()) return fail(KICP_ERR_COMM, "timed out waiting for a lane's all-reduce (KICP_WAIT_TIMEOUT_S)");
            }
            return 0;
        }
        for (int i = 0; i < kReduceWords; ++i) out_words[i] = h->rec.get()->words[i];
        out_words[kNumLimbs] = out_words[kNumLimbs] != 0 ? 1 : 0;
        return 1;
    }
    const uint32_t tag = f.tag;
    const int row_words = f.own_rows ? kSmallRowWords : kReduceWords;
    for (; f.row_next < f.rows; ++f.row_next) {
        const unsigned long long *row = h->rows.get() + f.row_next * row_words;
        unsigned long long w[kReduceWords];
        bool ok = true;
        for (int i = 0; i < row_words; ++i) {
            w[i] = __atomic_load_n(row + i, __ATOMIC_RELAXED);
            ok = ok && (static_cast<uint32_t>(w[i]) & 0xFFFFu) == tag;
        }
        if (!ok) {
            if (++f.polls % 256u == 0u) {
                if (h->last_via_aql) {
                    if (h->aql.queue_error) return fail(KICP_ERR_HIP, "the AQL queue reported error " + std::to_string(h->aql.queue_error));
                } else {  // (the query makes the runtime flush commands it may still hold back, and reports device faults)
                    const hipError_t q = hipStreamQuery(h->stream);
                    if (q != hipSuccess && q != hipErrorNotReady) return fail(KICP_ERR_HIP, std::string("stream fault: ") + hipGetErrorString(q));
                }
                if (f.since.passed()) return fail(KICP_ERR_HIP, "timed out waiting for the pass kernel's rows (KICP_WAIT_TIMEOUT_S)");
            }
            return 0;
        }
        if (f.own_rows) {
            for (int i = 0; i < kNumSums; ++i)
                f.total[i] += static_cast<__int128>(w[2 * i] >> 16) + (static_cast<__int128>(static_cast<long long>(w[2 * i + 1]) >> 16) << 48);
            f.flags |= w[2 * kNumSums] >> 16;
        } else {
            for (int i = 0; i < kReduceWords; ++i)
                if (i != kNumLimbs) f.words[i] += static_cast<long long>(w[i]) >> 16;
            f.words[kNumLimbs] |= row_flags(static_cast<long long>(w[kNumLimbs]) >> 16);
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (f.own_rows) {  // (the layout of the all-reduce payload: three 40-bit limbs per sum, then the range flag - wait_rows_small)
        for (int i = 0; i < kReduceWords; ++i) out_words[i] = 0;
        const unsigned __int128 m40 = (static_cast<unsigned __int128>(1) << 40) - 1;
        for (int i = 0; i < kNumSums; ++i) {
            const unsigned __int128 u = static_cast<unsigned __int128>(f.total[i]);
            out_words[3 * i] = static_cast<long long>(u & m40), out_words[3 * i + 1] = static_cast<long long>((u >> 40) & m40);
            out_words[3 * i + 2] = static_cast<long long>(f.total[i] >> 80);
        }
        out_words[kNumLimbs] = (f.flags & 1ull) ? 1 : 0;
    } else {
        for (int i = 0; i < kReduceWords; ++i) out_words[i] = f.words[i];
    }
    return 1;
}
int flight_launch(BatchFlight &f, const kicp_map *map, const double *d_frame, size_t n, double tau) {
    kicp_reg *h = f.h;
    f.pl = h->use_small ? small_plan(h, n) : SmallPlan();
    f.small = f.pl.grid != 0 && !f.pl.generic;
    f.row_next = 0, f.flags = 0, f.polls = 0;
    for (auto &w : f.words) w = 0;
    for (auto &t : f.total) t = 0;
    PassParams &pp = f.small ? f.sp.p : f.pp;
    if (n == 0) d_frame = reinterpret_cast<const double *>(h->d_state.get());  // (an empty shard: the one workgroup's lanes are all idle, but an idle lane still reads point 0)
    fill_pass(pp, h, map, d_frame, n, tau, search_params(tau, map->mirror.view.voxel_size));
    SolveParams &sol = pp.sol;
    set_pose(sol, f.loop.T);
    sol.mode = HandOff::GroupRows;
    f.own_rows = f.small && !grouped_rows(h, f.pl, false);
    if (f.small) {  // one wave per query / sub-lanes per query; the launch serves this pass only
        if (f.own_rows) {  // every workgroup's row goes straight to the host
            f.rows = f.pl.grid;
            if (int rc = ensure_rows(h, (f.rows * kSmallRowWords + kReduceWords - 1) / kReduceWords)) return rc;
        } else {  // one row per group of 32 workgroups (counting accumulators)
            f.rows = (f.pl.grid + kGroup - 1) / kGroup;
            if (int rc = ensure_partials(h, kPipeSlots * f.pl.grid)) return rc;
            if (int rc = ensure_rows(h, kPipeSlots * f.rows)) return rc;
            if (int rc = clear_stale_tickets(h)) return rc;
            pp.group_acc = h->d_group_acc.get(), sol.pub_rows = h->rows.dev(), sol.rec = h->rec.dev();
        }
        if (int rc = ensure_cmd(h)) return rc;
        if (int rc = next_tag(h, &f.tag)) return rc;
        SmallParams &sp = f.sp;
        sp.group_rows = f.own_rows ? 0 : 1;
        sp.cmd = h->cmd.dev(), sp.rows = h->rows.dev(), sp.cmd_dev = h->d_cmd_copies, sp.relay = (h->small_cmd == 1 && h->cmd_bar) ? 0 : 1;
        sp.timeout_ticks = 5000, sp.trace = nullptr, sp.scans = nullptr, sp.rotate = 0;
        sp.tag0 = f.tag, sp.max_passes = 1, sp.seq_base = h->cmd_seq;
        h->cmd_seq += 1;
        f.since = Deadline();
        return launch_small(h, sp, f.pl);
    }
    const uint32_t grid = pass_grid(h, n);
    f.rows = (grid + kGroup - 1) / kGroup;
    if (int rc = ensure_partials(h, grid)) return rc;
    if (int rc = ensure_rows(h, f.rows)) return rc;
    if (int rc = clear_stale_tickets(h)) return rc;  // (nothing to do unless an earlier call left a pass uncollected)
    pp.partials = h->d_partials.get(), pp.tickets = h->d_tickets.get(), pp.group_acc = h->d_group_acc.get();
    sol.rec = h->rec.dev(), sol.pub_rows = h->rows.dev();
    if (int rc = next_tag(h, &sol.tag)) return rc;
    f.tag = sol.tag;
    f.since = Deadline();
    if (f.via_comm) {  // device-side tree -> all-reduce on the lane's communicator -> the totals to the host, all on the lane's stream
        sol.mode = HandOff::Totals;
        const unsigned long long call_id = ++h->call_id;
        f.comm_seq = (call_id << 16) | static_cast<unsigned long long>(f.loop.iter + 1);
        if (int rc = launch_pass(h, pp, false)) return rc;
        if (int rc = enqueue_allreduce(h)) return rc;
        publish_words(h->stream, h->d_state.get(), h->rec.dev(), call_id, f.loop.iter);
        HIP_TRY(hipGetLastError());
        return KICP_OK;
    }
    return launch_pass(h, pp, true);
}
// SEVERAL SCANS PER LAUNCH (option "batch_group" = G > 1; unsharded batches).  The first passes of a batch's scans depend on nothing
// the host computes during the call, and a dispatch per scan pays for its own fill and drain of the device, its own packet, kernarg
// slot and doorbell, and a turn-round of the host on its queue.  So a lane - a queue with this thread behind it, batch_queues / G of
// them - launches GROUPS of up to G jobs in one dispatch of k_pass_gather32_jobs (2-D grid: blockIdx.y = the job), a job being the
// next pass of one scan: its own PassParams, tag, accumulators and host rows (slot s of the lane's buffers).  The lane adds the
// jobs' rows as they land and runs HostLoop::step per job; when the group is collected, the scans that go on and fresh ones from
// the front of the batch (BatchGroups, kicp_batch_groups.hpp) make the next group.  Scans that take another kernel - the small-scan
// kernels, sub-lanes per query - keep their launch per scan and pass (flight_launch) in between.  Bit-equal to one call per scan:
// the same kernel body on the same arguments, exact integer sums.
struct GroupJob {
    size_t k = 0;  // the scan
    HostLoop loop;
    uint32_t tag = 0;
    size_t rows = 0, row_next = 0;  // group rows of the pass in flight; how many are in
    long long words[kReduceWords] = {};
    bool collected = false, goes_on = false;
};
struct GroupLane {
    BatchFlight solo;  // (also holds the lane's handle)
    std::vector<GroupJob> jobs;
    bool active = false, is_solo = false;
    size_t pending = 0;  // jobs of the group whose rows are not all in yet
    unsigned polls = 0;
    Deadline since;
    JobsParams jp;
};
static int group_launch(kicp_reg *r, GroupLane &L, int group, size_t slot_groups, const kicp_map *map, const double *const *d_frames, const size_t *n, double tau) {
    kicp_reg *h = L.solo.h;
    const size_t slots = static_cast<size_t>(group);
    if (int rc = ensure_partials(h, slots * slot_groups * kGroup)) return rc;
    if (int rc = ensure_rows(h, slots * slot_groups)) return rc;
    if (int rc = clear_stale_tickets(h)) return rc;
    uint32_t tag0 = 0, grid_x = 0;
    if (int rc = next_tag_range(h, static_cast<uint32_t>(L.jobs.size()), &tag0)) return rc;
    const SearchParams search = search_params(tau, map->mirror.view.voxel_size);
    for (size_t s = 0; s < L.jobs.size(); ++s) {
        GroupJob &j = L.jobs[s];
        PassParams &pp = L.jp.job[s];
        pp = PassParams{};
        fill_pass(pp, h, map, d_frames[j.k], n[j.k], tau, search);
        // (a job's group rows leave through its counting accumulators only - the rows -> ticket -> reload hand-over, "dbg" 14, keeps a
        //  launch per scan - so a job has no workgroup rows and no tickets: a slot's share of them would not hold grid + groups rows)
        pp.partials = nullptr, pp.tickets = nullptr;
        pp.group_acc = h->d_group_acc.get() + s * 2 * slot_groups * kAccStride;
        SolveParams &sol = pp.sol;
        set_pose(sol, j.loop.T);
        sol.mode = HandOff::GroupRows;
        sol.rec = h->rec.dev(), sol.pub_rows = h->rows.dev() + s * slot_groups * kReduceWords;
        sol.tag = j.tag = tag0 + static_cast<uint32_t>(s);
        pp.tiles = pass_tiles(h, n[j.k], true);  // (per job: a list may mix tile counts)
        const uint32_t grid = pass_grid(h, n[j.k], true);
        L.jp.nblocks[s] = grid, grid_x = std::max(grid_x, grid);
        j.rows = (grid + kGroup - 1) / kGroup, j.row_next = 0, j.collected = false, j.goes_on = false;
        for (auto &w : j.words) w = 0;
    }
    L.pending = L.jobs.size(), L.polls = 0, L.since = Deadline();
    ++r->batch_group_launches;
    if (int rc = launch_jobs(h, L.jp, static_cast<uint32_t>(L.jobs.size()), grid_x)) return rc;
    if (h->last_via_aql) ++r->batch_group_aql_launches;
    return KICP_OK;
}
// the rows of job `s` that have arrived since the last look: 1 all in (sums in j.words), 0 not yet
static int group_job_rows(GroupLane &L, size_t s, size_t slot_groups) {
    GroupJob &j = L.jobs[s];
    const unsigned long long *base = L.solo.h->rows.get() + s * slot_groups * kReduceWords;
    for (; j.row_next < j.rows; ++j.row_next) {
        const unsigned long long *row = base + j.row_next * kReduceWords;
        unsigned long long w[kReduceWords];
        bool ok = true;
        for (int i = 0; i < kReduceWords; ++i) {
            w[i] = __atomic_load_n(row + i, __ATOMIC_RELAXED);
            ok = ok && (static_cast<uint32_t>(w[i]) & 0xFFFFu) == j.tag;
        }
        if (!ok) return 0;
        for (int i = 0; i < kReduceWords; ++i)
            if (i != kNumLimbs) j.words[i] += static_cast<long long>(w[i]) >> 16;
        j.words[kNumLimbs] |= row_flags(static_cast<long long>(w[kNumLimbs]) >> 16);
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return 1;
}
static int run_batch_groups(kicp_reg *r, kicp_map *map, size_t count, const double *const *d_frames, const size_t *n, const double *last_poses_qt,
                            const double *rel_odoms_qt, double tau, double *out_poses_qt, int *out_iterations, size_t *done, int *worst, int lanes, int group) {
    std::vector<GroupLane> L(static_cast<size_t>(lanes));
    std::vector<unsigned char> solo(count, 0);
    size_t slot_groups = 1;
    for (int j = 0; j < lanes; ++j) L[j].solo.h = r->batch_lanes[j];
    kicp_reg *h0 = L[0].solo.h;
    for (size_t k = 0; k < count; ++k) {
        const SmallPlan pl = h0->use_small ? small_plan(h0, n[k]) : SmallPlan();
        solo[k] = (pl.grid != 0 && !pl.generic) || lanes_for(h0, n[k]) != 1;
        if (!solo[k]) slot_groups = std::max<size_t>(slot_groups, (pass_grid(h0, n[k], true) + kGroup - 1) / kGroup);
    }
    BatchGroups sched(count, group, solo);
    auto leave = [&](int rc) {  // nothing of this call may still be running when it returns: the caller owns the frames
        for (int j = 0; j < lanes; ++j) {
            kicp_reg *h = L[j].solo.h;
            (void)aql_quiesce(h);
            (void)hipStreamSynchronize(h->stream);
            if (rc < 0 && L[j].active) h->acc_dirty = true;  // (a group that was not collected: every job's accumulators may be part full)
        }
        *done = sched.done();
        return rc;
    };
    auto finish_scan = [&](const HostLoop &loop, size_t k) {
        pose_to(loop.T, out_poses_qt + 7 * k);
        if (out_iterations) out_iterations[k] = loop.iter;
        sched.finish(k);
        if (loop.nan_flag == 2) return fail(KICP_ERR_CAPACITY, "a per-point term exceeded the exact-accumulation range (|x| >= 2^43)");
        if (loop.nan_flag) *worst = std::max(*worst, static_cast<int>(KICP_WARN_NO_CORRESPONDENCES));
        return static_cast<int>(KICP_OK);
    };
    std::vector<size_t> carry, scans;
    std::vector<GroupJob> next;
    // the lane's next group: what goes on of the one it has just collected, then fresh scans
    auto start_group = [&](GroupLane &g) {
        carry.clear();
        if (g.active && g.is_solo) carry.push_back(g.solo.k);  // (only ever called for a solo scan that goes on)
        else if (g.active)
            for (const GroupJob &j : g.jobs)
                if (j.goes_on) carry.push_back(j.k);
        const bool fresh_solo = carry.empty();
        const bool is_solo = sched.next_group(carry, scans);
        if (scans.empty()) {
            g.active = false, g.jobs.clear();
            return static_cast<int>(KICP_OK);
        }
        auto fresh = [&](size_t k) {
            HostLoop loop;
            loop.T = pose_mul(pose_from(last_poses_qt + 7 * k), pose_from(rel_odoms_qt + 7 * k));  // Registration.cpp:156
            return loop;
        };
        if (is_solo) {
            BatchFlight &f = g.solo;
            if (!(g.active && g.is_solo && !fresh_solo)) f.k = scans[0], f.loop = fresh(f.k);
            g.jobs.clear(), g.active = true, g.is_solo = true, f.active = true;
            return flight_launch(f, map, d_frames[f.k], n[f.k], tau);
        }
        next.clear();
        for (size_t k : scans) {
            GroupJob nj;
            nj.k = k;
            bool found = false;
            for (const GroupJob &j : g.jobs)
                if (g.active && !g.is_solo && j.goes_on && j.k == k) nj.loop = j.loop, found = true;
            if (!found) nj.loop = fresh(k);
            next.push_back(nj);
        }
        g.jobs.swap(next);
        g.active = true, g.is_solo = false, g.solo.active = false;
        return group_launch(r, g, group, slot_groups, map, d_frames, n, tau);
    };
    while (!sched.all_finished()) {
        bool any_active = false;
        for (int jl = 0; jl < lanes; ++jl) {
            GroupLane &g = L[jl];
            if (!g.active) {
                if (int rc = start_group(g)) return leave(rc);
                any_active = any_active || g.active;
                continue;
            }
            any_active = true;
            if (g.is_solo) {
                BatchFlight &f = g.solo;
                long long words[kReduceWords];
                const int ready = flight_rows(f, words);
                if (ready < 0) return leave(ready);
                if (ready == 0) continue;
                if ((static_cast<unsigned long long>(words[kNumLimbs]) >> 8) != 0ull)
                    return leave(fail(KICP_ERR_HIP, "a workgroup's row did not reach its group's reader in time (kRowWaitTicks)"));
                ++r->batch_queue_passes;
                if (!f.loop.step(f.h, words, nullptr)) {
                    if (int rc = start_group(g)) return leave(rc);
                    continue;
                }
                if (int rc = finish_scan(f.loop, f.k)) return leave(rc);
                g.active = false, f.active = false;
                continue;
            }
            for (size_t s = 0; s < g.jobs.size(); ++s) {
                GroupJob &j = g.jobs[s];
                if (j.collected || !group_job_rows(g, s, slot_groups)) continue;
                j.collected = true, --g.pending;
                if ((static_cast<unsigned long long>(j.words[kNumLimbs]) >> 8) != 0ull)
                    return leave(fail(KICP_ERR_HIP, "a workgroup's row did not reach its group's reader in time (kRowWaitTicks)"));
                ++r->batch_queue_passes;
                j.goes_on = !j.loop.step(g.solo.h, j.words, nullptr);
                if (!j.goes_on)
                    if (int rc = finish_scan(j.loop, j.k)) return leave(rc);
            }
            if (g.pending != 0) {
                if (++g.polls % 256u == 0u) {
                    kicp_reg *h = g.solo.h;
                    if (h->last_via_aql) {
                        if (h->aql.queue_error) return leave(fail(KICP_ERR_HIP, "the AQL queue reported error " + std::to_string(h->aql.queue_error)));
                    } else {  // (the query makes the runtime flush commands it may still hold back, and reports device faults)
                        const hipError_t q = hipStreamQuery(h->stream);
                        if (q != hipSuccess && q != hipErrorNotReady) return leave(fail(KICP_ERR_HIP, std::string("stream fault: ") + hipGetErrorString(q)));
                    }
                    if (g.since.passed()) return leave(fail(KICP_ERR_HIP, "timed out waiting for the pass kernel's rows (KICP_WAIT_TIMEOUT_S)"));
                }
                continue;
            }
            if (int rc = start_group(g)) return leave(rc);  // the group is collected: the next one goes out at once
        }
        if (!any_active && !sched.all_finished()) return leave(fail(KICP_ERR_ARG, "internal: scans left over without a lane to run them"));
    }
    *done = count;
    return KICP_OK;
}
int run_batch_queues(kicp_reg *r, kicp_map *map, size_t count, const double *const *d_frames, const size_t *n, const double *last_poses_qt,
                     const double *rel_odoms_qt, double tau, double *out_poses_qt, int *out_iterations, size_t *done, int *worst) {
    *done = 0;
    const int max_it = r->cfg.max_num_iterations;
    // SHARDED batches (the shared segment attached, kicp_reg_shm_init): every rank calls with ITS shard of every scan, the lanes'
    // exchanges go through the segment (below).  Every decision up to here and in the loop must then be the same on every rank - so
    // none of them looks at the shard sizes, which differ.
    // ... or through RCCL: lane j owns a sub-communicator of the handle's (ncclCommSplit on first use: every rank comes here with the
    // same arguments, so the splits line up), its collectives go out in the lane's own fixed order - scans j, j + lanes, ..., pass by
    // pass - on the lane's own stream, and the lanes' collectives interleave freely (round 6: until then an RCCL batch registered scan
    // after scan while the shared segment kept four in flight)
    const bool over_rccl = r->comm != nullptr && !r->shm && g_comm.CommSplit != nullptr && !r->lane_comms_failed;
    const bool sharded = r->shm != nullptr || over_rccl;
    if (r->batch_queues < 2 || max_it <= 0 || kicp_map_empty(map)) return 1;
    // Several scans per launch ("batch_group" = G): "batch_queues" is the number of scans in flight, on batch_queues / G lanes, each
    // with a list of up to G jobs per launch (run_batch_groups).  A launch per scan and pass, each scan on a queue of its own, is
    // what remains for G = 1, for sharded batches (their lanes exchange per scan and pass), for batches too short to give every lane
    // two groups, and for batches in which most scans take another kernel than the one the job list serves.  That path is as it
    // was: "batch_queues" queues where the caller has set the option, else the four it has always run on (the default of eight
    // scans in flight is sized for two lanes of four jobs), and batches of fewer than two scans per queue go elsewhere.  (None of
    // these decisions looks at a sharded batch's sizes.)
    const int in_flight = std::min(r->batch_queues, kMaxBatchInFlight);
    int group = (sharded || r->dbg == 14) ? 1 : std::min({r->batch_group, in_flight, static_cast<int>(kMaxJobs)});
    int lanes = std::min(in_flight / group, kMaxBatchQueues);
    if (group > 1 && count < 2u * static_cast<size_t>(lanes) * static_cast<size_t>(group)) group = 1;
    if (group > 1) {
        size_t shared = 0;
        for (size_t k = 0; k < count; ++k) {
            const SmallPlan pl = r->use_small ? small_plan(r, n[k]) : SmallPlan();
            if ((pl.grid == 0 || pl.generic) && lanes_for(r, n[k]) == 1) ++shared;
        }
        if (2 * shared < count) group = 1;
    }
    if (group == 1) {
        lanes = r->batch_queues_set ? std::min(r->batch_queues, kMaxBatchQueues) : kDefaultScanQueues;
        if (lanes < 2 || count < 2u * static_cast<size_t>(lanes)) return 1;
    }
    const int queues = lanes;
    if (!(r->use_aql && (!r->comm || over_rccl) && !r->allreduce_fn && !r->d_p2p_table && r->timing == 0 &&
          r->wait_mode == 0 && (r->dbg == 0 || r->dbg == 11 || r->dbg == 12 || r->dbg == 14)))
        return 1;
    if (r->shm && r->shm_poisoned)
        return fail(KICP_ERR_COMM, "the shared-segment exchange is out of step after a sharded batch that failed: kicp_reg_shm_destroy and _init again on every rank");
    // a batch of small scans only (kicp_small.hpp) is better off with ONE resident kernel and several scans in flight inside it
    // (run_batch_resident): a launch and a sweep over every workgroup's row per pass is more than one host thread can turn round in
    // the 4.5 us such a pass takes (measured, cfg4: 5.0 us per scan on four queues, 4.5 resident).  Mixed batches come here.
    bool any_large = sharded;  // (a shard goes through the generic kernel whatever its size: its group rows feed the exchange)
    for (size_t k = 0; k < count && !sharded; ++k) {
        if (n[k] == 0) return 1;
        if (!any_large) {
            const SmallPlan pl = r->use_small ? small_plan(r, n[k]) : SmallPlan();
            any_large = pl.grid == 0 || pl.generic;
        }
    }
    if (!any_large) return 1;
    if (int rc = set_device(r->device)) return rc;
    const uint64_t epoch_before = map->mirror.synced_epoch;
    if (int rc = map_sync(map, r->device, r->stream)) return rc;
    if (map->mirror.synced_epoch != epoch_before) HIP_TRY(hipStreamSynchronize(r->stream));  // (the lanes only read the copy)
    while (static_cast<int>(r->batch_lanes.size()) < lanes) {
        kicp_reg *c = nullptr;
        if (int rc = kicp_reg_clone(r, &c)) return rc;
        r->batch_lanes.push_back(c);
    }
    BatchFlight flights[kMaxBatchQueues];
    for (int j = 0; j < lanes; ++j) {
        kicp_reg *h = r->batch_lanes[j];
        h->cfg = r->cfg, h->lanes_per_query = r->lanes_per_query;
        h->query_every = r->query_every, h->dbg = r->dbg, h->latency_kernel = 0, h->small_resident = 0, h->batch_queues = 0;
        h->pass_tiles = r->pass_tiles, h->scans_in_flight = group > 1 ? lanes * group : lanes;
        h->small_group_rows = r->small_group_rows;
        h->use_small = sharded ? 0 : r->use_small, h->small_block = r->small_block, h->small_wave = r->small_wave, h->wave_block = r->wave_block;
        flights[j].h = h;
        flights[j].next = static_cast<size_t>(j);  // (sharded: lane j's first scan)
        flights[j].via_comm = over_rccl;
        if (over_rccl) {
            if (!r->lane_comms[j]) {
                const ncclResult_t rc = g_comm.CommSplit(r->comm, 0, r->rank, &r->lane_comms[j], nullptr);
                if (rc != ncclSuccess || !r->lane_comms[j]) {  // (every rank fails alike: the same library, the same arguments)
                    r->lane_comms[j] = nullptr, r->lane_comms_failed = true;
                    for (int i = 0; i < j; ++i) flights[i].h->comm = nullptr;
                    return 1;  // this and later batches go scan after scan over the handle's own communicator
                }
            }
            h->comm = r->lane_comms[j], h->nranks = r->nranks, h->rank = r->rank;
        }
    }
    r->last_small = 0, r->last_resident_passes = 0;
    {
        const SmallPlan first = r->use_small ? small_plan(flights[0].h, n[0]) : SmallPlan();
        if (first.grid && !first.generic) r->last_small = first.wave ? 2 : 1;  // ("small_active": the path of the batch's first scan)
    }
    if (group > 1)
        return run_batch_groups(r, map, count, d_frames, n, last_poses_qt, rel_odoms_qt, tau, out_poses_qt, out_iterations, done, worst, lanes, group);
    std::vector<unsigned char> complete(count, 0);
    size_t next_scan = 0, front = 0, finished_scans = 0;
    auto leave = [&](int rc) {  // nothing of this call may still be running when it returns: the caller owns the frames
        for (int j = 0; j < queues; ++j) {
            (void)aql_quiesce(flights[j].h);
            (void)hipStreamSynchronize(flights[j].h->stream);
            if (rc < 0 && flights[j].active) flights[j].h->acc_dirty = true;  // (a pass that was not collected: its accumulators may be part full)
        }
        if (rc < 0 && r->shm) r->shm_poisoned = true;  // (the ranks' lane counters can no longer be assumed equal)
        for (int j = 0; j < queues && over_rccl; ++j) flights[j].h->comm = nullptr;  // (the communicators stay this handle's)
        while (front < count && complete[front]) ++front;
        *done = front;
        return rc;
    };
    // the slots of lane j's hand-off `step` in the shared segment: [nranks], double-buffered by the hand-off's parity
    auto lane_slots = [&](int j, unsigned long long step) { return r->shm + 2 * static_cast<size_t>(r->nranks) * (1 + j) + (step & 1) * r->nranks; };
    while (finished_scans < count) {
        for (int j = 0; j < queues; ++j) {
            BatchFlight &f = flights[j];
            if (!f.active) {
                if (sharded) {  // the deal is static - lane j registers scans j, j + queues, ... - so that every rank's lane j issues the same exchanges
                    if (f.next >= count) continue;
                    f.k = f.next, f.next += static_cast<size_t>(queues), f.active = true;
                } else {
                    if (next_scan >= count) continue;
                    f.k = next_scan++, f.active = true;
                }
                f.at_peers = false;
                f.loop = HostLoop();
                f.loop.T = pose_mul(pose_from(last_poses_qt + 7 * f.k), pose_from(rel_odoms_qt + 7 * f.k));  // Registration.cpp:156
                if (int rc = flight_launch(f, map, d_frames[f.k], n[f.k], tau)) return leave(rc);
                continue;
            }
            long long words[kReduceWords];
            if (!f.at_peers) {
                const int ready = flight_rows(f, words);
                if (ready < 0) return leave(ready);
                if (ready == 0) continue;
                if ((static_cast<unsigned long long>(words[kNumLimbs]) >> 8) != 0ull)
                    return leave(fail(KICP_ERR_HIP, "a workgroup's row did not reach its group's reader in time (kRowWaitTicks)"));
                if (r->shm) {  // this rank's totals of the pass go into its slot of the lane's area; then the lane waits for every rank's
                    const unsigned long long step = r->shm_lane_step[j]++;
                    kicp_reg::ShmSlot *mine = lane_slots(j, step) + r->rank;
                    for (int i = 0; i < kReduceWords; ++i) mine->words[i] = words[i];
                    __atomic_store_n(&mine->seq, step + 1, __ATOMIC_RELEASE);
                    f.at_peers = true, f.shm_value = step + 1, f.since = Deadline(), f.polls = 0;
                }
            }
            if (r->shm) {  // (a non-blocking look: the other lanes' rows and hand-offs are served meanwhile)
                const kicp_reg::ShmSlot *slots = lane_slots(j, f.shm_value - 1);
                bool all_in = true;
                for (int k = 0; k < r->nranks && all_in; ++k) all_in = __atomic_load_n(&slots[k].seq, __ATOMIC_ACQUIRE) == f.shm_value;
                if (!all_in) {
                    if (++f.polls % 4096u == 0u && f.since.passed()) return leave(fail(KICP_ERR_COMM, "timed out waiting for a peer rank's hand-off (KICP_WAIT_TIMEOUT_S)"));
                    continue;
                }
                for (int i = 0; i < kReduceWords; ++i) words[i] = 0;
                for (int k = 0; k < r->nranks; ++k)
                    for (int i = 0; i < kReduceWords; ++i) words[i] += slots[k].words[i];  // (exact integers: the order does not matter)
                words[kNumLimbs] = words[kNumLimbs] != 0 ? 1 : 0;
                f.at_peers = false;
            }
            ++r->batch_queue_passes;
            if (!f.loop.step(f.h, words, nullptr)) {
                if (int rc = flight_launch(f, map, d_frames[f.k], n[f.k], tau)) return leave(rc);
                continue;
            }
            pose_to(f.loop.T, out_poses_qt + 7 * f.k);
            if (out_iterations) out_iterations[f.k] = f.loop.iter;
            complete[f.k] = 1, f.active = false, ++finished_scans;
            if (f.loop.nan_flag == 2) return leave(fail(KICP_ERR_CAPACITY, "a per-point term exceeded the exact-accumulation range (|x| >= 2^43)"));
            if (f.loop.nan_flag) *worst = std::max(*worst, static_cast<int>(KICP_WARN_NO_CORRESPONDENCES));
        }
    }
    for (int j = 0; j < queues && over_rccl; ++j) flights[j].h->comm = nullptr;
    *done = count;
    return KICP_OK;
}
}  // namespace host
}  // namespace kicp
