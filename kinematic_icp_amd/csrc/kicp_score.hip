// kicp_score.hip -- one frame at many poses: scored (kicp_score_poses*, kernel: kicp_score.hpp), the sums of a planar 3-DoF step
// (kicp_planar_sums*, kernel: kicp_planar.hpp) and the refinement of all poses in lock step on top of them (kicp_refine_poses_planar*),
// and kicp_relocalize / kicp_relocalize_planar: score the candidates, refine the best few, score again (see kicp_reg_internal.hpp
// for the handle)
#include "kicp_planar.hpp"
#include "kicp_planar_host.hpp"
#include "kicp_reg_internal.hpp"
#include "kicp_score.hpp"

using namespace kicp;
using namespace kicp::host;

namespace {
constexpr size_t kScoreMaxPoses = static_cast<size_t>(1) << 24;
constexpr size_t kScoreMaxPoints = 0x7FFFFFF0ull / 3;
constexpr size_t kScoreBatch = 65536;     // poses uploaded, scored and collected at a time (buffers: 120 bytes per pose)
constexpr uint32_t kScoreMaxGrid = 2048;  // workgroups of a launch; they stride over the launch's items

// poses the two buffers hold (ensure_score empties both before it replaces them)
size_t score_cap(const kicp_reg *r) { return r->d_score_acc.capacity() / kScoreWords; }
int ensure_score(kicp_reg *r, size_t poses) {
    if (poses <= score_cap(r)) return KICP_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    const size_t want = std::min(kScoreBatch, poses + poses / 2 + 64);
    r->d_score_poses.release(), r->d_score_acc.release();
    if (int rc = r->d_score_poses.reserve(want * 7)) return rc;
    return r->d_score_acc.reserve(want * kScoreWords);
}
// the rows of kicp_planar_sums beside them (kPlanarWords per pose), as many poses as the two buffers above hold
int ensure_planar(kicp_reg *r, size_t poses) {
    if (int rc = ensure_score(r, poses)) return rc;
    const size_t want = score_cap(r) * kPlanarWords;
    if (want <= r->d_planar_acc.capacity()) return KICP_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->d_planar_acc.release();
    return r->d_planar_acc.reserve(want);
}
// A sum of a pose from the four limb sums of its accumulator row: the limb sums (limb k at 2^(21 k)) are put together as ONE integer,
// cut into the three 40-bit limbs every hand-off of the pass kernels carries (i128_to_limbs) and converted by the same function: the
// double kicp_pass_sums returns for the same integer.
double limb_sums_to_double(const unsigned long long *limb_sums) {
    __int128 t = 0;
    for (int j = 0; j < kTermLimbs; ++j) t += static_cast<__int128>(static_cast<long long>(limb_sums[j])) * (static_cast<__int128>(1) << (21 * j));
    const unsigned __int128 u = static_cast<unsigned __int128>(t);
    const unsigned long long m40 = (1ull << 40) - 1;
    const long long l[3] = {static_cast<long long>(static_cast<unsigned long long>(u) & m40), static_cast<long long>(static_cast<unsigned long long>(u >> 40) & m40),
                            static_cast<long long>(t >> 80)};
    return host_limbs_to_double(l);
}
void row_to_sums(const unsigned long long *row, double &n_corr, double &ssr) {
    ssr = limb_sums_to_double(row);
    n_corr = static_cast<double>(row[kScoreCountWord]);
}
// the eight sums of kicp_planar_sums from a row of k_planar_poses: N, S_x, S_y (the row holds sum -s.y, the pass kernels' term), S_ss,
// S_a, S_b, S_c, ssr
void row_to_planar_sums(const unsigned long long *row, double *sums) {
    sums[0] = static_cast<double>(row[kPlanarCountWord]);
    for (int i = 0; i < kPlanarTerms; ++i) sums[1 + i] = limb_sums_to_double(row + kTermLimbs * i);
    sums[2] = -sums[2];
}
int check_score_args(const kicp_reg *reg, const kicp_map *map, const void *frame, size_t n, const double *poses_qt, size_t count, const double *out_a,
                     const double *out_b) {
    if (!reg || !map || (!frame && n) || (count && (!poses_qt || !out_a || !out_b))) return fail(KICP_ERR_ARG, "null argument");
    if (count > kScoreMaxPoses) return fail(KICP_ERR_CAPACITY, "more than 2^24 poses");
    if (n > kScoreMaxPoints) return fail(KICP_ERR_CAPACITY, "frame too large");
    if (reg->comm || reg->allreduce_fn || reg->shm || reg->d_p2p_table) return fail(KICP_ERR_ARG, "detach the multi-GPU exchange first: poses are scored per device");
    return KICP_OK;
}
// One frame at `count` poses: the accumulator rows of k_score_poses (PLANAR: of k_planar_poses), handed to on_row(pose index, row)
// batch by batch.  Nothing is launched, and on_row is not called, for an empty map, an empty frame or no poses.
// (arguments checked; `d_frame` on the handle's device)
template <bool PLANAR, class OnRow>
int rows_device(kicp_reg *reg, kicp_map *map, const double *d_frame, size_t n, const double *poses_qt, size_t count, double tau, OnRow on_row) {
    constexpr int kRowWords = PLANAR ? kPlanarWords : kScoreWords;
    reg->score_launches = 0, reg->score_items_per_workgroup = 0;
    if (int rc = map_finish_pending(map)) return rc;  // (a deferred update's error is this call's: the map it would score against is not the updated one)
    if (kicp_map_empty(map) || n == 0 || count == 0) return KICP_OK;
    if (int rc = set_device(reg->device)) return rc;
    if (int rc = map_sync(map, reg->device, reg->stream)) return rc;
    if (int rc = aql_quiesce(reg)) return rc;
    reg->stream_dirty = true;
    if (int rc = PLANAR ? ensure_planar(reg, std::min(count, kScoreBatch)) : ensure_score(reg, std::min(count, kScoreBatch))) return rc;
    unsigned long long *d_acc = PLANAR ? reg->d_planar_acc.get() : reg->d_score_acc.get();
    ScoreParams sp{};
    sp.pass.src = d_frame, sp.pass.n = static_cast<uint32_t>(n), sp.pass.map = map->mirror.view, sp.pass.tau = tau;
    sp.pass.search = search_params(tau, map->mirror.view.voxel_size);
    const unsigned long long tiles = (n + kScoreBlock - 1) / kScoreBlock;
    // a launch serves whole tiles (256 queries, the frame's last one fewer): as many as fit "score_chunk", at least one
    const unsigned long long per_launch = std::max<unsigned long long>(1ull, static_cast<unsigned long long>(reg->score_chunk / kScoreBlock));
    std::vector<unsigned long long> rows;
    for (size_t first = 0; first < count; first += score_cap(reg)) {
        const size_t m = std::min(score_cap(reg), count - first);
        if (int rc = staged_upload(reg->stage, 0, reg->d_score_poses.get(), poses_qt + 7 * first, m * 7 * sizeof(double), reg->stream)) return rc;
        HIP_TRY(hipMemsetAsync(d_acc, 0, m * kRowWords * sizeof(unsigned long long), reg->stream));
        sp.poses = reg->d_score_poses.get(), sp.acc = d_acc, sp.count = static_cast<uint32_t>(m);
        const unsigned long long total = tiles * m;
        for (unsigned long long item0 = 0; item0 < total; item0 += per_launch) {
            sp.item0 = item0, sp.items = std::min(per_launch, total - item0);
            const uint32_t grid = static_cast<uint32_t>(std::min<unsigned long long>(sp.items, kScoreMaxGrid));
            reg->score_items_per_workgroup = std::max(reg->score_items_per_workgroup, (sp.items + grid - 1) / grid);
            if (PLANAR) hipLaunchKernelGGL(k_planar_poses, dim3(grid), dim3(kScoreBlock), 0, reg->stream, sp);
            else hipLaunchKernelGGL(k_score_poses, dim3(grid), dim3(kScoreBlock), 0, reg->stream, sp);
            ++reg->score_launches;
        }
        HIP_TRY(hipGetLastError());
        rows.resize(m * kRowWords);
        if (int rc = staged_download(reg->stage, rows.data(), d_acc, rows.size() * sizeof(unsigned long long), reg->stream)) return rc;
        for (size_t k = 0; k < m; ++k) on_row(first + k, &rows[k * kRowWords]);
    }
    return KICP_OK;
}
int score_device(kicp_reg *reg, kicp_map *map, const double *d_frame, size_t n, const double *poses_qt, size_t count, double tau, double *out_n_corr,
                 double *out_ssr) {
    for (size_t k = 0; k < count; ++k) out_n_corr[k] = out_ssr[k] = 0.0;
    return rows_device<false>(reg, map, d_frame, n, poses_qt, count, tau,
                              [&](size_t k, const unsigned long long *row) { row_to_sums(row, out_n_corr[k], out_ssr[k]); });
}
// the eight sums of a planar step per pose (count x kPlanarSums doubles)
int planar_sums_device(kicp_reg *reg, kicp_map *map, const double *d_frame, size_t n, const double *poses_qt, size_t count, double tau, double *out_sums) {
    for (size_t k = 0; k < count * kPlanarSums; ++k) out_sums[k] = 0.0;
    return rows_device<true>(reg, map, d_frame, n, poses_qt, count, tau,
                             [&](size_t k, const unsigned long long *row) { row_to_planar_sums(row, out_sums + kPlanarSums * k); });
}
// one Gauss-Newton step of a pose from its sums: T <- T * pose_exp({dx, dy, 0, 0, 0, dtheta}); false (nothing written): degenerate
bool planar_step(const double *sums, const double *pose_qt, double *out_pose_qt, double *out_dx) {
    double dx[3], xi[6];
    if (!planar_solve(sums, dx)) return false;
    planar_twist(dx, xi);
    const Pose next = pose_mul(pose_from(pose_qt), pose_exp(xi));
    pose_to(next, out_pose_qt);
    if (out_dx) out_dx[0] = dx[0], out_dx[1] = dx[1], out_dx[2] = dx[2];
    return true;
}
constexpr int kPlanarConverged = 0, kPlanarIterationLimit = 1, kPlanarDegenerate = 2;
// All poses in lock step: iteration j takes the sums of every pose still active from ONE call of planar_sums_device (the active poses
// compacted; integer sums: a pose's row does not depend on its neighbours in the launch), then steps each of them on the host.
// (`iterations`, `status`: count elements each)
int refine_planar_device(kicp_reg *reg, kicp_map *map, const double *d_frame, size_t n, const double *poses_qt, size_t count, double tau, int max_iterations,
                         double convergence, double *out_poses_qt, int *iterations, int *status) {
    if (count) std::memmove(out_poses_qt, poses_qt, count * 7 * sizeof(double));
    for (size_t k = 0; k < count; ++k) iterations[k] = 0, status[k] = kPlanarDegenerate;
    reg->score_launches = 0, reg->score_items_per_workgroup = 0;
    if (int rc = map_finish_pending(map)) return rc;
    if (kicp_map_empty(map) || n == 0 || count == 0) return KICP_OK;
    std::vector<size_t> active(count), next;
    for (size_t k = 0; k < count; ++k) active[k] = k;
    std::vector<double> poses, sums;
    int launches = 0;
    unsigned long long items_per_workgroup = 0;
    while (!active.empty()) {
        poses.resize(7 * active.size()), sums.resize(kPlanarSums * active.size());
        for (size_t j = 0; j < active.size(); ++j) std::memcpy(&poses[7 * j], out_poses_qt + 7 * active[j], 7 * sizeof(double));
        if (int rc = planar_sums_device(reg, map, d_frame, n, poses.data(), active.size(), tau, sums.data())) return rc;
        launches += reg->score_launches, items_per_workgroup = std::max(items_per_workgroup, reg->score_items_per_workgroup);
        next.clear();
        for (size_t j = 0; j < active.size(); ++j) {
            const size_t k = active[j];
            double dx[3];
            if (!planar_step(&sums[kPlanarSums * j], &poses[7 * j], out_poses_qt + 7 * k, dx)) continue;  // (status: degenerate; the pose as it stood)
            ++iterations[k];
            if (planar_step_norm(dx) < convergence) status[k] = kPlanarConverged;
            else if (iterations[k] >= max_iterations) status[k] = kPlanarIterationLimit;
            else next.push_back(k);
        }
        active.swap(next);
    }
    reg->score_launches = launches, reg->score_items_per_workgroup = items_per_workgroup;
    return KICP_OK;
}
int check_refine_args(int max_iterations, double convergence) {
    if (max_iterations < 1 || !(convergence >= 0.0)) return fail(KICP_ERR_ARG, "max_iterations must be >= 1 and convergence >= 0");
    return KICP_OK;
}
// a host frame into the handle's device frame (nothing to do for an empty frame or map: no kernel will read it)
int upload_frame(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n) {
    if (n == 0 || kicp_map_empty(map)) return KICP_OK;
    if (int rc = set_device(reg->device)) return rc;
    if (int rc = ensure_frame(reg, n)) return rc;
    if (int rc = aql_quiesce(reg)) return rc;
    reg->stream_dirty = true;
    return staged_upload(reg->stage, 0, reg->d_frame.get(), frame_xyz, n * 24, reg->stream);
}
bool pose_is_finite(const double *p) {
    for (int i = 0; i < 7; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}
// kicp_relocalize and kicp_relocalize_planar: everything but step 3.  refine(d_frame, start, m, refined, out) refines the m poses of
// `start` into `refined` and marks in `out` those that are out of the running; a negative return is the call's error.
template <class Refine>
int relocalize_with(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *candidates_qt, size_t count,
                    double max_correspondence_distance, size_t top_m, double out_pose_qt[7], size_t *out_candidate, double *out_cost_before,
                    double *out_cost_after, Refine refine) {
    if (!out_pose_qt) return fail(KICP_ERR_ARG, "null argument");
    if (count == 0 || top_m == 0) return fail(KICP_ERR_ARG, "kicp_relocalize needs at least one candidate and top_m >= 1");
    if (int rc = check_score_args(reg, map, frame_xyz, n, candidates_qt, count, out_pose_qt, out_pose_qt)) return rc;
    if (int rc = map_finish_pending(map)) return rc;
    const double tau = max_correspondence_distance;
    auto result = [&](const double *pose, size_t candidate, double before, double after) {
        std::memcpy(out_pose_qt, pose, 7 * sizeof(double));
        if (out_candidate) *out_candidate = candidate;
        if (out_cost_before) *out_cost_before = before;
        if (out_cost_after) *out_cost_after = after;
    };
    if (n == 0 || kicp_map_empty(map)) {  // nothing can correspond: every candidate costs tau^2, none can be refined
        result(candidates_qt, 0, tau * tau, tau * tau);
        return KICP_WARN_NO_CORRESPONDENCES;
    }
    if (int rc = upload_frame(reg, map, frame_xyz, n)) return rc;  // once: the scoring and the refinements read this copy
    const double *d_frame = reg->d_frame.get();
    // truncated least squares, lower is better: a point without a correspondence costs tau^2
    auto cost_of = [&](double n_corr, double ssr) { return (ssr + (static_cast<double>(n) - n_corr) * (tau * tau)) / static_cast<double>(n); };
    // 1. every candidate
    std::vector<double> n_corr(count), ssr(count), cost(count);
    if (int rc = score_device(reg, map, d_frame, n, candidates_qt, count, tau, n_corr.data(), ssr.data())) return rc;
    int launches = reg->score_launches;
    for (size_t k = 0; k < count; ++k) cost[k] = cost_of(n_corr[k], ssr[k]);
    // 2. the top_m cheapest, ties to the lower index
    const size_t m = std::min(top_m, count);
    std::vector<size_t> rank(count);
    for (size_t k = 0; k < count; ++k) rank[k] = k;
    std::partial_sort(rank.begin(), rank.begin() + m, rank.end(), [&](size_t a, size_t b) { return cost[a] < cost[b] || (cost[a] == cost[b] && a < b); });
    // 3. refined, all from the same device frame
    std::vector<double> start(7 * m), refined(7 * m);
    std::vector<char> out(m, 0);
    for (size_t j = 0; j < m; ++j) std::memcpy(&start[7 * j], candidates_qt + 7 * rank[j], 7 * sizeof(double));
    reg->score_launches = 0;
    const int rc_reg = refine(d_frame, start.data(), m, refined.data(), out.data());
    if (rc_reg < 0) return rc_reg;
    launches += reg->score_launches;  // (a refinement that scores: kicp_relocalize_planar)
    // 4. the refined poses, scored by one more call
    std::vector<double> n_after(m), ssr_after(m);
    if (int rc = score_device(reg, map, d_frame, n, refined.data(), m, tau, n_after.data(), ssr_after.data())) return rc;
    reg->score_launches += launches;
    // 5. the cheapest refined pose, ties to the earlier rank; a refinement that ended without correspondences is out
    size_t best = m;
    double best_cost = 0.0;
    for (size_t j = 0; j < m; ++j) {
        if (out[j]) continue;
        const double c = cost_of(n_after[j], ssr_after[j]);
        if (best == m || c < best_cost) best = j, best_cost = c;
    }
    if (best == m) {  // none survived: the best unrefined candidate
        result(candidates_qt + 7 * rank[0], rank[0], cost[rank[0]], cost[rank[0]]);
        return KICP_WARN_NO_CORRESPONDENCES;
    }
    result(&refined[7 * best], rank[best], cost[rank[best]], best_cost);
    return KICP_OK;
}
}  // namespace

extern "C" {

int kicp_score_poses_device(kicp_reg *reg, kicp_map *map, const double *d_frame_xyz, size_t n, const double *poses_qt, size_t count,
                            double max_correspondence_distance, double *out_n_corr, double *out_ssr) {
    KICP_TRACE_CALL();
    if (int rc = check_score_args(reg, map, d_frame_xyz, n, poses_qt, count, out_n_corr, out_ssr)) return rc;
    return score_device(reg, map, d_frame_xyz, n, poses_qt, count, max_correspondence_distance, out_n_corr, out_ssr);
}
int kicp_score_poses(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *poses_qt, size_t count,
                     double max_correspondence_distance, double *out_n_corr, double *out_ssr) {
    KICP_TRACE_CALL();
    if (int rc = check_score_args(reg, map, frame_xyz, n, poses_qt, count, out_n_corr, out_ssr)) return rc;
    if (int rc = map_finish_pending(map)) return rc;
    if (count)
        if (int rc = upload_frame(reg, map, frame_xyz, n)) return rc;
    return score_device(reg, map, reg->d_frame.get(), n, poses_qt, count, max_correspondence_distance, out_n_corr, out_ssr);
}

int kicp_relocalize(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *candidates_qt, size_t count,
                    double max_correspondence_distance, size_t top_m, double out_pose_qt[7], size_t *out_candidate, double *out_cost_before,
                    double *out_cost_after) {
    KICP_TRACE_CALL();
    // step 3: independent registrations of the same frame (last pose = candidate, odometry = identity); a NaN pose is out
    auto refine = [&](const double *d_frame, const double *start, size_t m, double *refined, char *out) {
        std::vector<const double *> frames(m, d_frame);
        std::vector<size_t> sizes(m, n);
        std::vector<double> odom(7 * m, 0.0);
        for (size_t j = 0; j < m; ++j) odom[7 * j + 3] = 1.0;
        const int rc = kicp_register_device_batch(reg, map, m, frames.data(), sizes.data(), start, odom.data(), max_correspondence_distance, refined, nullptr);
        for (size_t j = 0; j < m && rc >= 0; ++j) out[j] = !pose_is_finite(refined + 7 * j);
        return rc;
    };
    return relocalize_with(reg, map, frame_xyz, n, candidates_qt, count, max_correspondence_distance, top_m, out_pose_qt, out_candidate, out_cost_before,
                           out_cost_after, refine);
}
int kicp_relocalize_planar(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *candidates_qt, size_t count,
                           double max_correspondence_distance, size_t top_m, int max_iterations, double convergence, double out_pose_qt[7],
                           size_t *out_candidate, double *out_cost_before, double *out_cost_after) {
    KICP_TRACE_CALL();
    if (int rc = check_refine_args(max_iterations, convergence)) return rc;
    // step 3: the planar refinement of all finalists in lock step; a degenerate one is out
    auto refine = [&](const double *d_frame, const double *start, size_t m, double *refined, char *out) {
        std::vector<int> iterations(m), status(m);
        const int rc = refine_planar_device(reg, map, d_frame, n, start, m, max_correspondence_distance, max_iterations, convergence, refined, iterations.data(),
                                            status.data());
        for (size_t j = 0; j < m; ++j) out[j] = status[j] == kPlanarDegenerate;
        return rc;
    };
    return relocalize_with(reg, map, frame_xyz, n, candidates_qt, count, max_correspondence_distance, top_m, out_pose_qt, out_candidate, out_cost_before,
                           out_cost_after, refine);
}

int kicp_planar_sums_device(kicp_reg *reg, kicp_map *map, const double *d_frame_xyz, size_t n, const double *poses_qt, size_t count,
                            double max_correspondence_distance, double *out_sums) {
    KICP_TRACE_CALL();
    if (int rc = check_score_args(reg, map, d_frame_xyz, n, poses_qt, count, out_sums, out_sums)) return rc;
    return planar_sums_device(reg, map, d_frame_xyz, n, poses_qt, count, max_correspondence_distance, out_sums);
}
int kicp_planar_sums(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *poses_qt, size_t count,
                     double max_correspondence_distance, double *out_sums) {
    KICP_TRACE_CALL();
    if (int rc = check_score_args(reg, map, frame_xyz, n, poses_qt, count, out_sums, out_sums)) return rc;
    if (int rc = map_finish_pending(map)) return rc;
    if (count)
        if (int rc = upload_frame(reg, map, frame_xyz, n)) return rc;
    return planar_sums_device(reg, map, reg->d_frame.get(), n, poses_qt, count, max_correspondence_distance, out_sums);
}
int kicp_planar_step(const double sums[8], const double pose_qt[7], double out_pose_qt[7], double out_dx[3]) {
    if (!sums || !pose_qt || !out_pose_qt) return fail(KICP_ERR_ARG, "null argument");
    return planar_step(sums, pose_qt, out_pose_qt, out_dx) ? 1 : 0;
}
// (out_iterations / out_status may be null)
static int refine_planar_checked(kicp_reg *reg, kicp_map *map, const double *d_frame, size_t n, const double *poses_qt, size_t count, double tau,
                                 int max_iterations, double convergence, double *out_poses_qt, int *out_iterations, int *out_status) {
    std::vector<int> iterations(count), status(count);
    if (int rc = refine_planar_device(reg, map, d_frame, n, poses_qt, count, tau, max_iterations, convergence, out_poses_qt, iterations.data(), status.data()))
        return rc;
    if (out_iterations) std::copy(iterations.begin(), iterations.end(), out_iterations);
    if (out_status) std::copy(status.begin(), status.end(), out_status);
    return KICP_OK;
}
int kicp_refine_poses_planar_device(kicp_reg *reg, kicp_map *map, const double *d_frame_xyz, size_t n, const double *poses_qt, size_t count,
                                    double max_correspondence_distance, int max_iterations, double convergence, double *out_poses_qt,
                                    int *out_iterations, int *out_status) {
    KICP_TRACE_CALL();
    if (int rc = check_score_args(reg, map, d_frame_xyz, n, poses_qt, count, out_poses_qt, out_poses_qt)) return rc;
    if (int rc = check_refine_args(max_iterations, convergence)) return rc;
    return refine_planar_checked(reg, map, d_frame_xyz, n, poses_qt, count, max_correspondence_distance, max_iterations, convergence, out_poses_qt,
                                 out_iterations, out_status);
}
int kicp_refine_poses_planar(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *poses_qt, size_t count,
                             double max_correspondence_distance, int max_iterations, double convergence, double *out_poses_qt, int *out_iterations,
                             int *out_status) {
    KICP_TRACE_CALL();
    if (int rc = check_score_args(reg, map, frame_xyz, n, poses_qt, count, out_poses_qt, out_poses_qt)) return rc;
    if (int rc = check_refine_args(max_iterations, convergence)) return rc;
    if (int rc = map_finish_pending(map)) return rc;
    if (count)
        if (int rc = upload_frame(reg, map, frame_xyz, n)) return rc;
    return refine_planar_checked(reg, map, reg->d_frame.get(), n, poses_qt, count, max_correspondence_distance, max_iterations, convergence, out_poses_qt,
                                 out_iterations, out_status);
}

// Candidate poses for kicp_relocalize: center * planar(dx, dy, dyaw) for every offset i * step with |i * step| <= half extent (per
// axis; a step <= 0 or a half extent of 0 leaves that axis at the centre) - offsets in the centre's body frame, x slowest, yaw fastest.
size_t kicp_planar_grid(const double center_qt[7], double half_x, double half_y, double half_yaw, double step_x, double step_y, double step_yaw,
                        double *out_poses_qt, size_t cap_poses) {
    if (!center_qt) return 0;
    auto steps_of = [](double half, double step) { return (step > 0.0 && half > 0.0) ? static_cast<long>(std::floor(half / step + 1e-9)) : 0l; };
    const long kx = steps_of(half_x, step_x), ky = steps_of(half_y, step_y), kw = steps_of(half_yaw, step_yaw);
    const size_t total = static_cast<size_t>(2 * kx + 1) * static_cast<size_t>(2 * ky + 1) * static_cast<size_t>(2 * kw + 1);
    if (!out_poses_qt) return total;
    const Pose center = pose_from(center_qt);
    size_t at = 0;
    for (long ix = -kx; ix <= kx; ++ix)
        for (long iy = -ky; iy <= ky; ++iy)
            for (long iw = -kw; iw <= kw && at < cap_poses; ++iw, ++at) {
                const double yaw = static_cast<double>(iw) * step_yaw;
                const Pose offset{0.0, 0.0, std::sin(0.5 * yaw), std::cos(0.5 * yaw), static_cast<double>(ix) * step_x, static_cast<double>(iy) * step_y, 0.0};
                pose_to(pose_mul(center, offset), out_poses_qt + 7 * at);
            }
    return total;
}

}  // extern "C"
