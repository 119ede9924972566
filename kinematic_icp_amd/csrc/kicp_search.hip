// kicp_search.hip -- whole-map relocalisation: the occupancy pyramid of a map (kicp_occ_*; kernels: kicp_search.hpp), the scores of
// search nodes against it (kicp_occ_score_nodes), the branch-and-bound search on top of them (kicp_search_poses; traversal:
// kicp_search_host.hpp) and kicp_relocalize_search, which hands the search's result to kicp_relocalize_planar (see
// kicp_reg_internal.hpp for the handle)
#include <memory>

#include "kicp_reg_internal.hpp"
#include "kicp_search.hpp"
#include "kicp_search_host.hpp"

using namespace kicp;
using namespace kicp::host;

struct kicp_occ {
    int device = 0;
    OccGrid grid{};
    int dilate = 0, levels = 0;
    unsigned long long set_cells = 0;
    DevBuf<uint32_t> bits;  // levels + 1 levels of grid.level_words words each, level 0 first
};

namespace {
constexpr unsigned long long kOccMaxBytes = 1ull << 30;
constexpr double kOccMaxAxis = 16777216.0;       // cells per axis (occ_cell's range)
constexpr uint32_t kSearchMaxAxis = 1u << 20;     // nodes per axis of a window
constexpr uint32_t kSearchMaxYaws = 1u << 16;
constexpr size_t kSearchPiece = 1u << 20;         // nodes uploaded, scored and collected at a time (12 bytes per node)
constexpr uint32_t kSearchMaxGrid = 8192;         // workgroups of a launch; their waves stride over the piece's nodes
constexpr size_t kSearchMaxPoints = 0x7FFFFFF0ull / 3;
constexpr double kTwoPi = 6.283185307179586476925286766559;

double key_to_double(unsigned long long key) {
    const unsigned long long b = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}
int check_window(const kicp_search_window *w) {
    if (!w) return fail(KICP_ERR_ARG, "null argument");
    if (w->nx == 0 || w->ny == 0 || w->nyaw == 0 || w->nx > kSearchMaxAxis || w->ny > kSearchMaxAxis || w->nyaw > kSearchMaxYaws)
        return fail(KICP_ERR_ARG, "search window: nx, ny must be 1 .. 2^20 and nyaw 1 .. 2^16");
    if (!std::isfinite(w->x0) || !std::isfinite(w->y0) || !std::isfinite(w->z) || !std::isfinite(w->yaw0) || !std::isfinite(w->yaw_step))
        return fail(KICP_ERR_ARG, "search window: a field is not finite");
    return KICP_OK;
}
unsigned long long window_nodes(const kicp_search_window *w) { return static_cast<unsigned long long>(w->nx) * w->ny * w->nyaw; }
void yaw_table(const kicp_search_window *w, double *cs) {
    for (unsigned int j = 0; j < w->nyaw; ++j) {
        const double yaw = w->yaw0 + static_cast<double>(j) * w->yaw_step;
        cs[2 * j] = std::cos(yaw), cs[2 * j + 1] = std::sin(yaw);
    }
}
void node_pose(const kicp_search_window *w, double cell, unsigned long long node, double *pose_qt) {
    const unsigned long long ix = node % w->nx, row = node / w->nx, iy = row % w->ny, j = row / w->ny;
    const double yaw = w->yaw0 + static_cast<double>(j) * w->yaw_step;
    pose_qt[0] = 0.0, pose_qt[1] = 0.0, pose_qt[2] = std::sin(0.5 * yaw), pose_qt[3] = std::cos(0.5 * yaw);
    pose_qt[4] = w->x0 + static_cast<double>(ix) * cell, pose_qt[5] = w->y0 + static_cast<double>(iy) * cell, pose_qt[6] = w->z;
}
int check_search_args(const kicp_reg *reg, const kicp_occ *occ, const double *frame, size_t n, const kicp_search_window *w) {
    if (!reg || !occ || (!frame && n)) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_window(w)) return rc;
    if (n > kSearchMaxPoints) return fail(KICP_ERR_CAPACITY, "frame too large");
    if (reg->device != occ->device) return fail(KICP_ERR_ARG, "the occupancy pyramid lives on another device than the registration handle");
    if (reg->comm || reg->allreduce_fn || reg->shm || reg->d_p2p_table) return fail(KICP_ERR_ARG, "detach the multi-GPU exchange first: nodes are scored per device");
    return KICP_OK;
}
// The frame's cells at every yaw of the window, in the handle's buffers (arguments checked, n > 0): the frame and the rotation table
// go up once, k_search_cells writes the cells; score_prepared then serves any number of node lists.
int prepare_cells(kicp_reg *reg, const kicp_occ *occ, const double *frame_xyz, size_t n, const kicp_search_window *w) {
    const unsigned long long cell_bytes = 12ull * n * w->nyaw;
    if (cell_bytes > kOccMaxBytes) return fail(KICP_ERR_CAPACITY, "the cells of the frame at every yaw need " + std::to_string(cell_bytes) + " bytes (limit 1 GiB)");
    if (int rc = set_device(reg->device)) return rc;
    if (int rc = ensure_frame(reg, n)) return rc;
    if (int rc = aql_quiesce(reg)) return rc;
    reg->stream_dirty = true;
    if (3 * n * w->nyaw > reg->d_search_cells.capacity() || 2u * w->nyaw > reg->d_search_cs.capacity()) {
        HIP_TRY(hipStreamSynchronize(reg->stream));
        if (int rc = reg->d_search_cells.reserve(3 * n * w->nyaw)) return rc;
        if (int rc = reg->d_search_cs.reserve(2u * w->nyaw)) return rc;
    }
    if (int rc = staged_upload(reg->stage, 0, reg->d_frame.get(), frame_xyz, n * 24, reg->stream)) return rc;
    std::vector<double> cs(2u * w->nyaw);
    yaw_table(w, cs.data());
    if (int rc = staged_upload(reg->stage, 0, reg->d_search_cs.get(), cs.data(), cs.size() * sizeof(double), reg->stream)) return rc;
    const SearchWindowDev wd{w->x0, w->y0, w->z, w->nx, w->ny, w->nyaw};
    const uint32_t yaw_grid = std::min(w->nyaw, 1024u);
    reg->search_yaw_trips = (w->nyaw + yaw_grid - 1) / yaw_grid;
    hipLaunchKernelGGL(k_search_cells, dim3(static_cast<uint32_t>((n + 255) / 256), yaw_grid), dim3(256), 0, reg->stream, reg->d_frame.get(),
                       static_cast<uint32_t>(n), reg->d_search_cs.get(), wd, occ->grid, reg->d_search_cells.get());
    HIP_TRY(hipGetLastError());
    return KICP_OK;
}
// the scores of `count` nodes (indices checked by the caller) at `level`, a piece at a time
int score_prepared(kicp_reg *reg, const kicp_occ *occ, size_t n, const kicp_search_window *w, int level, const unsigned long long *nodes, size_t count,
                   unsigned int *out_hits) {
    if (count == 0) return KICP_OK;
    const size_t piece = std::min(count, kSearchPiece);
    if (piece > reg->d_search_nodes.capacity() || piece > reg->d_search_hits.capacity()) {  // (each on its own: one may have failed to grow)
        HIP_TRY(hipStreamSynchronize(reg->stream));
        if (int rc = reg->d_search_nodes.reserve(piece)) return rc;
        if (int rc = reg->d_search_hits.reserve(piece)) return rc;
    }
    const SearchWindowDev wd{w->x0, w->y0, w->z, w->nx, w->ny, w->nyaw};
    const uint32_t *level_bits = occ->bits.get() + static_cast<size_t>(level) * occ->grid.level_words;
    for (size_t first = 0; first < count; first += piece) {
        const size_t m = std::min(piece, count - first);
        if (int rc = staged_upload(reg->stage, 0, reg->d_search_nodes.get(), nodes + first, m * sizeof(unsigned long long), reg->stream)) return rc;
        const uint32_t grid = static_cast<uint32_t>(std::min<size_t>((m + kSearchBlock / 64 - 1) / (kSearchBlock / 64), kSearchMaxGrid));
        hipLaunchKernelGGL(k_search_score, dim3(grid), dim3(kSearchBlock), 0, reg->stream, reg->d_search_cells.get(), static_cast<uint32_t>(n), level_bits,
                           occ->grid, wd, level, reg->d_search_nodes.get(), static_cast<unsigned long long>(m), reg->d_search_hits.get());
        HIP_TRY(hipGetLastError());
        ++reg->search_launches;
        if (int rc = staged_download(reg->stage, out_hits + first, reg->d_search_hits.get(), m * sizeof(uint32_t), reg->stream)) return rc;
    }
    return KICP_OK;
}
// (arguments checked) the search itself; n == 0: every score is zero, the traversal runs over a scorer that says so
int search_device(kicp_reg *reg, const kicp_occ *occ, const double *frame_xyz, size_t n, const kicp_search_window *w, size_t top_m,
                  std::vector<SearchHit> &found) {
    reg->search_launches = 0, reg->search_nodes_scored = 0;
    if (n)
        if (int rc = prepare_cells(reg, occ, frame_xyz, n, w)) return rc;
    SearchCounts counts;
    auto scorer = [&](int level, const std::vector<unsigned long long> &nodes, std::vector<unsigned int> &hits) -> int {
        hits.assign(nodes.size(), 0u);
        return n ? score_prepared(reg, occ, n, w, level, nodes.data(), nodes.size(), hits.data()) : KICP_OK;
    };
    const int rc = search_top(w->nx, w->ny, w->nyaw, occ->levels, top_m, static_cast<unsigned long long>(reg->search_max_nodes), scorer, found, counts);
    reg->search_nodes_scored = counts.nodes_scored;
    if (rc == kSearchCapacity)
        return fail(KICP_ERR_CAPACITY, "the search would score more than \"search_max_nodes\" = " + std::to_string(static_cast<unsigned long long>(reg->search_max_nodes)) +
                                           " nodes (window: " + std::to_string(window_nodes(w)) + ")");
    return rc;
}
}  // namespace

extern "C" {

int kicp_occ_build(kicp_map *map, int device, double cell, int dilate, int levels, kicp_occ **out) {
    KICP_TRACE_CALL();
    if (!map || !out) return fail(KICP_ERR_ARG, "null argument");
    *out = nullptr;
    if (!(cell > 0.0) || !std::isfinite(cell)) return fail(KICP_ERR_ARG, "cell must be positive and finite");
    if (dilate < 0 || dilate > 4) return fail(KICP_ERR_ARG, "dilate must be 0 .. 4");
    if (levels < 0 || levels > 10) return fail(KICP_ERR_ARG, "levels must be 0 .. 10");
    if (int rc = map_finish_pending(map)) return rc;
    if (int rc = set_device(device)) return rc;
    std::unique_ptr<kicp_occ> occ(new kicp_occ);
    occ->device = device, occ->dilate = dilate, occ->levels = levels;
    OccGrid &g = occ->grid;
    g.cell = cell;
    const bool empty = kicp_map_empty(map) != 0;
    // The whole build runs on the null stream, deliberately: it is a rare, one-off call without a handle of its own, and the blocking
    // copy of the count at its end orders every kernel of it before any later use of the pyramid on a handle's stream.
    hipStream_t st = nullptr;
    const MapView *view = nullptr;
    uint32_t slots = 0;
    if (empty) {
        for (int a = 0; a < 3; ++a) g.min[a] = 0.0, g.dims[a] = 1;
    } else {
        if (int rc = map_sync(map, device, st)) return rc;
        view = &map->mirror.view;
        slots = static_cast<uint32_t>(map->mirror.live_slots);
        // the bounding box of the mirror's points, as order-preserving keys
        DevBuf<unsigned long long> d_bounds;
        if (int rc = d_bounds.reserve(6)) return rc;
        const unsigned long long init[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
        unsigned long long keys[6];
        HIP_TRY(hipMemcpyAsync(d_bounds.get(), init, sizeof init, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_occ_bounds, dim3((slots + 255u) / 256u), dim3(256), 0, st, map->mirror.d_table.get(), slots, map->mirror.d_pool.get(), view->cap,
                           view->cbits, d_bounds.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(keys, d_bounds.get(), sizeof keys, hipMemcpyDeviceToHost));
        if (keys[0] > keys[3]) return fail(KICP_ERR_HIP, "the map's device copy holds no point although the map is not empty");
        for (int a = 0; a < 3; ++a) {
            const double lo = key_to_double(keys[a]), hi = key_to_double(keys[3 + a]);
            if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(KICP_ERR_ARG, "the map holds a point that is not finite");
            g.min[a] = (std::floor(lo / cell) - static_cast<double>(dilate + 1)) * cell;
            const double dims = std::floor((hi - g.min[a]) / cell) + static_cast<double>(dilate + 2);
            if (!(dims >= 1.0) || dims >= kOccMaxAxis)
                return fail(KICP_ERR_CAPACITY, "the occupancy grid would have " + std::to_string(dims) + " cells along axis " + std::to_string(a) + " (limit 2^24)");
            g.dims[a] = static_cast<int32_t>(dims);
        }
    }
    g.wx = (static_cast<uint32_t>(g.dims[0]) + 31u) / 32u;
    g.level_words = static_cast<unsigned long long>(g.wx) * static_cast<unsigned long long>(g.dims[1]) * static_cast<unsigned long long>(g.dims[2]);
    const double bytes = 4.0 * static_cast<double>(g.wx) * g.dims[1] * g.dims[2] * (levels + 1);
    if (bytes > static_cast<double>(kOccMaxBytes))
        return fail(KICP_ERR_CAPACITY, "the occupancy pyramid would need " + std::to_string(static_cast<unsigned long long>(bytes)) + " bytes (" + std::to_string(g.dims[0]) +
                                           " x " + std::to_string(g.dims[1]) + " x " + std::to_string(g.dims[2]) + " cells, " + std::to_string(levels + 1) +
                                           " levels; limit 1 GiB)");
    const size_t words = static_cast<size_t>(g.level_words) * (levels + 1);
    if (int rc = occ->bits.reserve(words)) return rc;
    HIP_TRY(hipMemsetAsync(occ->bits.get(), 0, static_cast<size_t>(g.level_words) * sizeof(uint32_t), st));
    if (!empty) {
        hipLaunchKernelGGL(k_occ_mark, dim3((slots + 255u) / 256u), dim3(256), 0, st, map->mirror.d_table.get(), slots, map->mirror.d_pool.get(), view->cap, view->cbits,
                           g, dilate, occ->bits.get());
        HIP_TRY(hipGetLastError());
    }
    const uint32_t pool_grid = static_cast<uint32_t>((g.level_words + 255) / 256);
    for (int h = 1; h <= levels; ++h)
        hipLaunchKernelGGL(k_occ_pool, dim3(pool_grid), dim3(256), 0, st, occ->bits.get() + static_cast<size_t>(h - 1) * g.level_words,
                           occ->bits.get() + static_cast<size_t>(h) * g.level_words, g, 1u << (h - 1));
    HIP_TRY(hipGetLastError());
    DevBuf<unsigned long long> d_count;
    if (int rc = d_count.reserve(1)) return rc;
    HIP_TRY(hipMemsetAsync(d_count.get(), 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_occ_count, dim3(std::min(pool_grid, 2048u)), dim3(256), 0, st, occ->bits.get(), g.level_words, d_count.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&occ->set_cells, d_count.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *out = occ.release();
    return KICP_OK;
}
void kicp_occ_destroy(kicp_occ *occ) {
    if (!occ) return;
    (void)hipSetDevice(occ->device);
    delete occ;
}
int kicp_occ_info(const kicp_occ *occ, double out_min[3], int out_dims[3], double *out_cell, int *out_dilate, int *out_levels,
                  unsigned long long *out_set_cells) {
    if (!occ) return fail(KICP_ERR_ARG, "null argument");
    for (int a = 0; a < 3; ++a) {
        if (out_min) out_min[a] = occ->grid.min[a];
        if (out_dims) out_dims[a] = occ->grid.dims[a];
    }
    if (out_cell) *out_cell = occ->grid.cell;
    if (out_dilate) *out_dilate = occ->dilate;
    if (out_levels) *out_levels = occ->levels;
    if (out_set_cells) *out_set_cells = occ->set_cells;
    return KICP_OK;
}
int kicp_occ_level(const kicp_occ *occ, int level, unsigned int *out_words, size_t cap_words, size_t *out_total_words) {
    if (!occ || (!out_words && cap_words)) return fail(KICP_ERR_ARG, "null argument");
    if (level < 0 || level > occ->levels) return fail(KICP_ERR_ARG, "level must be 0 .. levels");
    const size_t total = static_cast<size_t>(occ->grid.level_words);
    if (out_total_words) *out_total_words = total;
    const size_t want = std::min(cap_words, total);
    if (want == 0) return KICP_OK;
    if (int rc = set_device(occ->device)) return rc;
    HIP_TRY(hipMemcpy(out_words, occ->bits.get() + static_cast<size_t>(level) * total, want * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return KICP_OK;
}

int kicp_search_yaws(const kicp_search_window *w, double *out_cs) {
    if (!out_cs) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_window(w)) return rc;
    yaw_table(w, out_cs);
    return KICP_OK;
}
int kicp_search_window_around(const kicp_occ *occ, const double center_xy[2], double half_x, double half_y, double z, double yaw_step,
                              kicp_search_window *out) {
    if (!occ || !out || (!center_xy && (half_x > 0.0 || half_y > 0.0))) return fail(KICP_ERR_ARG, "null argument");
    const OccGrid &g = occ->grid;
    kicp_search_window w{};
    auto axis = [&](int a, double half, double &origin, unsigned int &count) {
        if (half > 0.0) {
            const double k = std::floor(half / g.cell + 1e-9);
            if (!(k < 0.5 * kSearchMaxAxis)) return false;
            origin = center_xy[a] - k * g.cell, count = 2u * static_cast<unsigned int>(k) + 1u;
        } else {
            origin = g.min[a], count = static_cast<unsigned int>(g.dims[a]);
        }
        return count <= kSearchMaxAxis;
    };
    if (!axis(0, half_x, w.x0, w.nx) || !axis(1, half_y, w.y0, w.ny)) return fail(KICP_ERR_CAPACITY, "the window would have more than 2^20 nodes along an axis");
    w.z = z;
    if (yaw_step > 0.0) {
        const double steps = std::ceil(kTwoPi / yaw_step - 1e-9);
        if (!(steps <= kSearchMaxYaws)) return fail(KICP_ERR_CAPACITY, "the window would have more than 2^16 yaws");
        w.nyaw = std::max(1u, static_cast<unsigned int>(steps));
        w.yaw0 = -0.5 * kTwoPi, w.yaw_step = kTwoPi / static_cast<double>(w.nyaw);
    } else {
        w.nyaw = 1, w.yaw0 = 0.0, w.yaw_step = 0.0;
    }
    if (int rc = check_window(&w)) return rc;
    *out = w;
    return KICP_OK;
}

int kicp_occ_score_nodes(kicp_reg *reg, const kicp_occ *occ, const double *frame_xyz, size_t n, const kicp_search_window *w, int level,
                         const unsigned long long *nodes, size_t count, unsigned int *out_hits) {
    KICP_TRACE_CALL();
    if (int rc = check_search_args(reg, occ, frame_xyz, n, w)) return rc;
    if (count && (!nodes || !out_hits)) return fail(KICP_ERR_ARG, "null argument");
    if (level < 0 || level > occ->levels) return fail(KICP_ERR_ARG, "level must be 0 .. levels");
    const unsigned long long total = window_nodes(w);
    for (size_t k = 0; k < count; ++k)
        if (nodes[k] >= total) return fail(KICP_ERR_ARG, "node index " + std::to_string(nodes[k]) + " beyond the window's " + std::to_string(total) + " nodes");
    reg->search_launches = 0, reg->search_nodes_scored = count;
    for (size_t k = 0; k < count; ++k) out_hits[k] = 0u;
    if (n == 0 || count == 0) return KICP_OK;
    if (int rc = prepare_cells(reg, occ, frame_xyz, n, w)) return rc;
    return score_prepared(reg, occ, n, w, level, nodes, count, out_hits);
}

int kicp_search_poses(kicp_reg *reg, const kicp_occ *occ, const double *frame_xyz, size_t n, const kicp_search_window *w, size_t top_m,
                      unsigned long long *out_nodes, unsigned int *out_hits, double *out_poses_qt, size_t *out_found) {
    KICP_TRACE_CALL();
    if (int rc = check_search_args(reg, occ, frame_xyz, n, w)) return rc;
    if (!out_nodes || !out_hits || !out_found) return fail(KICP_ERR_ARG, "null argument");
    if (top_m == 0) return fail(KICP_ERR_ARG, "kicp_search_poses needs top_m >= 1");
    std::vector<SearchHit> found;
    if (int rc = search_device(reg, occ, frame_xyz, n, w, top_m, found)) return rc;
    for (size_t k = 0; k < found.size(); ++k) {
        out_nodes[k] = found[k].node, out_hits[k] = found[k].hits;
        if (out_poses_qt) node_pose(w, occ->grid.cell, found[k].node, out_poses_qt + 7 * k);
    }
    *out_found = found.size();
    return KICP_OK;
}

int kicp_relocalize_search(kicp_reg *reg, kicp_map *map, const kicp_occ *occ, const double *frame_xyz, size_t n, const kicp_search_window *w,
                           double max_correspondence_distance, size_t top_m, int max_iterations, double convergence, double out_pose_qt[7],
                           unsigned long long *out_node, double *out_cost_before, double *out_cost_after) {
    KICP_TRACE_CALL();
    if (!map || !out_pose_qt) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_search_args(reg, occ, frame_xyz, n, w)) return rc;
    if (top_m == 0) return fail(KICP_ERR_ARG, "kicp_relocalize_search needs top_m >= 1");
    if (max_iterations < 1 || !(convergence >= 0.0)) return fail(KICP_ERR_ARG, "max_iterations must be >= 1 and convergence >= 0");
    std::vector<SearchHit> found;
    if (int rc = search_device(reg, occ, frame_xyz, n, w, top_m, found)) return rc;
    std::vector<double> poses(7 * found.size());
    for (size_t k = 0; k < found.size(); ++k) node_pose(w, occ->grid.cell, found[k].node, &poses[7 * k]);
    size_t candidate = 0;
    const int rc = kicp_relocalize_planar(reg, map, frame_xyz, n, poses.data(), found.size(), max_correspondence_distance, found.size(), max_iterations, convergence,
                                          out_pose_qt, &candidate, out_cost_before, out_cost_after);
    if (rc >= 0 && out_node) *out_node = found[candidate].node;
    return rc;
}

}  // extern "C"
