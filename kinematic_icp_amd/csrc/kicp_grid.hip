// kicp_grid.hip -- the 2-D occupancy grid a mapping run draws beside its voxel map (kicp_grid_*; include/kicp.h states the semantics):
// per frame the used points' endpoint cells are HIT and the cells their rays cross are MISS, once per cell per frame.  Kernels:
// kicp_grid.hpp; the geometry they share with the host entries: kicp_grid_host.hpp.  A handle owns its stream, its staging buffer and
// its device memory: the counters (cells x 2 x 16 bit) and the two frame-local planes over the window.  The clearance and the costmap
// a planner reads off the counters (kicp_grid_clearance, kicp_grid_costmap; kernels: kicp_clear.hpp, arithmetic: kicp_clear_host.hpp)
// are entries of the same handle, and so is the cost-to-go field a planner spreads over that costmap (kicp_grid_potential,
// kicp_grid_potential_of_costmap; kernels: kicp_nav.hpp, arithmetic: kicp_nav_host.hpp; the pure-host kicp_plan_weights,
// kicp_potential_from_costmap and kicp_potential_path live here too).  A successful potential call leaves a PLAN in the handle - q and
// the potential, where they lie in HBM - on which kicp_grid_score_arcs scores a fan of arc trajectories (kernel: kicp_arcs.hpp,
// arithmetic: kicp_arcs_host.hpp; its host twin kicp_score_arcs_from_plan and the helpers kicp_plan_q, kicp_arc_steps,
// kicp_footprint_box and kicp_arcs_best are here as well).  The exploration frontiers of the counters - the free cells that border
// unknown space, grouped and ranked by that plan - are kicp_grid_frontiers (kernels: kicp_front.hpp, arithmetic: kicp_front_host.hpp;
// host twin: kicp_frontiers_from_occupancy).  What a sensor would see of the unknown cells from candidate viewpoints - such as those
// frontiers' best cells - is kicp_grid_gain (kernels: kicp_gain.hpp, arithmetic: kicp_gain_host.hpp; host twin:
// kicp_gain_from_occupancy).
#include <cerrno>
#include <memory>

#include "kicp_arcs.hpp"
#include "kicp_clear.hpp"
#include "kicp_front.hpp"
#include "kicp_gain.hpp"
#include "kicp_grid.hpp"
#include "kicp_internal.hpp"
#include "kicp_nav.hpp"

using namespace kicp;
using namespace kicp::host;

struct kicp_grid {
    int device = 0;
    kicp_grid_config cfg{};
    GridGeom geom{};
    size_t cells = 0;
    uint32_t plane_words = 0;  // ceil((2 reach + 1)^2 / 4)
    unsigned long long frames = 0;
    bool has_window = false;  // a frame has been integrated since creation or the last clear: (win_x0, win_y0) is its window's lower corner
    int32_t win_x0 = 0, win_y0 = 0;
    hipStream_t stream = nullptr;
    DevBuf<uint16_t> d_counts;          // cells x 2: hits, misses
    DevBuf<uint32_t> d_hit, d_miss;     // the planes, zero between frames
    DevBuf<unsigned int> d_stats;       // used, cells HIT, cells MISS of the frame in flight, and the length of d_rays
    DevBuf<uint32_t> d_rays;            // the frame's ray list: the window cells that became HIT (room for one per point)
    PinnedBuf<unsigned int> h_stats;
    DevBuf<double> d_frame;             // kicp_grid_integrate's upload
    DevBuf<int8_t> d_occupancy;         // kicp_grid_occupancy's readout
    DevBuf<uint8_t> d_coldist;          // kicp_grid_clearance / kicp_grid_costmap: the column distances, the caller's table and the result
    DevBuf<uint8_t> d_cost_table, d_cost;
    DevBuf<uint16_t> d_clearance;
    DevBuf<uint32_t> d_pot, d_goals;    // kicp_grid_potential*: the potential, the goal list, q = weight[costmap], the weight table,
    DevBuf<uint8_t> d_q, d_weight;      // the tiles' activity flags (two planes) and the counters: raised flags of each round of a
    DevBuf<uint8_t> d_nav_flags;        // batch, then the cells below and at max_potential
    DevBuf<uint32_t> d_nav_ctr;
    PinnedBuf<uint32_t> h_nav;
    bool plan_valid = false;             // d_q and d_pot hold the plan of the last potential call, and it succeeded (kicp_grid_score_arcs)
    DevBuf<double> d_arcs, d_footprint;  // kicp_grid_score_arcs: its uploads, its results and the pinned buffer they come back through
    DevBuf<uint32_t> d_arc_out;
    PinnedBuf<uint32_t> h_arc_out;
    DevBuf<uint8_t> d_front_flags;       // kicp_grid_frontiers: a byte per cell, the parent plane that becomes the label plane, the roots'
    DevBuf<uint32_t> d_front_parent, d_front_row_of, d_front_ctr;  // row numbers, the count of roots, the rows and where they and the
    DevBuf<unsigned long long> d_front_rows;                       // count land
    PinnedBuf<uint32_t> h_front_ctr;
    std::vector<unsigned long long> h_front_rows;
    DevBuf<uint8_t> d_gain_classes;      // kicp_grid_gain: a byte per cell, the viewpoints' upload, their rows and the pinned buffer the
    DevBuf<uint32_t> d_gain_views, d_gain_out;  // rows come back through
    PinnedBuf<uint32_t> h_gain_out;
    HostStage stage;
    ~kicp_grid() {
        if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
    }
};

namespace {
constexpr size_t kGridMaxPoints = 0x7FFFFFF0ull / 3;

int check_thresholds(double occupied_thresh, double free_thresh) {
    if (!(0.0 <= free_thresh && free_thresh < occupied_thresh && occupied_thresh <= 1.0))
        return fail(KICP_ERR_ARG, "thresholds must satisfy 0 <= free_thresh < occupied_thresh <= 1");
    return KICP_OK;
}
// the frame at d_xyz (n points; arguments checked): three launches, the statistics back, the stream drained
int integrate_on_device(kicp_grid *grid, const double *d_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], unsigned long long out_stats[4]) {
    unsigned long long stats[4] = {0, n, 0, 0};
    const GridFrame f = grid_frame(grid->geom, pose_qt, sensor_xyz);
    grid->has_window = true, grid->win_x0 = f.gx0, grid->win_y0 = f.gy0;
    if (n) {
        hipStream_t st = grid->stream;
        if (n > grid->d_rays.capacity()) {
            HIP_TRY(hipStreamSynchronize(st));
            if (int rc = grid->d_rays.reserve(n + n / 2)) return rc;
        }
        HIP_TRY(hipMemsetAsync(grid->d_stats.get(), 0, 4 * sizeof(unsigned int), st));
        const uint32_t blocks = static_cast<uint32_t>((n + kGridBlock - 1) / kGridBlock);
        hipLaunchKernelGGL(k_grid_mark, dim3(blocks), dim3(kGridBlock), 0, st, d_xyz, static_cast<uint32_t>(n), grid->geom, f, grid->d_hit.get(), grid->d_rays.get(),
                           grid->d_stats.get());
        // one wave per ray, at most one ray per point; the waves of up to 2048 workgroups stride over the list, whose length is on the device
        hipLaunchKernelGGL(k_grid_rays, dim3(std::min(blocks, 2048u)), dim3(kGridBlock), 0, st, grid->d_rays.get(), grid->d_stats.get() + 3, grid->geom.reach,
                           reinterpret_cast<uint8_t *>(grid->d_miss.get()));
        hipLaunchKernelGGL(k_grid_apply, dim3((grid->plane_words + kGridBlock - 1) / kGridBlock), dim3(kGridBlock), 0, st, grid->d_hit.get(), grid->d_miss.get(),
                           grid->plane_words, grid->geom, f, grid->d_counts.get(), grid->d_stats.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(grid->h_stats.get(), grid->d_stats.get(), 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const unsigned int *h = grid->h_stats.get();
        stats[0] = h[0], stats[1] = n - h[0], stats[2] = h[1], stats[3] = h[2];
    }
    ++grid->frames;
    if (out_stats)
        for (int k = 0; k < 4; ++k) out_stats[k] = stats[k];
    return KICP_OK;
}
int check_frame_args(const kicp_grid *grid, const double *xyz, size_t n, const double *pose_qt, const double *sensor_xyz) {
    if (!grid || !pose_qt || !sensor_xyz || (!xyz && n)) return fail(KICP_ERR_ARG, "null argument");
    if (n > kGridMaxPoints) return fail(KICP_ERR_CAPACITY, "frame too large");
    return KICP_OK;
}
// the configuration of a clearance call as the kernels take it
int check_clear_config(const kicp_grid_clearance_config *cfg, ClearParams &p) {
    if (cfg->min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    if (!(0.0 <= cfg->occupied_thresh && cfg->occupied_thresh <= 1.0)) return fail(KICP_ERR_ARG, "occupied_thresh must lie in [0, 1]");
    if (cfg->radius_cells < 1) return fail(KICP_ERR_ARG, "radius_cells must be at least 1");
    if (cfg->radius_cells > kClearMaxRadius)
        return fail(KICP_ERR_CAPACITY, "radius_cells = " + std::to_string(cfg->radius_cells) + " (limit " + std::to_string(kClearMaxRadius) + ")");
    p = ClearParams{cfg->min_observations, clear_source_min(cfg->occupied_thresh), cfg->unknown_is_obstacle ? 1u : 0u, static_cast<uint32_t>(cfg->radius_cells)};
    return KICP_OK;
}
int check_clear_rect(unsigned int width, unsigned int height, const ClearRect &r, size_t cap) {
    if (r.w < 1u || r.h < 1u || r.x0 >= width || r.y0 >= height || r.w > width - r.x0 || r.h > height - r.y0)
        return fail(KICP_ERR_ARG, "the rectangle must lie inside the grid of " + std::to_string(width) + " x " + std::to_string(height) + " cells, w and h at least 1");
    if (cap != static_cast<size_t>(r.w) * r.h) return fail(KICP_ERR_ARG, "cap must be w * h = " + std::to_string(static_cast<size_t>(r.w) * r.h));
    return KICP_OK;
}
int check_cost_table(const ClearParams &p, size_t table_len) {
    if (table_len != static_cast<size_t>(clear_far(p.radius)) + 1u)
        return fail(KICP_ERR_ARG, "the table must have radius_cells^2 + 2 = " + std::to_string(clear_far(p.radius) + 1u) + " entries");
    return KICP_OK;
}
// The clearance (table == nullptr: 16 bits per cell into `out`) or the costmap (a byte per cell) of a rectangle; arguments checked.
// Two launches, one copy, the stream drained.  The buffers grow while the stream is idle: every entry of the handle drains it.
// out == nullptr: the costmap stays in d_cost for the launches the caller queues behind these; nothing is copied or waited for.
int clear_on_device(kicp_grid *grid, const ClearParams &p, const ClearRect &r, const unsigned char *table, uint32_t inflate_unknown, void *out) {
    if (int rc = set_device(grid->device)) return rc;
    const size_t cells = static_cast<size_t>(r.w) * r.h;
    uint32_t cx0, cx1;
    clear_host::column_range(grid->cfg.width, r, p.radius, cx0, cx1);
    const uint32_t cw = cx1 - cx0;
    hipStream_t st = grid->stream;
    if (int rc = grid->d_coldist.reserve(static_cast<size_t>(cw) * r.h)) return rc;
    if (table) {
        if (int rc = grid->d_cost.reserve(cells)) return rc;
        if (int rc = grid->d_cost_table.reserve(static_cast<size_t>(clear_far(kClearMaxRadius)) + 1u)) return rc;
        HIP_TRY(hipMemcpyAsync(grid->d_cost_table.get(), table, static_cast<size_t>(clear_far(p.radius)) + 1u, hipMemcpyHostToDevice, st));
    } else if (int rc = grid->d_clearance.reserve(cells)) {
        return rc;
    }
    // a strip of at least R rows keeps the rows a workgroup reads beside its own at or below twice its own
    const uint32_t strip = std::max(32u, p.radius), strips = (r.h + strip - 1u) / strip, col_blocks = (cw + kClearBlock - 1u) / kClearBlock;
    const uint32_t segments = (r.w + kClearSegment - 1u) / kClearSegment;  // (both products stay below 2^29: cells <= 2^28)
    hipLaunchKernelGGL(k_clear_columns, dim3(strips * col_blocks), dim3(kClearBlock), 0, st, grid->d_counts.get(), grid->cfg.width, grid->cfg.height, p, r, cx0, cw, strip,
                       col_blocks, grid->d_coldist.get());
    if (table)
        hipLaunchKernelGGL(k_clear_rows<true>, dim3(r.h * segments), dim3(kClearBlock), 0, st, grid->d_coldist.get(), cx0, cw, grid->d_counts.get(), grid->cfg.width, p, r,
                           segments, grid->d_cost_table.get(), inflate_unknown, static_cast<void *>(grid->d_cost.get()));
    else
        hipLaunchKernelGGL(k_clear_rows<false>, dim3(r.h * segments), dim3(kClearBlock), 0, st, grid->d_coldist.get(), cx0, cw, grid->d_counts.get(), grid->cfg.width, p, r,
                           segments, static_cast<const uint8_t *>(nullptr), 0u, static_cast<void *>(grid->d_clearance.get()));
    HIP_TRY(hipGetLastError());
    if (!out) return KICP_OK;
    if (table)
        HIP_TRY(hipMemcpyAsync(out, grid->d_cost.get(), cells, hipMemcpyDeviceToHost, st));
    else
        HIP_TRY(hipMemcpyAsync(out, grid->d_clearance.get(), cells * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return KICP_OK;
}
// what the potential entries share: the configuration, the output's size and the goal list
int check_plan_args(const kicp_plan_config *cfg, unsigned int width, unsigned int height, const unsigned int *goals, size_t n_goals, size_t cap) {
    if (cfg->max_potential < 1u || cfg->max_potential > kNavMaxPotential) return fail(KICP_ERR_ARG, "max_potential must lie in 1 .. 0xFFFFFFFE");
    if (cap != static_cast<size_t>(width) * height) return fail(KICP_ERR_ARG, "cap must be width * height = " + std::to_string(static_cast<size_t>(width) * height));
    if (n_goals < 1u) return fail(KICP_ERR_ARG, "at least one goal is needed");
    if (n_goals > kGridMaxCells) return fail(KICP_ERR_CAPACITY, "n_goals = " + std::to_string(n_goals) + " (limit 2^28 = " + std::to_string(kGridMaxCells) + ")");
    for (size_t g = 0; g < n_goals; ++g)
        if (goals[2 * g] >= width || goals[2 * g + 1] >= height)
            return fail(KICP_ERR_ARG, "goal " + std::to_string(g) + " = (" + std::to_string(goals[2 * g]) + ", " + std::to_string(goals[2 * g + 1]) + ") lies outside the grid of " +
                                          std::to_string(width) + " x " + std::to_string(height) + " cells");
    return KICP_OK;
}
// The potential over the costmap at d_costmap (the grid's width x height bytes, written by work already queued on the stream);
// arguments checked.  Two launches, rounds of k_nav_relax in batches of kNavBatch with a look at their counters after each batch, the
// count, one copy of the result, the stream drained.
int potential_on_device(kicp_grid *grid, const uint8_t *d_costmap, const unsigned char *weight, uint32_t max_potential, const unsigned int *goals, size_t n_goals,
                        unsigned int *out, unsigned long long out_stats[4]) {
    const uint32_t width = grid->cfg.width, height = grid->cfg.height, cells = static_cast<uint32_t>(grid->cells);
    const uint32_t tiles_x = (width + kNavTile - 1u) / kNavTile, tiles_y = (height + kNavTile - 1u) / kNavTile, tiles = tiles_x * tiles_y;
    hipStream_t st = grid->stream;
    grid->plan_valid = false;  // until this call has succeeded
    if (int rc = grid->d_pot.reserve(cells)) return rc;
    if (int rc = grid->d_q.reserve(cells)) return rc;
    if (int rc = grid->d_nav_flags.reserve(2 * static_cast<size_t>(tiles))) return rc;
    if (int rc = grid->d_weight.reserve(256)) return rc;
    if (int rc = grid->d_goals.reserve(2 * n_goals)) return rc;
    if (int rc = grid->d_nav_ctr.reserve(kNavBatch + 2u)) return rc;
    if (int rc = grid->h_nav.reserve(kNavBatch + 2u, hipHostMallocDefault, false)) return rc;
    uint8_t *flags = grid->d_nav_flags.get();
    uint32_t *ctr = grid->d_nav_ctr.get(), *h = grid->h_nav.get();
    HIP_TRY(hipMemcpyAsync(grid->d_weight.get(), weight, 256, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(grid->d_goals.get(), goals, 2 * n_goals * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(flags, 0, 2 * static_cast<size_t>(tiles), st));
    HIP_TRY(hipMemsetAsync(ctr, 0, (kNavBatch + 2u) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_nav_init, dim3((cells + kNavBlock - 1u) / kNavBlock), dim3(kNavBlock), 0, st, d_costmap, grid->d_weight.get(), cells, grid->d_q.get(),
                       grid->d_pot.get());
    hipLaunchKernelGGL(k_nav_goals, dim3(static_cast<uint32_t>((n_goals + kNavBlock - 1u) / kNavBlock)), dim3(kNavBlock), 0, st, grid->d_goals.get(),
                       static_cast<uint32_t>(n_goals), width, tiles_x, grid->d_q.get(), grid->d_pot.get(), flags);
    // A round holds a full sweep of every active tile, so the rounds end within the number of cells; never loop without that limit.
    const unsigned long long limit = static_cast<unsigned long long>(cells) + 1ull;
    unsigned long long rounds = 0;
    for (bool done = false; !done;) {
        if (rounds >= limit) return fail(KICP_ERR_INTERNAL, "the potential did not settle within " + std::to_string(limit) + " rounds");
        const uint32_t batch = static_cast<uint32_t>(std::min<unsigned long long>(kNavBatch, limit - rounds));
        for (uint32_t i = 0; i < batch; ++i) {
            const uint32_t parity = static_cast<uint32_t>((rounds + i) & 1ull);
            hipLaunchKernelGGL(k_nav_relax, dim3(tiles), dim3(kNavBlock), 0, st, grid->d_pot.get(), grid->d_q.get(), width, height, tiles_x, tiles_y, max_potential,
                               flags + static_cast<size_t>(parity) * tiles, flags + static_cast<size_t>(parity ^ 1u) * tiles, ctr + i);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, ctr, kNavBatch * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemsetAsync(ctr, 0, kNavBatch * sizeof(uint32_t), st));
        HIP_TRY(hipStreamSynchronize(st));
        uint32_t i = 0;
        while (i < batch && h[i] != 0u) ++i;  // the first round that raised no flag: every later one found no tile active
        done = i < batch;
        rounds += done ? i + 1u : batch;
    }
    hipLaunchKernelGGL(k_nav_count, dim3(std::min((cells + kNavBlock - 1u) / kNavBlock, 1024u)), dim3(kNavBlock), 0, st, grid->d_pot.get(), cells, max_potential,
                       ctr + kNavBatch);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, grid->d_pot.get(), static_cast<size_t>(cells) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h + kNavBatch, ctr + kNavBatch, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (out_stats) {
        out_stats[0] = 0ull, out_stats[1] = h[kNavBatch], out_stats[2] = h[kNavBatch + 1u], out_stats[3] = rounds;
        for (size_t g = 0; g < n_goals; ++g) out_stats[0] += out[static_cast<size_t>(goals[2 * g + 1]) * width + goals[2 * g]] == 0u ? 1ull : 0ull;  // 0 only on a passable goal
    }
    grid->plan_valid = true;
    return KICP_OK;
}
// what the entries that take a list of arcs share
int check_arc_count(size_t n_arcs) {
    if (n_arcs < 1u) return fail(KICP_ERR_ARG, "at least one arc is needed");
    if (n_arcs > kArcsMaxK) return fail(KICP_ERR_CAPACITY, "n_arcs = " + std::to_string(n_arcs) + " (limit 2^20 = " + std::to_string(kArcsMaxK) + ")");
    return KICP_OK;
}
// what the two scoring entries share
int check_arcs_args(const double *start, const double *arcs, size_t n_arcs, unsigned int n_steps, const double *footprint_xy, size_t n_samples, const unsigned int *out,
                    size_t cap) {
    if (!start || !arcs || !footprint_xy || !out) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_arc_count(n_arcs)) return rc;
    if (n_steps < 1u) return fail(KICP_ERR_ARG, "at least one step is needed");
    if (n_steps > kArcsMaxT) return fail(KICP_ERR_CAPACITY, "n_steps = " + std::to_string(n_steps) + " (limit " + std::to_string(kArcsMaxT) + ")");
    if (n_samples < 1u) return fail(KICP_ERR_ARG, "at least one footprint sample is needed");
    if (n_samples > kArcsMaxP) return fail(KICP_ERR_CAPACITY, "n_samples = " + std::to_string(n_samples) + " (limit " + std::to_string(kArcsMaxP) + ")");
    if (cap != 4 * n_arcs) return fail(KICP_ERR_ARG, "cap must be 4 * n_arcs = " + std::to_string(4 * n_arcs));
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(start[i])) return fail(KICP_ERR_ARG, "the start (x, y, cosine, sine) must be finite");
    return KICP_OK;
}
// what the two frontier entries share: the configuration, and the two outputs with their capacities
int check_front_args(const kicp_frontier_config *cfg, size_t cells, const unsigned long long *out_rows, size_t cap_rows, const unsigned int *out_labels, size_t cap_labels,
                     FrontParams &p) {
    if (cfg->min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    if (!(0.0 <= cfg->occupied_thresh && cfg->occupied_thresh <= 1.0)) return fail(KICP_ERR_ARG, "occupied_thresh must lie in [0, 1]");
    if (cfg->min_size < 1u) return fail(KICP_ERR_ARG, "min_size must be at least 1");
    if (!out_rows && cap_rows) return fail(KICP_ERR_ARG, "out_rows may be null only when cap_rows is 0");
    if (cap_labels != 0u && cap_labels != cells) return fail(KICP_ERR_ARG, "cap_labels must be 0 or width * height = " + std::to_string(cells));
    if ((out_labels == nullptr) != (cap_labels == 0u)) return fail(KICP_ERR_ARG, "out_labels must be null exactly when cap_labels is 0");
    p = FrontParams{cfg->min_observations, clear_source_min(cfg->occupied_thresh)};
    return KICP_OK;
}
int front_result(size_t n, size_t cap_rows, size_t *out_n) {
    *out_n = n;
    if (n > cap_rows) return fail(KICP_ERR_CAPACITY, std::to_string(n) + " frontiers pass the filter, cap_rows is " + std::to_string(cap_rows));
    return KICP_OK;
}
constexpr size_t kGainMaxViews = 1u << 24;  // viewpoints per call: one workgroup each
// what the two gain entries share: the configuration, the viewpoints - each a cell index below `cells` - and the output
int check_gain_args(const kicp_gain_config *cfg, size_t cells, const unsigned int *views, size_t n_views, const unsigned int *out, size_t cap_out, GainParams &p) {
    if (cfg->min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    if (!(0.0 <= cfg->occupied_thresh && cfg->occupied_thresh <= 1.0)) return fail(KICP_ERR_ARG, "occupied_thresh must lie in [0, 1]");
    if (cfg->range_cells < 1u || cfg->range_cells > kGainMaxRange) return fail(KICP_ERR_ARG, "range_cells must lie in 1 .. " + std::to_string(kGainMaxRange));
    if (n_views > kGainMaxViews) return fail(KICP_ERR_CAPACITY, "n_views = " + std::to_string(n_views) + " (limit 2^24 = " + std::to_string(kGainMaxViews) + ")");
    if (n_views && (!views || !out)) return fail(KICP_ERR_ARG, "views and out may be null only when n_views is 0");
    if (cap_out != kGainWords * n_views) return fail(KICP_ERR_ARG, "cap_out must be 4 * n_views = " + std::to_string(kGainWords * n_views));
    for (size_t i = 0; i < n_views; ++i)
        if (views[i] >= cells)
            return fail(KICP_ERR_ARG, "viewpoint " + std::to_string(i) + " is cell " + std::to_string(views[i]) + ", outside the grid's " + std::to_string(cells) + " cells");
    p = GainParams{cfg->min_observations, clear_source_min(cfg->occupied_thresh), cfg->range_cells};
    return KICP_OK;
}
}  // namespace

extern "C" {

int kicp_grid_create(const kicp_grid_config *cfg, int device, kicp_grid **out) {
    KICP_TRACE_CALL();
    if (!cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    *out = nullptr;
    if (!(cfg->cell > 0.0) || !std::isfinite(cfg->cell)) return fail(KICP_ERR_ARG, "cell must be positive and finite");
    if (!(cfg->max_ray > 0.0) || !std::isfinite(cfg->max_ray)) return fail(KICP_ERR_ARG, "max_ray must be positive and finite");
    if (!std::isfinite(cfg->origin_x) || !std::isfinite(cfg->origin_y)) return fail(KICP_ERR_ARG, "the origin must be finite");
    if (!(cfg->z_min < cfg->z_max)) return fail(KICP_ERR_ARG, "the band needs z_min < z_max");
    if (cfg->width == 0 || cfg->height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    const unsigned long long cells = static_cast<unsigned long long>(cfg->width) * cfg->height;
    if (cells > kGridMaxCells)
        return fail(KICP_ERR_CAPACITY, "the grid would have " + std::to_string(cfg->width) + " x " + std::to_string(cfg->height) + " = " + std::to_string(cells) +
                                           " cells (limit 2^28 = " + std::to_string(kGridMaxCells) + ")");
    const double reach = std::ceil(cfg->max_ray / cfg->cell);
    if (!(reach <= static_cast<double>(kGridMaxReach)))
        return fail(KICP_ERR_CAPACITY, "max_ray / cell gives a reach of " + std::to_string(reach) + " cells (limit " + std::to_string(kGridMaxReach) + ")");
    if (int rc = set_device(device)) return rc;
    std::unique_ptr<kicp_grid> grid(new kicp_grid);
    grid->device = device, grid->cfg = *cfg, grid->cells = static_cast<size_t>(cells);
    grid->geom = GridGeom{cfg->cell, cfg->origin_x, cfg->origin_y, cfg->z_min, cfg->z_max, cfg->width, cfg->height, static_cast<int32_t>(reach)};
    const unsigned long long side = 2ull * static_cast<unsigned long long>(grid->geom.reach) + 1ull;
    grid->plane_words = static_cast<uint32_t>((side * side + 3ull) / 4ull);
    HIP_TRY(hipStreamCreateWithFlags(&grid->stream, hipStreamNonBlocking));
    if (int rc = grid->d_counts.reserve(2 * grid->cells)) return rc;
    if (int rc = grid->d_hit.reserve(grid->plane_words)) return rc;
    if (int rc = grid->d_miss.reserve(grid->plane_words)) return rc;
    if (int rc = grid->d_stats.reserve(4)) return rc;
    if (int rc = grid->h_stats.reserve(4, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemsetAsync(grid->d_counts.get(), 0, 2 * grid->cells * sizeof(uint16_t), grid->stream));
    HIP_TRY(hipMemsetAsync(grid->d_hit.get(), 0, grid->plane_words * sizeof(uint32_t), grid->stream));
    HIP_TRY(hipMemsetAsync(grid->d_miss.get(), 0, grid->plane_words * sizeof(uint32_t), grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    *out = grid.release();
    return KICP_OK;
}
void kicp_grid_destroy(kicp_grid *grid) {
    if (!grid) return;
    (void)hipSetDevice(grid->device);
    delete grid;
}
int kicp_grid_info(const kicp_grid *grid, kicp_grid_config *out_config, int *out_reach, unsigned long long *out_frames) {
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    if (out_config) *out_config = grid->cfg;
    if (out_reach) *out_reach = grid->geom.reach;
    if (out_frames) *out_frames = grid->frames;
    return KICP_OK;
}
int kicp_grid_clear(kicp_grid *grid) {
    KICP_TRACE_CALL();
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = set_device(grid->device)) return rc;
    HIP_TRY(hipMemsetAsync(grid->d_counts.get(), 0, 2 * grid->cells * sizeof(uint16_t), grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    grid->frames = 0, grid->has_window = false;
    return KICP_OK;
}
int kicp_grid_integrate(kicp_grid *grid, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(grid, frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    if (n) {
        if (3 * n > grid->d_frame.capacity()) {
            HIP_TRY(hipStreamSynchronize(grid->stream));
            if (int rc = grid->d_frame.reserve(3 * n + 3 * n / 2)) return rc;
        }
        if (int rc = staged_upload(grid->stage, 0, grid->d_frame.get(), frame_xyz, n * 24, grid->stream)) return rc;
    }
    return integrate_on_device(grid, grid->d_frame.get(), n, pose_qt, sensor_xyz, out_stats);
}
int kicp_grid_integrate_device(kicp_grid *grid, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                               unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(grid, d_frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    return integrate_on_device(grid, d_frame_xyz, n, pose_qt, sensor_xyz, out_stats);
}
int kicp_grid_counts(const kicp_grid *grid, unsigned short *out, size_t cap_cells) {
    KICP_TRACE_CALL();
    if (!grid || !out) return fail(KICP_ERR_ARG, "null argument");
    if (cap_cells != grid->cells) return fail(KICP_ERR_ARG, "cap_cells must be the grid's " + std::to_string(grid->cells) + " cells");
    if (int rc = set_device(grid->device)) return rc;
    HIP_TRY(hipMemcpyAsync(out, grid->d_counts.get(), 2 * grid->cells * sizeof(uint16_t), hipMemcpyDeviceToHost, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_set_counts(kicp_grid *grid, const unsigned short *in, size_t cells) {
    KICP_TRACE_CALL();
    if (!grid || !in) return fail(KICP_ERR_ARG, "null argument");
    if (cells != grid->cells) return fail(KICP_ERR_ARG, "cells must be the grid's " + std::to_string(grid->cells) + " cells");
    if (int rc = set_device(grid->device)) return rc;
    HIP_TRY(hipMemcpyAsync(grid->d_counts.get(), in, 2 * grid->cells * sizeof(uint16_t), hipMemcpyHostToDevice, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_occupancy(const kicp_grid *cgrid, unsigned int min_observations, signed char *out, size_t cap_cells) {
    KICP_TRACE_CALL();
    if (!cgrid || !out) return fail(KICP_ERR_ARG, "null argument");
    if (min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    if (cap_cells != cgrid->cells) return fail(KICP_ERR_ARG, "cap_cells must be the grid's " + std::to_string(cgrid->cells) + " cells");
    kicp_grid *grid = const_cast<kicp_grid *>(cgrid);  // logically const: the readout's buffer is scratch
    if (int rc = set_device(grid->device)) return rc;
    if (int rc = grid->d_occupancy.reserve(grid->cells)) return rc;
    hipLaunchKernelGGL(k_grid_readout, dim3(static_cast<uint32_t>((grid->cells + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, grid->stream,
                       grid->d_counts.get(), grid->cells, min_observations, grid->d_occupancy.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, grid->d_occupancy.get(), grid->cells, hipMemcpyDeviceToHost, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_occupancy_from_counts(const unsigned short *counts, size_t cells, unsigned int min_observations, signed char *out) {
    if ((!counts || !out) && cells) return fail(KICP_ERR_ARG, "null argument");
    if (min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    for (size_t i = 0; i < cells; ++i) out[i] = grid_readout(counts[2 * i], counts[2 * i + 1], min_observations);
    return KICP_OK;
}
int kicp_grid_clearance(const kicp_grid *cgrid, const kicp_grid_clearance_config *cfg, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h,
                        unsigned short *out, size_t cap) {
    KICP_TRACE_CALL();
    if (!cgrid || !cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    ClearParams p;
    const ClearRect r{x0, y0, w, h};
    if (int rc = check_clear_config(cfg, p)) return rc;
    if (int rc = check_clear_rect(cgrid->cfg.width, cgrid->cfg.height, r, cap)) return rc;
    return clear_on_device(const_cast<kicp_grid *>(cgrid), p, r, nullptr, 0u, out);  // logically const: the buffers are scratch
}
int kicp_grid_costmap(const kicp_grid *cgrid, const kicp_grid_clearance_config *cfg, const unsigned char *table, size_t table_len, int inflate_unknown, unsigned int x0,
                      unsigned int y0, unsigned int w, unsigned int h, unsigned char *out, size_t cap) {
    KICP_TRACE_CALL();
    if (!cgrid || !cfg || !table || !out) return fail(KICP_ERR_ARG, "null argument");
    ClearParams p;
    const ClearRect r{x0, y0, w, h};
    if (int rc = check_clear_config(cfg, p)) return rc;
    if (int rc = check_cost_table(p, table_len)) return rc;
    if (int rc = check_clear_rect(cgrid->cfg.width, cgrid->cfg.height, r, cap)) return rc;
    return clear_on_device(const_cast<kicp_grid *>(cgrid), p, r, table, inflate_unknown ? 1u : 0u, out);
}
int kicp_grid_clearance_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_grid_clearance_config *cfg, unsigned int x0,
                                       unsigned int y0, unsigned int w, unsigned int h, unsigned short *out, size_t cap) {
    if (!occupancy || !cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    ClearParams p;
    const ClearRect r{x0, y0, w, h};
    if (int rc = check_clear_config(cfg, p)) return rc;
    if (int rc = check_clear_rect(width, height, r, cap)) return rc;
    clear_host::clearance(reinterpret_cast<const int8_t *>(occupancy), width, height, p, r, out);
    return KICP_OK;
}
int kicp_grid_costmap_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_grid_clearance_config *cfg,
                                     const unsigned char *table, size_t table_len, int inflate_unknown, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h,
                                     unsigned char *out, size_t cap) {
    if (!occupancy || !cfg || !table || !out) return fail(KICP_ERR_ARG, "null argument");
    ClearParams p;
    const ClearRect r{x0, y0, w, h};
    if (int rc = check_clear_config(cfg, p)) return rc;
    if (int rc = check_cost_table(p, table_len)) return rc;
    if (int rc = check_clear_rect(width, height, r, cap)) return rc;
    clear_host::costmap(reinterpret_cast<const int8_t *>(occupancy), width, height, p, table, inflate_unknown ? 1u : 0u, r, out);
    return KICP_OK;
}
int kicp_grid_cost_table_nav2(double cell, int radius_cells, double inscribed_radius, double cost_scaling_factor, unsigned char *table, size_t cap) {
    if (!table) return fail(KICP_ERR_ARG, "null argument");
    if (radius_cells < 1) return fail(KICP_ERR_ARG, "radius_cells must be at least 1");
    if (radius_cells > kClearMaxRadius)
        return fail(KICP_ERR_CAPACITY, "radius_cells = " + std::to_string(radius_cells) + " (limit " + std::to_string(kClearMaxRadius) + ")");
    if (!(cell > 0.0) || !std::isfinite(cell)) return fail(KICP_ERR_ARG, "cell must be positive and finite");
    if (!(inscribed_radius >= 0.0) || !std::isfinite(inscribed_radius) || !(cost_scaling_factor >= 0.0) || !std::isfinite(cost_scaling_factor))
        return fail(KICP_ERR_ARG, "inscribed_radius and cost_scaling_factor must be finite and not negative");
    const ClearParams p{1u, 0, 0u, static_cast<uint32_t>(radius_cells)};
    if (int rc = check_cost_table(p, cap)) return rc;
    clear_host::cost_table_nav2(cell, p.radius, inscribed_radius, cost_scaling_factor, table);
    return KICP_OK;
}
int kicp_plan_weights(unsigned int neutral, unsigned int factor_num, unsigned int factor_den, unsigned int lethal_from, unsigned int unknown_weight,
                      unsigned char out[256]) {
    if (!out) return fail(KICP_ERR_ARG, "null argument");
    if (neutral < 1u || neutral > 255u) return fail(KICP_ERR_ARG, "neutral must lie in 1 .. 255");
    if (factor_den < 1u) return fail(KICP_ERR_ARG, "factor_den must be at least 1");
    if (lethal_from > 255u) return fail(KICP_ERR_ARG, "lethal_from must lie in 0 .. 255");
    if (unknown_weight > 255u) return fail(KICP_ERR_ARG, "unknown_weight must lie in 0 .. 255");
    nav_host::weights(neutral, factor_num, factor_den, lethal_from, unknown_weight, out);
    return KICP_OK;
}
int kicp_potential_from_costmap(const unsigned char *costmap, unsigned int width, unsigned int height, const unsigned char weight[256], const kicp_plan_config *cfg,
                                const unsigned int *goals_xy, size_t n_goals, unsigned int *out, size_t cap, unsigned long long out_stats[4]) {
    if (!costmap || !weight || !cfg || !goals_xy || !out) return fail(KICP_ERR_ARG, "null argument");
    if (width == 0 || height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    if (static_cast<unsigned long long>(width) * height > kGridMaxCells) return fail(KICP_ERR_CAPACITY, "width * height exceeds 2^28 = " + std::to_string(kGridMaxCells));
    if (int rc = check_plan_args(cfg, width, height, goals_xy, n_goals, cap)) return rc;
    unsigned long long stats[4];
    nav_host::potential(costmap, width, height, weight, cfg->max_potential, goals_xy, n_goals, out, stats);
    if (out_stats)
        for (int k = 0; k < 4; ++k) out_stats[k] = stats[k];
    return KICP_OK;
}
int kicp_potential_path(const unsigned int *potential, const unsigned char *costmap, unsigned int width, unsigned int height, const unsigned char weight[256],
                        unsigned int start_x, unsigned int start_y, unsigned int *out_xy, size_t cap_cells, size_t *out_n) {
    if (!potential || !costmap || !weight || !out_n || (!out_xy && cap_cells)) return fail(KICP_ERR_ARG, "null argument");
    *out_n = 0;
    if (width == 0 || height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    if (start_x >= width || start_y >= height) return fail(KICP_ERR_ARG, "the start lies outside the grid of " + std::to_string(width) + " x " + std::to_string(height) + " cells");
    const int rc = nav_host::path(potential, costmap, width, height, weight, start_x, start_y, out_xy, cap_cells, out_n);
    if (rc == 1) return fail(KICP_ERR_ARG, "the start is unreachable: its potential is 0xFFFFFFFF");
    if (rc == 2) return fail(KICP_ERR_CAPACITY, "the path enters the zone that max_potential clamped: no neighbour continues it; raise max_potential");
    if (*out_n > cap_cells) return fail(KICP_ERR_CAPACITY, "the path has " + std::to_string(*out_n) + " cells, cap_cells is " + std::to_string(cap_cells));
    return KICP_OK;
}
int kicp_grid_potential_of_costmap(const kicp_grid *cgrid, const unsigned char *costmap, const unsigned char weight[256], const kicp_plan_config *cfg,
                                   const unsigned int *goals_xy, size_t n_goals, unsigned int *out, size_t cap, unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (cgrid) const_cast<kicp_grid *>(cgrid)->plan_valid = false;  // a call that fails, on its arguments too, leaves no plan
    if (!cgrid || !costmap || !weight || !cfg || !goals_xy || !out) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_plan_args(cfg, cgrid->cfg.width, cgrid->cfg.height, goals_xy, n_goals, cap)) return rc;
    kicp_grid *grid = const_cast<kicp_grid *>(cgrid);  // logically const: the buffers are scratch
    if (int rc = set_device(grid->device)) return rc;
    if (int rc = grid->d_cost.reserve(grid->cells)) return rc;
    HIP_TRY(hipMemcpyAsync(grid->d_cost.get(), costmap, grid->cells, hipMemcpyHostToDevice, grid->stream));
    return potential_on_device(grid, grid->d_cost.get(), weight, cfg->max_potential, goals_xy, n_goals, out, out_stats);
}
int kicp_grid_potential(const kicp_grid *cgrid, const kicp_grid_clearance_config *clearance, const unsigned char *table, size_t table_len, int inflate_unknown,
                        const unsigned char weight[256], const kicp_plan_config *cfg, const unsigned int *goals_xy, size_t n_goals, unsigned int *out, size_t cap,
                        unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (cgrid) const_cast<kicp_grid *>(cgrid)->plan_valid = false;
    if (!cgrid || !clearance || !table || !weight || !cfg || !goals_xy || !out) return fail(KICP_ERR_ARG, "null argument");
    ClearParams p;
    const ClearRect r{0u, 0u, cgrid->cfg.width, cgrid->cfg.height};
    if (int rc = check_clear_config(clearance, p)) return rc;
    if (int rc = check_cost_table(p, table_len)) return rc;
    if (int rc = check_plan_args(cfg, r.w, r.h, goals_xy, n_goals, cap)) return rc;
    kicp_grid *grid = const_cast<kicp_grid *>(cgrid);
    if (int rc = clear_on_device(grid, p, r, table, inflate_unknown ? 1u : 0u, nullptr)) return rc;  // the costmap stays in d_cost
    return potential_on_device(grid, grid->d_cost.get(), weight, cfg->max_potential, goals_xy, n_goals, out, out_stats);
}
int kicp_plan_q(const unsigned char *costmap, size_t cells, const unsigned char weight[256], unsigned char *out) {
    if (!weight || ((!costmap || !out) && cells)) return fail(KICP_ERR_ARG, "null argument");
    for (size_t c = 0; c < cells; ++c) out[c] = weight[costmap[c]];
    return KICP_OK;
}
int kicp_arc_steps(const double *v, const double *omega, double dt, size_t n_arcs, double *out) {
    if (!v || !omega || !out) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_arc_count(n_arcs)) return rc;
    arcs_host::steps(v, omega, dt, n_arcs, out);
    return KICP_OK;
}
int kicp_footprint_box(double x_min, double x_max, double y_min, double y_max, double spacing, double *out_xy, size_t cap, size_t *out_n) {
    if (!out_n || (!out_xy && cap)) return fail(KICP_ERR_ARG, "null argument");
    *out_n = 0;
    if (!std::isfinite(x_min) || !std::isfinite(x_max) || !std::isfinite(y_min) || !std::isfinite(y_max) || !(x_min <= x_max) || !(y_min <= y_max))
        return fail(KICP_ERR_ARG, "the box must be finite with x_min <= x_max and y_min <= y_max");
    if (!(spacing > 0.0) || !std::isfinite(spacing)) return fail(KICP_ERR_ARG, "spacing must be positive and finite");
    const double nx = arcs_host::box_count(x_min, x_max, spacing), ny = arcs_host::box_count(y_min, y_max, spacing);
    if (!(nx * ny <= static_cast<double>(kArcsMaxP)))
        return fail(KICP_ERR_CAPACITY, "the lattice would have more samples than a footprint may (limit " + std::to_string(kArcsMaxP) + ")");
    *out_n = static_cast<size_t>(nx) * static_cast<size_t>(ny);
    arcs_host::box(x_min, x_max, y_min, y_max, static_cast<size_t>(nx), static_cast<size_t>(ny), out_xy, cap);
    if (*out_n > cap) return fail(KICP_ERR_CAPACITY, "the lattice has " + std::to_string(*out_n) + " samples, cap is " + std::to_string(cap));
    return KICP_OK;
}
int kicp_arcs_best(const unsigned int *results, size_t n_arcs, unsigned int w_potential, unsigned int w_cost, unsigned int w_blocked, unsigned int n_steps,
                   unsigned int min_free_steps, size_t *out_index) {
    if (!results || !out_index) return fail(KICP_ERR_ARG, "null argument");
    *out_index = n_arcs;
    if (int rc = check_arc_count(n_arcs)) return rc;
    *out_index = arcs_host::best(results, n_arcs, w_potential, w_cost, w_blocked, n_steps, min_free_steps);
    return KICP_OK;
}
int kicp_score_arcs_from_plan(const unsigned char *q, const unsigned int *potential, double cell, double origin_x, double origin_y, unsigned int width,
                              unsigned int height, const double start[4], const double *arcs, size_t n_arcs, unsigned int n_steps, const double *footprint_xy,
                              size_t n_samples, unsigned int *out, size_t cap) {
    if (!q || !potential) return fail(KICP_ERR_ARG, "null argument");
    if (!(cell > 0.0) || !std::isfinite(cell) || !std::isfinite(origin_x) || !std::isfinite(origin_y)) return fail(KICP_ERR_ARG, "cell must be positive and finite, the origin finite");
    if (width == 0 || height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    if (static_cast<unsigned long long>(width) * height > kGridMaxCells) return fail(KICP_ERR_CAPACITY, "width * height exceeds 2^28 = " + std::to_string(kGridMaxCells));
    if (int rc = check_arcs_args(start, arcs, n_arcs, n_steps, footprint_xy, n_samples, out, cap)) return rc;
    arcs_host::score(ArcGeom{cell, origin_x, origin_y, width, height}, q, potential, start, arcs, n_arcs, n_steps, footprint_xy, static_cast<uint32_t>(n_samples), out);
    return KICP_OK;
}
int kicp_grid_has_plan(const kicp_grid *grid) { return grid && grid->plan_valid ? 1 : 0; }
int kicp_grid_score_arcs(const kicp_grid *cgrid, const double start[4], const double *arcs, size_t n_arcs, unsigned int n_steps, const double *footprint_xy,
                         size_t n_samples, unsigned int *out, size_t cap) {
    KICP_TRACE_CALL();
    if (!cgrid) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_arcs_args(start, arcs, n_arcs, n_steps, footprint_xy, n_samples, out, cap)) return rc;
    if (!cgrid->plan_valid)
        return fail(KICP_ERR_ARG, "the handle holds no plan: call kicp_grid_potential or kicp_grid_potential_of_costmap first (a call of theirs that failed left none)");
    kicp_grid *grid = const_cast<kicp_grid *>(cgrid);  // logically const: the buffers are scratch, the plan is only read
    if (int rc = set_device(grid->device)) return rc;
    hipStream_t st = grid->stream;
    // the buffers grow while the stream is idle: every entry of the handle drains it
    if (int rc = grid->d_arcs.reserve(4 * n_arcs)) return rc;
    if (int rc = grid->d_footprint.reserve(2 * n_samples)) return rc;
    if (int rc = grid->d_arc_out.reserve(4 * n_arcs)) return rc;
    if (int rc = grid->h_arc_out.reserve(4 * n_arcs, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemcpyAsync(grid->d_arcs.get(), arcs, 4 * n_arcs * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(grid->d_footprint.get(), footprint_xy, 2 * n_samples * sizeof(double), hipMemcpyHostToDevice, st));
    const uint32_t blocks = static_cast<uint32_t>((n_arcs + kArcsPerBlock - 1u) / kArcsPerBlock);
    hipLaunchKernelGGL(k_arcs_score, dim3(blocks), dim3(kArcsBlock), 0, st, grid->d_q.get(), grid->d_pot.get(),
                       ArcGeom{grid->cfg.cell, grid->cfg.origin_x, grid->cfg.origin_y, grid->cfg.width, grid->cfg.height}, ArcPose{start[0], start[1], start[2], start[3]},
                       grid->d_arcs.get(), static_cast<uint32_t>(n_arcs), n_steps, grid->d_footprint.get(), static_cast<uint32_t>(n_samples), grid->d_arc_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(grid->h_arc_out.get(), grid->d_arc_out.get(), 4 * n_arcs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(out, grid->h_arc_out.get(), 4 * n_arcs * sizeof(uint32_t));
    return KICP_OK;
}
int kicp_frontiers_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_frontier_config *cfg, const unsigned int *potential,
                                  unsigned long long *out_rows, size_t cap_rows, size_t *out_n, unsigned int *out_labels, size_t cap_labels) {
    if (out_n) *out_n = 0;
    if (!occupancy || !cfg || !out_n) return fail(KICP_ERR_ARG, "null argument");
    if (width == 0 || height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    if (static_cast<unsigned long long>(width) * height > kGridMaxCells) return fail(KICP_ERR_CAPACITY, "width * height exceeds 2^28 = " + std::to_string(kGridMaxCells));
    FrontParams p;
    if (int rc = check_front_args(cfg, static_cast<size_t>(width) * height, out_rows, cap_rows, out_labels, cap_labels, p)) return rc;
    return front_result(front_host::frontiers(reinterpret_cast<const int8_t *>(occupancy), width, height, p.source_min, cfg->min_size, potential, out_rows, cap_rows, out_labels),
                        cap_rows, out_n);
}
int kicp_grid_frontiers(const kicp_grid *cgrid, const kicp_frontier_config *cfg, int use_plan, unsigned long long *out_rows, size_t cap_rows, size_t *out_n,
                        unsigned int *out_labels, size_t cap_labels) {
    KICP_TRACE_CALL();
    if (out_n) *out_n = 0;
    if (!cgrid || !cfg || !out_n) return fail(KICP_ERR_ARG, "null argument");
    FrontParams p;
    if (int rc = check_front_args(cfg, cgrid->cells, out_rows, cap_rows, out_labels, cap_labels, p)) return rc;
    if (use_plan && !cgrid->plan_valid)
        return fail(KICP_ERR_ARG, "the handle holds no plan: call kicp_grid_potential or kicp_grid_potential_of_costmap first (a call of theirs that failed left none)");
    kicp_grid *grid = const_cast<kicp_grid *>(cgrid);  // logically const: the buffers are scratch, the counters and the plan are only read
    if (int rc = set_device(grid->device)) return rc;
    hipStream_t st = grid->stream;
    const uint32_t width = grid->cfg.width, height = grid->cfg.height, cells = static_cast<uint32_t>(grid->cells);
    const uint32_t tiles_x = (width + kFrontTile - 1u) / kFrontTile, tiles_y = (height + kFrontTile - 1u) / kFrontTile;
    // the buffers grow while the stream is idle: every entry of the handle drains it
    if (int rc = grid->d_front_flags.reserve(cells)) return rc;
    if (int rc = grid->d_front_parent.reserve(cells)) return rc;
    if (int rc = grid->d_front_row_of.reserve(cells)) return rc;
    if (int rc = grid->d_front_ctr.reserve(1)) return rc;
    if (int rc = grid->h_front_ctr.reserve(1, hipHostMallocDefault, false)) return rc;
    const uint32_t cell_blocks = (cells + kFrontBlock - 1u) / kFrontBlock;
    HIP_TRY(hipMemsetAsync(grid->d_front_ctr.get(), 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_front_mark, dim3(cell_blocks), dim3(kFrontBlock), 0, st, grid->d_counts.get(), width, height, cells, p, grid->d_front_flags.get());
    hipLaunchKernelGGL(k_front_local, dim3(tiles_x * tiles_y), dim3(kFrontBlock), 0, st, grid->d_front_flags.get(), width, height, tiles_x, grid->d_front_parent.get());
    const uint32_t row_lanes = (tiles_y - 1u) * width, lanes = row_lanes + (tiles_x - 1u) * height;  // (both below cells / 16)
    if (lanes)
        hipLaunchKernelGGL(k_front_border, dim3((lanes + kFrontBlock - 1u) / kFrontBlock), dim3(kFrontBlock), 0, st, grid->d_front_flags.get(), width, height, row_lanes, lanes,
                           grid->d_front_parent.get());
    hipLaunchKernelGGL(k_front_flatten, dim3(cell_blocks), dim3(kFrontBlock), 0, st, grid->d_front_flags.get(), cells, grid->d_front_parent.get(), grid->d_front_row_of.get(),
                       grid->d_front_ctr.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(grid->h_front_ctr.get(), grid->d_front_ctr.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (out_labels) HIP_TRY(hipMemcpyAsync(out_labels, grid->d_front_parent.get(), static_cast<size_t>(cells) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the number of frontiers sizes the rows
    const uint32_t n_rows = grid->h_front_ctr.get()[0];
    if (n_rows == 0u) return KICP_OK;
    if (int rc = grid->d_front_rows.reserve(static_cast<size_t>(n_rows) * kFrontWords)) return rc;
    grid->h_front_rows.resize(static_cast<size_t>(n_rows) * kFrontWords);
    hipLaunchKernelGGL(k_front_rows, dim3((n_rows + kFrontBlock - 1u) / kFrontBlock), dim3(kFrontBlock), 0, st, grid->d_front_rows.get(), n_rows);
    hipLaunchKernelGGL(k_front_sum, dim3(cell_blocks), dim3(kFrontBlock), 0, st, grid->d_front_flags.get(), grid->d_front_parent.get(), grid->d_front_row_of.get(),
                       use_plan ? grid->d_pot.get() : static_cast<const uint32_t *>(nullptr), width, cells, n_rows, grid->d_front_rows.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(grid->h_front_rows.data(), grid->d_front_rows.get(), grid->h_front_rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return front_result(front_emit(grid->h_front_rows.data(), n_rows, cfg->min_size, out_rows, cap_rows), cap_rows, out_n);
}
int kicp_gain_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_gain_config *cfg, const unsigned int *views, size_t n_views,
                             unsigned int *out, size_t cap_out) {
    if (!occupancy || !cfg) return fail(KICP_ERR_ARG, "null argument");
    if (width == 0 || height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    if (static_cast<unsigned long long>(width) * height > kGridMaxCells) return fail(KICP_ERR_CAPACITY, "width * height exceeds 2^28 = " + std::to_string(kGridMaxCells));
    GainParams p;
    if (int rc = check_gain_args(cfg, static_cast<size_t>(width) * height, views, n_views, out, cap_out, p)) return rc;
    if (n_views) gain_host::gain(reinterpret_cast<const int8_t *>(occupancy), width, height, p.source_min, p.range, views, n_views, out);
    return KICP_OK;
}
int kicp_grid_gain(const kicp_grid *cgrid, const kicp_gain_config *cfg, const unsigned int *views, size_t n_views, unsigned int *out, size_t cap_out) {
    KICP_TRACE_CALL();
    if (!cgrid || !cfg) return fail(KICP_ERR_ARG, "null argument");
    GainParams p;
    if (int rc = check_gain_args(cfg, cgrid->cells, views, n_views, out, cap_out, p)) return rc;
    if (n_views == 0u) return KICP_OK;
    kicp_grid *grid = const_cast<kicp_grid *>(cgrid);  // logically const: the buffers are scratch, the counters and the plan are only read
    if (int rc = set_device(grid->device)) return rc;
    hipStream_t st = grid->stream;
    const uint32_t cells = static_cast<uint32_t>(grid->cells), n = static_cast<uint32_t>(n_views);
    // the buffers grow while the stream is idle: every entry of the handle drains it
    if (int rc = grid->d_gain_classes.reserve(cells)) return rc;
    if (int rc = grid->d_gain_views.reserve(n_views)) return rc;
    if (int rc = grid->d_gain_out.reserve(kGainWords * n_views)) return rc;
    if (int rc = grid->h_gain_out.reserve(kGainWords * n_views, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemcpyAsync(grid->d_gain_views.get(), views, n_views * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gain_classes, dim3((cells + kGainBlock - 1u) / kGainBlock), dim3(kGainBlock), 0, st, grid->d_counts.get(), cells, p.min_observations, p.source_min,
                       grid->d_gain_classes.get());
    hipLaunchKernelGGL(k_gain_rays, dim3(n), dim3(kGainBlock), gain_lds_bytes(p.range), st, grid->d_gain_classes.get(), grid->cfg.width, grid->cfg.height, p.range,
                       grid->d_gain_views.get(), grid->d_gain_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(grid->h_gain_out.get(), grid->d_gain_out.get(), kGainWords * n_views * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(out, grid->h_gain_out.get(), kGainWords * n_views * sizeof(uint32_t));
    return KICP_OK;
}
int kicp_grid_last_window(const kicp_grid *grid, unsigned int *x0, unsigned int *y0, unsigned int *w, unsigned int *h) {
    if (!grid || !x0 || !y0 || !w || !h) return fail(KICP_ERR_ARG, "null argument");
    *x0 = *y0 = *w = *h = 0u;
    if (!grid->has_window) return KICP_OK;
    const int64_t side = 2 * static_cast<int64_t>(grid->geom.reach) + 1;
    const int64_t ax = std::max<int64_t>(grid->win_x0, 0), bx = std::min<int64_t>(grid->win_x0 + side, grid->cfg.width);
    const int64_t ay = std::max<int64_t>(grid->win_y0, 0), by = std::min<int64_t>(grid->win_y0 + side, grid->cfg.height);
    if (ax >= bx || ay >= by) return KICP_OK;
    *x0 = static_cast<unsigned int>(ax), *y0 = static_cast<unsigned int>(ay), *w = static_cast<unsigned int>(bx - ax), *h = static_cast<unsigned int>(by - ay);
    return KICP_OK;
}
int kicp_grid_write_map(const char *prefix, const signed char *occupancy, unsigned int width, unsigned int height, double cell, double origin_x, double origin_y,
                        double occupied_thresh, double free_thresh) {
    if (!prefix || !occupancy) return fail(KICP_ERR_ARG, "null argument");
    if (width == 0 || height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    if (!(cell > 0.0) || !std::isfinite(cell) || !std::isfinite(origin_x) || !std::isfinite(origin_y))
        return fail(KICP_ERR_ARG, "cell must be positive and finite, the origin finite");
    if (int rc = check_thresholds(occupied_thresh, free_thresh)) return rc;
    const std::string pgm = std::string(prefix) + ".pgm", yaml = std::string(prefix) + ".yaml";
    std::FILE *f = std::fopen(pgm.c_str(), "wb");
    if (!f) return fail(KICP_ERR_ARG, "cannot write " + pgm + ": " + std::strerror(errno));
    bool ok = std::fprintf(f, "P5\n%u %u\n255\n", width, height) > 0;
    std::vector<unsigned char> row(width);
    for (unsigned int iy = height; ok && iy-- > 0;) {  // the image's first row is the grid's highest iy
        for (unsigned int ix = 0; ix < width; ++ix) row[ix] = grid_pixel(occupancy[static_cast<size_t>(iy) * width + ix], occupied_thresh, free_thresh);
        ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
    }
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) return fail(KICP_ERR_ARG, "cannot write " + pgm + ": " + std::strerror(errno));
    f = std::fopen(yaml.c_str(), "wb");
    if (!f) return fail(KICP_ERR_ARG, "cannot write " + yaml + ": " + std::strerror(errno));
    const size_t slash = pgm.find_last_of('/');
    ok = std::fprintf(f, "image: %s\nmode: trinary\nresolution: %.17g\norigin: [%.17g, %.17g, 0]\nnegate: 0\noccupied_thresh: %.17g\nfree_thresh: %.17g\n",
                      pgm.c_str() + (slash == std::string::npos ? 0 : slash + 1), cell, origin_x, origin_y, occupied_thresh, free_thresh) > 0;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) return fail(KICP_ERR_ARG, "cannot write " + yaml + ": " + std::strerror(errno));
    return KICP_OK;
}
int kicp_grid_save_map(const kicp_grid *grid, const char *prefix, unsigned int min_observations, double occupied_thresh, double free_thresh) {
    KICP_TRACE_CALL();
    if (!grid || !prefix) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_thresholds(occupied_thresh, free_thresh)) return rc;
    std::vector<signed char> occupancy(grid->cells);
    if (int rc = kicp_grid_occupancy(grid, min_observations, occupancy.data(), grid->cells)) return rc;
    return kicp_grid_write_map(prefix, occupancy.data(), grid->cfg.width, grid->cfg.height, grid->cfg.cell, grid->cfg.origin_x, grid->cfg.origin_y, occupied_thresh,
                               free_thresh);
}

}  // extern "C"
