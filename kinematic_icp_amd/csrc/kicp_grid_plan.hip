// kicp_grid_plan.hip -- what a planner plans on, read off the grid's counters (include/kicp.h states the semantics): the clearance of
// every cell and the costmap a table makes of it (kicp_grid_clearance, kicp_grid_costmap; kernels: kicp_clear.hpp, arithmetic:
// kicp_clear_host.hpp), and the cost-to-go field spread over that costmap from the goals (kicp_grid_potential,
// kicp_grid_potential_of_costmap; kernels: kicp_nav.hpp, arithmetic: kicp_nav_host.hpp), with their pure-host twins and helpers.  A
// successful potential call leaves the PLAN in the handle (kicp_grid_internal.hpp, which also has the stream rule cited below).
#include "kicp_clear.hpp"
#include "kicp_grid_internal.hpp"
#include "kicp_nav.hpp"

namespace {
// the configuration of a clearance call as the kernels take it
int check_clear_config(const kicp_grid_clearance_config *cfg, ClearParams &p) {
    p = ClearParams{cfg->min_observations, 0, cfg->unknown_is_obstacle ? 1u : 0u, static_cast<uint32_t>(cfg->radius_cells)};
    if (int rc = check_cell_classes(cfg->min_observations, cfg->occupied_thresh, p.source_min)) return rc;
    if (cfg->radius_cells < 1) return fail(KICP_ERR_ARG, "radius_cells must be at least 1");
    if (cfg->radius_cells > kClearMaxRadius)
        return fail(KICP_ERR_CAPACITY, "radius_cells = " + std::to_string(cfg->radius_cells) + " (limit " + std::to_string(kClearMaxRadius) + ")");
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
// Two launches, one copy, the stream drained.  out == nullptr: the costmap stays in d_cost for the launches the caller queues behind
// these; nothing is copied or waited for (the stream rule's exception).  With the handle's switch on (kicp_grid_use_transients) and a
// transient plane to read, the kPlane instantiations run: the plane's cells are sources.  The clearance's rows take no class, so they
// have no such instantiation.
int clear_on_device(const kicp_grid *grid, const ClearParams &p, const ClearRect &r, const unsigned char *table, uint32_t inflate_unknown, void *out) {
    if (int rc = set_device(grid->device)) return rc;
    const size_t cells = static_cast<size_t>(r.w) * r.h;
    uint32_t cx0, cx1;
    clear_host::column_range(grid->cfg.width, r, p.radius, cx0, cx1);
    const uint32_t cw = cx1 - cx0;
    hipStream_t st = grid->stream;
    auto &c = grid->clear;
    if (int rc = c.d_coldist.reserve(static_cast<size_t>(cw) * r.h)) return rc;
    if (table) {
        if (int rc = c.d_cost.reserve(cells)) return rc;
        if (int rc = c.d_cost_table.reserve(static_cast<size_t>(clear_far(kClearMaxRadius)) + 1u)) return rc;
        HIP_TRY(hipMemcpyAsync(c.d_cost_table.get(), table, static_cast<size_t>(clear_far(p.radius)) + 1u, hipMemcpyHostToDevice, st));
    } else if (int rc = c.d_clearance.reserve(cells)) {
        return rc;
    }
    // a strip of at least R rows keeps the rows a workgroup reads beside its own at or below twice its own
    const uint32_t strip = std::max(32u, p.radius), strips = (r.h + strip - 1u) / strip, col_blocks = (cw + kClearBlock - 1u) / kClearBlock;
    const uint32_t segments = (r.w + kClearSegment - 1u) / kClearSegment;  // (both products stay below 2^29: cells <= 2^28)
    const uint8_t *plane = grid->use_transients ? grid->d_transient_plane.get() : nullptr;  // (no plane yet: all 0)
    const auto columns = plane ? &k_clear_columns<true> : &k_clear_columns<false>;
    const auto cost_rows = plane ? &k_clear_rows<true, true> : &k_clear_rows<true, false>;
    const auto clearance_rows = &k_clear_rows<false, false>;
    hipLaunchKernelGGL(columns, dim3(strips * col_blocks), dim3(kClearBlock), 0, st, grid->d_counts.get(), grid->cfg.width, grid->cfg.height, p, r, cx0, cw, strip,
                       col_blocks, c.d_coldist.get(), plane);
    if (table)
        hipLaunchKernelGGL(cost_rows, dim3(r.h * segments), dim3(kClearBlock), 0, st, c.d_coldist.get(), cx0, cw, grid->d_counts.get(), grid->cfg.width, p, r, segments,
                           c.d_cost_table.get(), inflate_unknown, static_cast<void *>(c.d_cost.get()), plane);
    else
        hipLaunchKernelGGL(clearance_rows, dim3(r.h * segments), dim3(kClearBlock), 0, st, c.d_coldist.get(), cx0, cw, grid->d_counts.get(), grid->cfg.width, p, r, segments,
                           static_cast<const uint8_t *>(nullptr), 0u, static_cast<void *>(c.d_clearance.get()), static_cast<const uint8_t *>(nullptr));
    HIP_TRY(hipGetLastError());
    if (!out) return KICP_OK;
    if (table)
        HIP_TRY(hipMemcpyAsync(out, c.d_cost.get(), cells, hipMemcpyDeviceToHost, st));
    else
        HIP_TRY(hipMemcpyAsync(out, c.d_clearance.get(), cells * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
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
int potential_on_device(const kicp_grid *grid, const uint8_t *d_costmap, const unsigned char *weight, uint32_t max_potential, const unsigned int *goals, size_t n_goals,
                        unsigned int *out, unsigned long long out_stats[4]) {
    const uint32_t width = grid->cfg.width, height = grid->cfg.height, cells = static_cast<uint32_t>(grid->cells);
    const uint32_t tiles_x = (width + kNavTile - 1u) / kNavTile, tiles_y = (height + kNavTile - 1u) / kNavTile, tiles = tiles_x * tiles_y;
    hipStream_t st = grid->stream;
    auto &pl = grid->plan;
    pl.valid = false;  // until this call has succeeded
    if (int rc = pl.d_pot.reserve(cells)) return rc;
    if (int rc = pl.d_q.reserve(cells)) return rc;
    if (int rc = pl.d_flags.reserve(2 * static_cast<size_t>(tiles))) return rc;
    if (int rc = pl.d_weight.reserve(256)) return rc;
    if (int rc = pl.d_goals.reserve(2 * n_goals)) return rc;
    if (int rc = pl.d_ctr.reserve(kNavBatch + 2u)) return rc;
    if (int rc = pl.h_ctr.reserve(kNavBatch + 2u, hipHostMallocDefault, false)) return rc;
    uint8_t *flags = pl.d_flags.get();
    uint32_t *ctr = pl.d_ctr.get(), *h = pl.h_ctr.get();
    HIP_TRY(hipMemcpyAsync(pl.d_weight.get(), weight, 256, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(pl.d_goals.get(), goals, 2 * n_goals * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(flags, 0, 2 * static_cast<size_t>(tiles), st));
    HIP_TRY(hipMemsetAsync(ctr, 0, (kNavBatch + 2u) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_nav_init, dim3((cells + kNavBlock - 1u) / kNavBlock), dim3(kNavBlock), 0, st, d_costmap, pl.d_weight.get(), cells, pl.d_q.get(), pl.d_pot.get());
    hipLaunchKernelGGL(k_nav_goals, dim3(static_cast<uint32_t>((n_goals + kNavBlock - 1u) / kNavBlock)), dim3(kNavBlock), 0, st, pl.d_goals.get(),
                       static_cast<uint32_t>(n_goals), width, tiles_x, pl.d_q.get(), pl.d_pot.get(), flags);
    // A round holds a full sweep of every active tile, so the rounds end within the number of cells; never loop without that limit.
    const unsigned long long limit = static_cast<unsigned long long>(cells) + 1ull;
    unsigned long long rounds = 0;
    for (bool done = false; !done;) {
        if (rounds >= limit) return fail(KICP_ERR_INTERNAL, "the potential did not settle within " + std::to_string(limit) + " rounds");
        const uint32_t batch = static_cast<uint32_t>(std::min<unsigned long long>(kNavBatch, limit - rounds));
        for (uint32_t i = 0; i < batch; ++i) {
            const uint32_t parity = static_cast<uint32_t>((rounds + i) & 1ull);
            hipLaunchKernelGGL(k_nav_relax, dim3(tiles), dim3(kNavBlock), 0, st, pl.d_pot.get(), pl.d_q.get(), width, height, tiles_x, tiles_y, max_potential,
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
    hipLaunchKernelGGL(k_nav_count, dim3(std::min((cells + kNavBlock - 1u) / kNavBlock, 1024u)), dim3(kNavBlock), 0, st, pl.d_pot.get(), cells, max_potential,
                       ctr + kNavBatch);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, pl.d_pot.get(), static_cast<size_t>(cells) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h + kNavBatch, ctr + kNavBatch, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (out_stats) {
        out_stats[0] = 0ull, out_stats[1] = h[kNavBatch], out_stats[2] = h[kNavBatch + 1u], out_stats[3] = rounds;
        for (size_t g = 0; g < n_goals; ++g) out_stats[0] += out[static_cast<size_t>(goals[2 * g + 1]) * width + goals[2 * g]] == 0u ? 1ull : 0ull;  // 0 only on a passable goal
    }
    pl.valid = true;
    return KICP_OK;
}
}  // namespace

extern "C" {

int kicp_grid_clearance(const kicp_grid *grid, const kicp_grid_clearance_config *cfg, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, unsigned short *out,
                        size_t cap) {
    KICP_TRACE_CALL();
    if (!grid || !cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    ClearParams p;
    const ClearRect r{x0, y0, w, h};
    if (int rc = check_clear_config(cfg, p)) return rc;
    if (int rc = check_clear_rect(grid->cfg.width, grid->cfg.height, r, cap)) return rc;
    return clear_on_device(grid, p, r, nullptr, 0u, out);
}
int kicp_grid_costmap(const kicp_grid *grid, const kicp_grid_clearance_config *cfg, const unsigned char *table, size_t table_len, int inflate_unknown, unsigned int x0,
                      unsigned int y0, unsigned int w, unsigned int h, unsigned char *out, size_t cap) {
    KICP_TRACE_CALL();
    if (!grid || !cfg || !table || !out) return fail(KICP_ERR_ARG, "null argument");
    ClearParams p;
    const ClearRect r{x0, y0, w, h};
    if (int rc = check_clear_config(cfg, p)) return rc;
    if (int rc = check_cost_table(p, table_len)) return rc;
    if (int rc = check_clear_rect(grid->cfg.width, grid->cfg.height, r, cap)) return rc;
    return clear_on_device(grid, p, r, table, inflate_unknown ? 1u : 0u, out);
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
    if (int rc = check_grid_dims(width, height)) return rc;
    if (int rc = check_plan_args(cfg, width, height, goals_xy, n_goals, cap)) return rc;
    unsigned long long stats[4];
    nav_host::potential(costmap, width, height, weight, cfg->max_potential, goals_xy, n_goals, out, stats);
    copy_stats(out_stats, stats);
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
int kicp_grid_potential_of_costmap(const kicp_grid *grid, const unsigned char *costmap, const unsigned char weight[256], const kicp_plan_config *cfg,
                                   const unsigned int *goals_xy, size_t n_goals, unsigned int *out, size_t cap, unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (grid) grid->plan.valid = false;  // a call that fails, on its arguments too, leaves no plan
    if (!grid || !costmap || !weight || !cfg || !goals_xy || !out) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_plan_args(cfg, grid->cfg.width, grid->cfg.height, goals_xy, n_goals, cap)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    if (int rc = grid->clear.d_cost.reserve(grid->cells)) return rc;
    HIP_TRY(hipMemcpyAsync(grid->clear.d_cost.get(), costmap, grid->cells, hipMemcpyHostToDevice, grid->stream));
    return potential_on_device(grid, grid->clear.d_cost.get(), weight, cfg->max_potential, goals_xy, n_goals, out, out_stats);
}
int kicp_grid_potential(const kicp_grid *grid, const kicp_grid_clearance_config *clearance, const unsigned char *table, size_t table_len, int inflate_unknown,
                        const unsigned char weight[256], const kicp_plan_config *cfg, const unsigned int *goals_xy, size_t n_goals, unsigned int *out, size_t cap,
                        unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (grid) grid->plan.valid = false;  // as above
    if (!grid || !clearance || !table || !weight || !cfg || !goals_xy || !out) return fail(KICP_ERR_ARG, "null argument");
    ClearParams p;
    const ClearRect r{0u, 0u, grid->cfg.width, grid->cfg.height};
    if (int rc = check_clear_config(clearance, p)) return rc;
    if (int rc = check_cost_table(p, table_len)) return rc;
    if (int rc = check_plan_args(cfg, r.w, r.h, goals_xy, n_goals, cap)) return rc;
    if (int rc = clear_on_device(grid, p, r, table, inflate_unknown ? 1u : 0u, nullptr)) return rc;  // the costmap stays in d_cost
    return potential_on_device(grid, grid->clear.d_cost.get(), weight, cfg->max_potential, goals_xy, n_goals, out, out_stats);
}
int kicp_plan_q(const unsigned char *costmap, size_t cells, const unsigned char weight[256], unsigned char *out) {
    if (!weight || ((!costmap || !out) && cells)) return fail(KICP_ERR_ARG, "null argument");
    for (size_t c = 0; c < cells; ++c) out[c] = weight[costmap[c]];
    return KICP_OK;
}
int kicp_grid_has_plan(const kicp_grid *grid) { return grid && grid->plan.valid ? 1 : 0; }

}  // extern "C"
