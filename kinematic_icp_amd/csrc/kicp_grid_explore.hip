// kicp_grid_explore.hip -- where to go while mapping (include/kicp.h states the semantics): the exploration frontiers of the counters -
// the free cells that border unknown space, grouped and ranked by the handle's plan (kicp_grid_frontiers; kernels: kicp_front.hpp,
// arithmetic: kicp_front_host.hpp; host twin: kicp_frontiers_from_occupancy) - and what a sensor would see of the unknown cells from
// candidate viewpoints such as those frontiers' best cells (kicp_grid_gain; kernels: kicp_gain.hpp, arithmetic: kicp_gain_host.hpp;
// host twin: kicp_gain_from_occupancy).  The handle, its plan and the stream rule cited below: kicp_grid_internal.hpp.
#include "kicp_front.hpp"
#include "kicp_gain.hpp"
#include "kicp_grid_internal.hpp"

namespace {
// what the two frontier entries share: the configuration, and the two outputs with their capacities
int check_front_args(const kicp_frontier_config *cfg, size_t cells, const unsigned long long *out_rows, size_t cap_rows, const unsigned int *out_labels, size_t cap_labels,
                     FrontParams &p) {
    p.min_observations = cfg->min_observations;
    if (int rc = check_cell_classes(cfg->min_observations, cfg->occupied_thresh, p.source_min)) return rc;
    if (cfg->min_size < 1u) return fail(KICP_ERR_ARG, "min_size must be at least 1");
    if (!out_rows && cap_rows) return fail(KICP_ERR_ARG, "out_rows may be null only when cap_rows is 0");
    if (cap_labels != 0u && cap_labels != cells) return fail(KICP_ERR_ARG, "cap_labels must be 0 or width * height = " + std::to_string(cells));
    if ((out_labels == nullptr) != (cap_labels == 0u)) return fail(KICP_ERR_ARG, "out_labels must be null exactly when cap_labels is 0");
    return KICP_OK;
}
int front_result(size_t n, size_t cap_rows, size_t *out_n) {
    *out_n = n;
    if (n > cap_rows) return fail(KICP_ERR_CAPACITY, std::to_string(n) + " frontiers pass the filter, cap_rows is " + std::to_string(cap_rows));
    return KICP_OK;
}
// what the two gain entries share: the configuration, the viewpoints - each a cell index below `cells` - and the output
int check_gain_args(const kicp_gain_config *cfg, size_t cells, const unsigned int *views, size_t n_views, const unsigned int *out, size_t cap_out, GainParams &p) {
    p.min_observations = cfg->min_observations, p.range = cfg->range_cells;
    if (int rc = check_cell_classes(cfg->min_observations, cfg->occupied_thresh, p.source_min)) return rc;
    if (cfg->range_cells < 1u || cfg->range_cells > kGainMaxRange) return fail(KICP_ERR_ARG, "range_cells must lie in 1 .. " + std::to_string(kGainMaxRange));
    if (n_views > kGainMaxViews) return fail(KICP_ERR_CAPACITY, "n_views = " + std::to_string(n_views) + " (limit 2^24 = " + std::to_string(kGainMaxViews) + ")");
    if (n_views && (!views || !out)) return fail(KICP_ERR_ARG, "views and out may be null only when n_views is 0");
    if (cap_out != kGainWords * n_views) return fail(KICP_ERR_ARG, "cap_out must be 4 * n_views = " + std::to_string(kGainWords * n_views));
    for (size_t i = 0; i < n_views; ++i)
        if (views[i] >= cells)
            return fail(KICP_ERR_ARG, "viewpoint " + std::to_string(i) + " is cell " + std::to_string(views[i]) + ", outside the grid's " + std::to_string(cells) + " cells");
    return KICP_OK;
}
}  // namespace

extern "C" {

int kicp_frontiers_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_frontier_config *cfg, const unsigned int *potential,
                                  unsigned long long *out_rows, size_t cap_rows, size_t *out_n, unsigned int *out_labels, size_t cap_labels) {
    if (out_n) *out_n = 0;
    if (!occupancy || !cfg || !out_n) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_grid_dims(width, height)) return rc;
    FrontParams p;
    if (int rc = check_front_args(cfg, static_cast<size_t>(width) * height, out_rows, cap_rows, out_labels, cap_labels, p)) return rc;
    return front_result(front_host::frontiers(reinterpret_cast<const int8_t *>(occupancy), width, height, p.source_min, cfg->min_size, potential, out_rows, cap_rows, out_labels),
                        cap_rows, out_n);
}
int kicp_grid_frontiers(const kicp_grid *grid, const kicp_frontier_config *cfg, int use_plan, unsigned long long *out_rows, size_t cap_rows, size_t *out_n,
                        unsigned int *out_labels, size_t cap_labels) {
    KICP_TRACE_CALL();
    if (out_n) *out_n = 0;
    if (!grid || !cfg || !out_n) return fail(KICP_ERR_ARG, "null argument");
    FrontParams p;
    if (int rc = check_front_args(cfg, grid->cells, out_rows, cap_rows, out_labels, cap_labels, p)) return rc;
    if (int rc = use_plan ? check_has_plan(grid) : KICP_OK) return rc;
    if (int rc = set_device(grid->device)) return rc;
    hipStream_t st = grid->stream;
    auto &f = grid->front;
    const uint32_t width = grid->cfg.width, height = grid->cfg.height, cells = static_cast<uint32_t>(grid->cells);
    const uint32_t tiles_x = (width + kFrontTile - 1u) / kFrontTile, tiles_y = (height + kFrontTile - 1u) / kFrontTile;
    if (int rc = f.d_flags.reserve(cells)) return rc;  // (the stream rule)
    if (int rc = f.d_parent.reserve(cells)) return rc;
    if (int rc = f.d_row_of.reserve(cells)) return rc;
    if (int rc = f.d_ctr.reserve(1)) return rc;
    if (int rc = f.h_ctr.reserve(1, hipHostMallocDefault, false)) return rc;
    const uint32_t cell_blocks = (cells + kFrontBlock - 1u) / kFrontBlock;
    HIP_TRY(hipMemsetAsync(f.d_ctr.get(), 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_front_mark, dim3(cell_blocks), dim3(kFrontBlock), 0, st, grid->d_counts.get(), width, height, cells, p, f.d_flags.get());
    hipLaunchKernelGGL(k_front_local, dim3(tiles_x * tiles_y), dim3(kFrontBlock), 0, st, f.d_flags.get(), width, height, tiles_x, f.d_parent.get());
    const uint32_t row_lanes = (tiles_y - 1u) * width, lanes = row_lanes + (tiles_x - 1u) * height;  // (both below cells / 16)
    if (lanes)
        hipLaunchKernelGGL(k_front_border, dim3((lanes + kFrontBlock - 1u) / kFrontBlock), dim3(kFrontBlock), 0, st, f.d_flags.get(), width, height, row_lanes, lanes,
                           f.d_parent.get());
    hipLaunchKernelGGL(k_front_flatten, dim3(cell_blocks), dim3(kFrontBlock), 0, st, f.d_flags.get(), cells, f.d_parent.get(), f.d_row_of.get(), f.d_ctr.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(f.h_ctr.get(), f.d_ctr.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (out_labels) HIP_TRY(hipMemcpyAsync(out_labels, f.d_parent.get(), static_cast<size_t>(cells) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the number of frontiers sizes the rows
    const uint32_t n_rows = f.h_ctr.get()[0];
    if (n_rows == 0u) return KICP_OK;
    if (int rc = f.d_rows.reserve(static_cast<size_t>(n_rows) * kFrontWords)) return rc;
    f.h_rows.resize(static_cast<size_t>(n_rows) * kFrontWords);
    hipLaunchKernelGGL(k_front_rows, dim3((n_rows + kFrontBlock - 1u) / kFrontBlock), dim3(kFrontBlock), 0, st, f.d_rows.get(), n_rows);
    hipLaunchKernelGGL(k_front_sum, dim3(cell_blocks), dim3(kFrontBlock), 0, st, f.d_flags.get(), f.d_parent.get(), f.d_row_of.get(),
                       use_plan ? grid->plan.d_pot.get() : static_cast<const uint32_t *>(nullptr), width, cells, n_rows, f.d_rows.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(f.h_rows.data(), f.d_rows.get(), f.h_rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return front_result(front_emit(f.h_rows.data(), n_rows, cfg->min_size, out_rows, cap_rows), cap_rows, out_n);
}
int kicp_gain_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_gain_config *cfg, const unsigned int *views, size_t n_views,
                             unsigned int *out, size_t cap_out) {
    if (!occupancy || !cfg) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_grid_dims(width, height)) return rc;
    GainParams p;
    if (int rc = check_gain_args(cfg, static_cast<size_t>(width) * height, views, n_views, out, cap_out, p)) return rc;
    if (n_views) gain_host::gain(reinterpret_cast<const int8_t *>(occupancy), width, height, p.source_min, p.range, views, n_views, out);
    return KICP_OK;
}
int kicp_grid_gain(const kicp_grid *grid, const kicp_gain_config *cfg, const unsigned int *views, size_t n_views, unsigned int *out, size_t cap_out) {
    KICP_TRACE_CALL();
    if (!grid || !cfg) return fail(KICP_ERR_ARG, "null argument");
    GainParams p;
    if (int rc = check_gain_args(cfg, grid->cells, views, n_views, out, cap_out, p)) return rc;
    if (n_views == 0u) return KICP_OK;
    if (int rc = set_device(grid->device)) return rc;
    hipStream_t st = grid->stream;
    auto &g = grid->gain;
    const uint32_t cells = static_cast<uint32_t>(grid->cells), n = static_cast<uint32_t>(n_views);
    if (int rc = g.d_classes.reserve(cells)) return rc;  // (the stream rule)
    if (int rc = g.d_views.reserve(n_views)) return rc;
    if (int rc = g.d_out.reserve(kGainWords * n_views)) return rc;
    if (int rc = g.h_out.reserve(kGainWords * n_views, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemcpyAsync(g.d_views.get(), views, n_views * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gain_classes, dim3((cells + kGainBlock - 1u) / kGainBlock), dim3(kGainBlock), 0, st, grid->d_counts.get(), cells, p.min_observations, p.source_min,
                       g.d_classes.get());
    hipLaunchKernelGGL(k_gain_rays, dim3(n), dim3(kGainBlock), gain_lds_bytes(p.range), st, g.d_classes.get(), grid->cfg.width, grid->cfg.height, p.range, g.d_views.get(),
                       g.d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(g.h_out.get(), g.d_out.get(), kGainWords * n_views * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(out, g.h_out.get(), kGainWords * n_views * sizeof(uint32_t));
    return KICP_OK;
}

}  // extern "C"
