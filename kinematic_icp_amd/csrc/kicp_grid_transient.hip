// kicp_grid_transient.hip -- what stands in known free space right now (include/kicp.h states the semantics): the returns of one frame
// that end in cells the counters know as free, grouped into transients with ten words each (kicp_grid_transients*; kernels:
// kicp_transient.hpp and the union-find of kicp_front.hpp, arithmetic: kicp_transient_host.hpp; host twin: kicp_transients_from_counts),
// the plane of their cells that the handle keeps, and the switch that makes those cells sources of the clearance, the costmap and the
// potential (read by clear_on_device, kicp_grid_plan.hip).  The handle and the stream rule cited below: kicp_grid_internal.hpp.
#include <cstring>

#include "kicp_front.hpp"
#include "kicp_grid_internal.hpp"
#include "kicp_transient.hpp"

namespace {
// what the three detection entries share: the configuration, and the two outputs with their capacities
int check_transient_args(const kicp_transient_config *cfg, size_t cells, const unsigned long long *out_rows, size_t cap_rows, const unsigned int *out_labels,
                         size_t cap_labels, TransientParams &p) {
    p = TransientParams{cfg->min_observations, cfg->free_max, cfg->min_points, cfg->min_size};
    if (cfg->min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    if (cfg->free_max > 100u) return fail(KICP_ERR_ARG, "free_max must lie in 0 .. 100");
    if (cfg->min_points < 1u) return fail(KICP_ERR_ARG, "min_points must be at least 1");
    if (cfg->min_size < 1u) return fail(KICP_ERR_ARG, "min_size must be at least 1");
    if (!out_rows && cap_rows) return fail(KICP_ERR_ARG, "out_rows may be null only when cap_rows is 0");
    if (cap_labels != 0u && cap_labels != cells) return fail(KICP_ERR_ARG, "cap_labels must be 0 or width * height = " + std::to_string(cells));
    if ((out_labels == nullptr) != (cap_labels == 0u)) return fail(KICP_ERR_ARG, "out_labels must be null exactly when cap_labels is 0");
    return KICP_OK;
}
int transient_result(size_t n, size_t cap_rows, size_t *out_n) {
    *out_n = n;
    if (n > cap_rows) return fail(KICP_ERR_CAPACITY, std::to_string(n) + " transients pass the filter, cap_rows is " + std::to_string(cap_rows));
    return KICP_OK;
}
// the planes of the first call: allocated and zero; the stream is idle (the stream rule)
int transient_prepare(kicp_grid *grid) {
    auto &t = grid->transient;
    if (t.ready) return KICP_OK;
    const size_t cells = grid->cells;
    if (int rc = grid->d_transient_plane.reserve(cells)) return rc;
    if (int rc = t.d_returns.reserve(cells)) return rc;
    if (int rc = t.d_flags.reserve(cells)) return rc;
    if (int rc = t.d_parent.reserve(cells)) return rc;
    if (int rc = t.d_row_of.reserve(cells)) return rc;
    if (int rc = t.d_stats.reserve(5)) return rc;
    if (int rc = t.h_stats.reserve(5, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemsetAsync(grid->d_transient_plane.get(), 0, cells, grid->stream));
    HIP_TRY(hipMemsetAsync(t.d_returns.get(), 0, cells * sizeof(uint32_t), grid->stream));
    HIP_TRY(hipMemsetAsync(t.d_flags.get(), 0, cells, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    t.ready = true;
    return KICP_OK;
}
// the frame at d_xyz (n points; arguments checked): the plane replaced, the rows and the label plane back, the stream drained
int transients_on_device(kicp_grid *grid, const double *d_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], const TransientParams &p,
                         unsigned long long *out_rows, size_t cap_rows, size_t *out_n, unsigned int *out_labels, unsigned long long out_stats[4]) {
    unsigned long long stats[4] = {0, 0, 0, 0};
    if (int rc = transient_prepare(grid)) return rc;
    hipStream_t st = grid->stream;
    auto &t = grid->transient;
    const uint32_t width = grid->cfg.width, height = grid->cfg.height, cells = static_cast<uint32_t>(grid->cells);
    HIP_TRY(hipMemsetAsync(grid->d_transient_plane.get(), 0, cells, st));  // nothing of the previous frame stays
    if (n == 0u) {
        HIP_TRY(hipStreamSynchronize(st));
        if (out_labels) std::memset(out_labels, 0xFF, static_cast<size_t>(cells) * sizeof(unsigned int));
        copy_stats(out_stats, stats);
        return KICP_OK;
    }
    if (int rc = t.d_touched.reserve(n + n / 2)) return rc;  // (the stream rule: idle but for the memset, which does not touch it)
    const GridFrame f = grid_frame(grid->geom, pose_qt, sensor_xyz);
    const uint32_t points = static_cast<uint32_t>(n), point_blocks = (points + kTransientBlock - 1u) / kTransientBlock;
    const uint32_t tiles_x = (width + kFrontTile - 1u) / kFrontTile, tiles_y = (height + kFrontTile - 1u) / kFrontTile;
    const uint32_t cell_blocks = (cells + kFrontBlock - 1u) / kFrontBlock;
    unsigned int *d_stats = t.d_stats.get();
    HIP_TRY(hipMemsetAsync(d_stats, 0, 5 * sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_transient_count, dim3(point_blocks), dim3(kTransientBlock), 0, st, d_xyz, points, grid->geom, f, t.d_returns.get(), t.d_touched.get(), d_stats);
    hipLaunchKernelGGL(k_transient_flag, dim3(point_blocks), dim3(kTransientBlock), 0, st, t.d_touched.get(), d_stats + 2, t.d_returns.get(), grid->d_counts.get(), p,
                       t.d_flags.get(), d_stats);
    hipLaunchKernelGGL(k_front_local, dim3(tiles_x * tiles_y), dim3(kFrontBlock), 0, st, t.d_flags.get(), width, height, tiles_x, t.d_parent.get());
    const uint32_t row_lanes = (tiles_y - 1u) * width, lanes = row_lanes + (tiles_x - 1u) * height;  // (both below cells / 16)
    if (lanes)
        hipLaunchKernelGGL(k_front_border, dim3((lanes + kFrontBlock - 1u) / kFrontBlock), dim3(kFrontBlock), 0, st, t.d_flags.get(), width, height, row_lanes, lanes,
                           t.d_parent.get());
    hipLaunchKernelGGL(k_front_flatten, dim3(cell_blocks), dim3(kFrontBlock), 0, st, t.d_flags.get(), cells, t.d_parent.get(), t.d_row_of.get(), d_stats + 4);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t.h_stats.get(), d_stats, 5 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_labels) HIP_TRY(hipMemcpyAsync(out_labels, t.d_parent.get(), static_cast<size_t>(cells) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the number of transients sizes the rows, the list's length the launches below
    const unsigned int *h = t.h_stats.get();
    const uint32_t n_touched = h[2], n_rows = h[4];
    for (int k = 0; k < 4; ++k) stats[k] = h[k];
    copy_stats(out_stats, stats);
    if (n_touched > points || n_rows > n_touched) return fail(KICP_ERR_INTERNAL, "the transient kernels counted more cells than points");
    if (n_touched == 0u) return KICP_OK;  // nothing to sum, nothing to reset
    const uint32_t touched_blocks = (n_touched + kTransientBlock - 1u) / kTransientBlock;
    if (n_rows) {
        if (int rc = t.d_rows.reserve(static_cast<size_t>(n_rows) * kTransientWords)) return rc;  // (the stream rule: drained just above)
        hipLaunchKernelGGL(k_transient_rows, dim3((n_rows + kTransientBlock - 1u) / kTransientBlock), dim3(kTransientBlock), 0, st, t.d_rows.get(), n_rows);
        hipLaunchKernelGGL(k_transient_sum, dim3(touched_blocks), dim3(kTransientBlock), 0, st, t.d_touched.get(), n_touched, t.d_returns.get(), t.d_flags.get(),
                           t.d_parent.get(), t.d_row_of.get(), width, transient_sensor(f.gx0, grid->geom.reach), transient_sensor(f.gy0, grid->geom.reach), n_rows,
                           t.d_rows.get());
    }
    hipLaunchKernelGGL(k_transient_finish, dim3(touched_blocks), dim3(kTransientBlock), 0, st, t.d_touched.get(), n_touched, t.d_parent.get(), t.d_row_of.get(),
                       t.d_rows.get(), n_rows, p.min_size, t.d_returns.get(), t.d_flags.get(), grid->d_transient_plane.get());
    HIP_TRY(hipGetLastError());
    t.h_rows.resize(static_cast<size_t>(n_rows) * kTransientWords);
    if (n_rows) HIP_TRY(hipMemcpyAsync(t.h_rows.data(), t.d_rows.get(), t.h_rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return transient_result(transient_emit(t.h_rows.data(), n_rows, p.min_size, out_rows, cap_rows), cap_rows, out_n);
}
// the geometry of a pure-host call's grid, checked as kicp_grid_create checks its own
int check_geometry(const kicp_grid_config *cfg, GridGeom &g) {
    if (int rc = check_cell_origin(cfg->cell, cfg->origin_x, cfg->origin_y)) return rc;
    if (!(cfg->max_ray > 0.0) || !std::isfinite(cfg->max_ray)) return fail(KICP_ERR_ARG, "max_ray must be positive and finite");
    if (!(cfg->z_min < cfg->z_max)) return fail(KICP_ERR_ARG, "the band needs z_min < z_max");
    if (int rc = check_grid_dims(cfg->width, cfg->height)) return rc;
    const double reach = std::ceil(cfg->max_ray / cfg->cell);
    if (!(reach <= static_cast<double>(kGridMaxReach)))
        return fail(KICP_ERR_CAPACITY, "max_ray / cell gives a reach of " + std::to_string(reach) + " cells (limit " + std::to_string(kGridMaxReach) + ")");
    g = GridGeom{cfg->cell, cfg->origin_x, cfg->origin_y, cfg->z_min, cfg->z_max, cfg->width, cfg->height, static_cast<int32_t>(reach)};
    return KICP_OK;
}
int check_transient_frame(bool pointers, const double *xyz, size_t n) { return FrameUpload::check(pointers && (xyz || !n), n, "frame too large"); }
}  // namespace

extern "C" {

int kicp_transients_from_counts(const unsigned short *counts, const kicp_grid_config *grid_config, const double *frame_xyz, size_t n, const double pose_qt[7],
                                const double sensor_xyz[3], const kicp_transient_config *cfg, unsigned long long *out_rows, size_t cap_rows, size_t *out_n,
                                unsigned int *out_labels, size_t cap_labels, unsigned long long out_stats[4], unsigned char *out_plane, size_t cap_plane) {
    if (out_n) *out_n = 0;
    if (int rc = check_transient_frame(counts && grid_config && pose_qt && sensor_xyz && cfg && out_n, frame_xyz, n)) return rc;
    GridGeom g;
    if (int rc = check_geometry(grid_config, g)) return rc;
    const size_t cells = static_cast<size_t>(g.width) * g.height;
    TransientParams p;
    if (int rc = check_transient_args(cfg, cells, out_rows, cap_rows, out_labels, cap_labels, p)) return rc;
    if (cap_plane != 0u && cap_plane != cells) return fail(KICP_ERR_ARG, "cap_plane must be 0 or width * height = " + std::to_string(cells));
    if ((out_plane == nullptr) != (cap_plane == 0u)) return fail(KICP_ERR_ARG, "out_plane must be null exactly when cap_plane is 0");
    static_assert(sizeof(unsigned short) == sizeof(uint16_t), "a counter is 16 bits");
    return transient_result(transient_host::transients(g, counts, frame_xyz, n, pose_qt, sensor_xyz, p, out_rows, cap_rows, out_labels, out_plane, out_stats), cap_rows, out_n);
}
int kicp_grid_transients(kicp_grid *grid, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], const kicp_transient_config *cfg,
                         unsigned long long *out_rows, size_t cap_rows, size_t *out_n, unsigned int *out_labels, size_t cap_labels, unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (out_n) *out_n = 0;
    if (int rc = check_transient_frame(grid && pose_qt && sensor_xyz && cfg && out_n, frame_xyz, n)) return rc;
    TransientParams p;
    if (int rc = check_transient_args(cfg, grid->cells, out_rows, cap_rows, out_labels, cap_labels, p)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    if (int rc = grid->frame.upload.put(frame_xyz, n, grid->stream)) return rc;
    return transients_on_device(grid, grid->frame.upload.d_xyz.get(), n, pose_qt, sensor_xyz, p, out_rows, cap_rows, out_n, out_labels, out_stats);
}
int kicp_grid_transients_device(kicp_grid *grid, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], const kicp_transient_config *cfg,
                                unsigned long long *out_rows, size_t cap_rows, size_t *out_n, unsigned int *out_labels, size_t cap_labels,
                                unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (out_n) *out_n = 0;
    if (int rc = check_transient_frame(grid && pose_qt && sensor_xyz && cfg && out_n, d_frame_xyz, n)) return rc;
    TransientParams p;
    if (int rc = check_transient_args(cfg, grid->cells, out_rows, cap_rows, out_labels, cap_labels, p)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    return transients_on_device(grid, d_frame_xyz, n, pose_qt, sensor_xyz, p, out_rows, cap_rows, out_n, out_labels, out_stats);
}
int kicp_grid_transient_plane(const kicp_grid *grid, unsigned char *out, size_t cap_cells) {
    KICP_TRACE_CALL();
    if (!grid || !out) return fail(KICP_ERR_ARG, "null argument");
    if (cap_cells != grid->cells) return fail(KICP_ERR_ARG, "cap_cells must be the grid's " + std::to_string(grid->cells) + " cells");
    if (!grid->d_transient_plane.get()) {  // before the first call: all 0
        std::memset(out, 0, grid->cells);
        return KICP_OK;
    }
    if (int rc = set_device(grid->device)) return rc;
    HIP_TRY(hipMemcpyAsync(out, grid->d_transient_plane.get(), grid->cells, hipMemcpyDeviceToHost, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_use_transients(kicp_grid *grid, int on) {
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    grid->use_transients = on != 0;
    return KICP_OK;
}
int kicp_grid_uses_transients(const kicp_grid *grid) { return grid && grid->use_transients ? 1 : 0; }

}  // extern "C"
