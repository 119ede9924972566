// kicp_grid_arcs.hip -- from the field to a command: a fan of arc trajectories scored on the handle's plan (kicp_grid_score_arcs;
// include/kicp.h states the semantics; kernel: kicp_arcs.hpp, arithmetic: kicp_arcs_host.hpp), its host twin
// kicp_score_arcs_from_plan and the helpers kicp_arc_steps, kicp_footprint_box and kicp_arcs_best.  The handle and its plan:
// kicp_grid_internal.hpp.
#include "kicp_arcs.hpp"
#include "kicp_grid_internal.hpp"

namespace {
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
}  // namespace

extern "C" {

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
    if (int rc = check_cell_origin(cell, origin_x, origin_y)) return rc;
    if (int rc = check_grid_dims(width, height)) return rc;
    if (int rc = check_arcs_args(start, arcs, n_arcs, n_steps, footprint_xy, n_samples, out, cap)) return rc;
    arcs_host::score(ArcGeom{cell, origin_x, origin_y, width, height}, q, potential, start, arcs, n_arcs, n_steps, footprint_xy, static_cast<uint32_t>(n_samples), out);
    return KICP_OK;
}
int kicp_grid_score_arcs(const kicp_grid *grid, const double start[4], const double *arcs, size_t n_arcs, unsigned int n_steps, const double *footprint_xy,
                         size_t n_samples, unsigned int *out, size_t cap) {
    KICP_TRACE_CALL();
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_arcs_args(start, arcs, n_arcs, n_steps, footprint_xy, n_samples, out, cap)) return rc;
    if (int rc = check_has_plan(grid)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    hipStream_t st = grid->stream;
    auto &a = grid->arcs;
    if (int rc = a.d_arcs.reserve(4 * n_arcs)) return rc;  // (the stream rule)
    if (int rc = a.d_footprint.reserve(2 * n_samples)) return rc;
    if (int rc = a.d_out.reserve(4 * n_arcs)) return rc;
    if (int rc = a.h_out.reserve(4 * n_arcs, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemcpyAsync(a.d_arcs.get(), arcs, 4 * n_arcs * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a.d_footprint.get(), footprint_xy, 2 * n_samples * sizeof(double), hipMemcpyHostToDevice, st));
    const uint32_t blocks = static_cast<uint32_t>((n_arcs + kArcsPerBlock - 1u) / kArcsPerBlock);
    hipLaunchKernelGGL(k_arcs_score, dim3(blocks), dim3(kArcsBlock), 0, st, grid->plan.d_q.get(), grid->plan.d_pot.get(),
                       ArcGeom{grid->cfg.cell, grid->cfg.origin_x, grid->cfg.origin_y, grid->cfg.width, grid->cfg.height}, ArcPose{start[0], start[1], start[2], start[3]},
                       a.d_arcs.get(), static_cast<uint32_t>(n_arcs), n_steps, a.d_footprint.get(), static_cast<uint32_t>(n_samples), a.d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a.h_out.get(), a.d_out.get(), 4 * n_arcs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(out, a.h_out.get(), 4 * n_arcs * sizeof(uint32_t));
    return KICP_OK;
}

}  // extern "C"
