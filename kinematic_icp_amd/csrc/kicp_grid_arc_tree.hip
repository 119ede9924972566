// kicp_grid_arc_tree.hip -- commands that change along a trajectory: a tree of arc segments scored on the handle's plan
// (kicp_grid_score_arc_tree; include/kicp.h states the semantics; kernel: kicp_arc_tree.hpp, arithmetic: kicp_arc_tree_host.hpp), its
// host twin kicp_score_arc_tree_from_plan and the helpers kicp_arc_tree_nodes and kicp_arc_tree_best.  The handle and its plan:
// kicp_grid_internal.hpp.
#include "kicp_arc_tree.hpp"
#include "kicp_grid_internal.hpp"

namespace {
// what every entry that takes a tree shares: the shape, or the rule it breaks
int check_tree(unsigned int depth, const unsigned int *branch, const unsigned int *steps, ArcTreeShape &shape) {
    if (!branch || !steps) return fail(KICP_ERR_ARG, "null argument");
    switch (arc_tree_host::nodes(depth, branch, steps, shape)) {
    case arc_tree_host::kShapeZero: return fail(KICP_ERR_ARG, "depth and every entry of branch and steps must be at least 1");
    case arc_tree_host::kShapeDepth: return fail(KICP_ERR_CAPACITY, "depth = " + std::to_string(depth) + " (limit " + std::to_string(kArcTreeMaxDepth) + ")");
    case arc_tree_host::kShapeNodes:
        return fail(KICP_ERR_CAPACITY, "the tree has more nodes than a call may score (limit 2^20 = " + std::to_string(kArcTreeMaxNodes) + ")");
    case arc_tree_host::kShapeSteps: return fail(KICP_ERR_CAPACITY, "the steps along a path exceed the limit " + std::to_string(kArcTreeMaxT));
    case arc_tree_host::kShapeOk: break;
    }
    return KICP_OK;
}
// what the two scoring entries share
int check_tree_args(const double *start, unsigned int depth, const unsigned int *branch, const unsigned int *steps, const double *primitives, const double *footprint_xy,
                    size_t n_samples, const unsigned int *out, size_t cap, ArcTreeShape &shape) {
    if (!start || !primitives || !footprint_xy || !out) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_tree(depth, branch, steps, shape)) return rc;
    if (n_samples < 1u) return fail(KICP_ERR_ARG, "at least one footprint sample is needed");
    if (n_samples > kArcsMaxP) return fail(KICP_ERR_CAPACITY, "n_samples = " + std::to_string(n_samples) + " (limit " + std::to_string(kArcsMaxP) + ")");
    if (cap != 4 * shape.n_nodes) return fail(KICP_ERR_ARG, "cap must be 4 * n_nodes = " + std::to_string(4 * shape.n_nodes));
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(start[i])) return fail(KICP_ERR_ARG, "the start (x, y, cosine, sine) must be finite");
    return KICP_OK;
}
// the records of one level above the leaves: the levels alternate between the two halves of a buffer of twice as many
size_t record_half(const ArcTreeShape &shape) { return shape.depth > 1u ? shape.count[shape.depth - 2u] : 0u; }
}  // namespace

extern "C" {

int kicp_arc_tree_nodes(unsigned int depth, const unsigned int *branch, const unsigned int *steps, size_t *out_n_nodes, size_t *out_n_leaves, unsigned int *out_total_steps,
                        size_t *out_level_offset) {
    if (!out_n_nodes || !out_n_leaves || !out_total_steps) return fail(KICP_ERR_ARG, "null argument");
    *out_n_nodes = *out_n_leaves = 0, *out_total_steps = 0u;
    ArcTreeShape shape;
    if (int rc = check_tree(depth, branch, steps, shape)) return rc;
    *out_n_nodes = shape.n_nodes, *out_n_leaves = shape.n_leaves, *out_total_steps = shape.total_steps;
    if (out_level_offset)
        for (uint32_t e = 0; e < shape.depth; ++e) out_level_offset[e] = shape.offset[e];
    return KICP_OK;
}
int kicp_arc_tree_best(const unsigned int *results, unsigned int depth, const unsigned int *branch, const unsigned int *steps, unsigned int w_potential, unsigned int w_cost,
                       unsigned int w_blocked, unsigned int min_free_steps, size_t *out_leaf, unsigned int *out_path) {
    if (!results || !out_leaf || !out_path) return fail(KICP_ERR_ARG, "null argument");
    *out_leaf = 0;
    ArcTreeShape shape;
    if (int rc = check_tree(depth, branch, steps, shape)) return rc;
    *out_leaf = arc_tree_host::best(results, shape, branch, w_potential, w_cost, w_blocked, min_free_steps, out_path);
    return KICP_OK;
}
int kicp_score_arc_tree_from_plan(const unsigned char *q, const unsigned int *potential, double cell, double origin_x, double origin_y, unsigned int width,
                                  unsigned int height, const double start[4], unsigned int depth, const unsigned int *branch, const unsigned int *steps,
                                  const double *primitives, const double *footprint_xy, size_t n_samples, unsigned int *out, size_t cap) {
    if (!q || !potential) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_cell_origin(cell, origin_x, origin_y)) return rc;
    if (int rc = check_grid_dims(width, height)) return rc;
    ArcTreeShape shape;
    if (int rc = check_tree_args(start, depth, branch, steps, primitives, footprint_xy, n_samples, out, cap, shape)) return rc;
    std::vector<ArcTreeNode> records(2 * record_half(shape));
    arc_tree_host::score(ArcGeom{cell, origin_x, origin_y, width, height}, q, potential, start, shape, branch, steps, primitives, footprint_xy,
                         static_cast<uint32_t>(n_samples), records.data(), records.data() + record_half(shape), out);
    return KICP_OK;
}
int kicp_grid_score_arc_tree(const kicp_grid *grid, const double start[4], unsigned int depth, const unsigned int *branch, const unsigned int *steps,
                             const double *primitives, const double *footprint_xy, size_t n_samples, unsigned int *out, size_t cap) {
    KICP_TRACE_CALL();
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    ArcTreeShape shape;
    if (int rc = check_tree_args(start, depth, branch, steps, primitives, footprint_xy, n_samples, out, cap, shape)) return rc;
    if (int rc = check_has_plan(grid)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    hipStream_t st = grid->stream;
    auto &a = grid->arc_tree;
    const size_t half = record_half(shape), words = 4 * shape.n_nodes;
    if (int rc = a.d_primitives.reserve(4 * shape.n_primitives)) return rc;  // (the stream rule)
    if (int rc = a.d_footprint.reserve(2 * n_samples)) return rc;
    if (int rc = a.d_records.reserve(2 * half)) return rc;
    if (int rc = a.d_out.reserve(words)) return rc;
    if (int rc = a.h_out.reserve(words, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemcpyAsync(a.d_primitives.get(), primitives, 4 * shape.n_primitives * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a.d_footprint.get(), footprint_xy, 2 * n_samples * sizeof(double), hipMemcpyHostToDevice, st));
    const ArcGeom geom{grid->cfg.cell, grid->cfg.origin_x, grid->cfg.origin_y, grid->cfg.width, grid->cfg.height};
    const ArcTreeNode root = arc_tree_root(start);
    // level e + 1 writes the half e % 2 of the records and reads the other one, which the level above wrote
    for (uint32_t e = 0; e < shape.depth; ++e) {
        const ArcTreeNode *parents = e == 0u ? nullptr : a.d_records.get() + ((e - 1u) % 2u) * half;
        const uint32_t *parent_rows = e == 0u ? nullptr : a.d_out.get() + 4 * shape.offset[e - 1u];
        ArcTreeNode *children = e + 1u == shape.depth ? nullptr : a.d_records.get() + (e % 2u) * half;
        const uint32_t blocks = static_cast<uint32_t>((shape.count[e] + kArcTreePerBlock - 1u) / kArcTreePerBlock);
        hipLaunchKernelGGL(k_arc_tree_level, dim3(blocks), dim3(kArcTreeBlock), 0, st, grid->plan.d_q.get(), grid->plan.d_pot.get(), geom, root, parents, parent_rows,
                           a.d_primitives.get() + 4 * shape.primitive_offset[e], static_cast<uint32_t>(shape.count[e]), branch[e], steps[e], a.d_footprint.get(),
                           static_cast<uint32_t>(n_samples), children, a.d_out.get() + 4 * shape.offset[e]);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(a.h_out.get(), a.d_out.get(), words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(out, a.h_out.get(), words * sizeof(uint32_t));
    return KICP_OK;
}

}  // extern "C"
