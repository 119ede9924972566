// kicp_arc_tree_host.hpp -- the arithmetic of scoring a tree of arc segments on a plan (kicp_grid_score_arc_tree,
// kicp_score_arc_tree_from_plan; include/kicp.h states the semantics): the record a node leaves for its children and the continuation
// of a record by one segment; and of the pure-host helpers around it (kicp_arc_tree_nodes, kicp_arc_tree_best).  ONE text for the
// kernel (kicp_arc_tree.hpp), for the host entries (kicp_grid_arc_tree.hip) and for the stand-alone program that runs arc_tree_host::
// under sanitizers (tests/cpp/arc_tree_host_test.cpp).  The step, the cell and the pose's weight are kicp_arcs_host.hpp's, unchanged:
// a segment runs arc_score's loop from where the parent stopped, operation by operation, so a prefix rolled once and continued
// gives the bits of a rollout from the start.
#pragma once
#include "kicp_arcs_host.hpp"

namespace kicp {

constexpr uint32_t kArcTreeMaxDepth = 8u;
constexpr size_t kArcTreeMaxNodes = kArcsMaxK;   // nodes of all levels together
constexpr uint32_t kArcTreeMaxT = kArcsMaxT;     // steps along a path: cost_sum <= 1024 * 255

// What a node leaves for its children: the last free pose of its path and the sums along it.  alive: the path took every step of
// every segment so far; a node that is not alive ended at a colliding pose, and its descendants repeat its four words.
struct ArcTreeNode {
    ArcPose pose;
    uint32_t free_steps, cost_sum, cost_max, alive;
};
inline ArcTreeNode arc_tree_root(const double start[4]) { return ArcTreeNode{ArcPose{start[0], start[1], start[2], start[3]}, 0u, 0u, 0u, 1u}; }

// One segment: `n_steps` steps of the primitive `arc` from the record of a parent that is ALIVE -> the child's record and its four
// words (free_steps, cost_sum, cost_max, end_potential).  pose_weight as arc_score's: 0 when the pose collides, else the largest
// weight under the footprint; the loop leaves at the first colliding pose.
template <class PoseWeight>
KICP_HD void arc_tree_segment(const ArcGeom &g, const uint32_t *potential, const ArcTreeNode &parent, const double *arc, uint32_t n_steps, PoseWeight &&pose_weight,
                              ArcTreeNode &child, uint32_t out[4]) {
    const double dx = arc[0], dy = arc[1], dc = arc[2], ds = arc[3];
    ArcPose last = parent.pose;
    uint32_t taken = 0u, free_steps = parent.free_steps, cost_sum = parent.cost_sum, cost_max = parent.cost_max;
    while (taken < n_steps) {
        const ArcPose next = arc_step(last, dx, dy, dc, ds);
        const uint32_t m = pose_weight(next);
        if (m == 0u) break;
        last = next, ++taken, ++free_steps, cost_sum += m, cost_max = m > cost_max ? m : cost_max;
    }
    child.pose = last, child.free_steps = free_steps, child.cost_sum = cost_sum, child.cost_max = cost_max, child.alive = taken == n_steps ? 1u : 0u;
    size_t c;
    out[0] = free_steps, out[1] = cost_sum, out[2] = cost_max, out[3] = arc_cell(g, last.x, last.y, c) ? potential[c] : kNavUnreached;
}

// The shape of a tree: per level e = 0 .. depth - 1 (the header's level e + 1) its nodes, the row its nodes begin at and the row its
// primitives begin at; and the totals.
struct ArcTreeShape {
    uint32_t depth = 0u, total_steps = 0u;
    size_t n_nodes = 0, n_leaves = 0, n_primitives = 0;
    size_t count[kArcTreeMaxDepth] = {}, offset[kArcTreeMaxDepth] = {}, primitive_offset[kArcTreeMaxDepth] = {};
};

namespace arc_tree_host {
enum ShapeError { kShapeOk = 0, kShapeZero, kShapeDepth, kShapeNodes, kShapeSteps };
// kicp_arc_tree_nodes (pointers checked): the counts, or which rule the tree breaks.  Nothing overflows: a level is refused as soon as
// the nodes so far exceed 2^20, and eight 32-bit step counts sum below 2^35.
inline ShapeError nodes(unsigned int depth, const unsigned int *branch, const unsigned int *steps, ArcTreeShape &shape) {
    shape = ArcTreeShape{};
    if (depth < 1u) return kShapeZero;
    if (depth > kArcTreeMaxDepth) return kShapeDepth;
    for (unsigned int e = 0; e < depth; ++e)
        if (branch[e] < 1u || steps[e] < 1u) return kShapeZero;
    unsigned long long total_steps = 0;
    for (unsigned int e = 0; e < depth; ++e) total_steps += steps[e];
    if (total_steps > kArcTreeMaxT) return kShapeSteps;
    size_t level = 1;
    for (unsigned int e = 0; e < depth; ++e) {
        level *= branch[e];  // (at most 2^20 * 2^32)
        shape.count[e] = level, shape.offset[e] = shape.n_nodes, shape.primitive_offset[e] = shape.n_primitives;
        shape.n_nodes += level, shape.n_primitives += branch[e];
        if (shape.n_nodes > kArcTreeMaxNodes) return kShapeNodes;
    }
    shape.depth = depth, shape.total_steps = static_cast<uint32_t>(total_steps), shape.n_leaves = level;
    return kShapeOk;
}
// kicp_score_arc_tree_from_plan (arguments checked): level by level, every node from its parent's record.  Two levels of records are
// live at a time; the leaves leave none.
inline void score(const ArcGeom &g, const uint8_t *q, const uint32_t *potential, const double start[4], const ArcTreeShape &shape, const unsigned int *branch,
                  const unsigned int *steps, const double *primitives, const double *footprint_xy, uint32_t n_samples, ArcTreeNode *parents, ArcTreeNode *children,
                  uint32_t *out) {
    const ArcTreeNode root = arc_tree_root(start);
    for (uint32_t e = 0; e < shape.depth; ++e) {
        const bool leaves = e + 1u == shape.depth;
        for (size_t j = 0; j < shape.count[e]; ++j) {
            const size_t up = j / branch[e], b = j % branch[e];
            const ArcTreeNode &parent = e == 0u ? root : parents[up];
            uint32_t *row = out + 4 * (shape.offset[e] + j);
            if (!parent.alive) {
                const uint32_t *from = out + 4 * (shape.offset[e - 1u] + up);
                row[0] = from[0], row[1] = from[1], row[2] = from[2], row[3] = from[3];
                if (!leaves) children[j] = parent;
                continue;
            }
            ArcTreeNode child;
            arc_tree_segment(g, potential, parent, primitives + 4 * (shape.primitive_offset[e] + b), steps[e],
                             [&](const ArcPose &p) {
                                 uint32_t largest;
                                 return arc_pose_part(g, q, p, footprint_xy, n_samples, 0u, 1u, largest) ? 0u : largest;
                             },
                             child, row);
            if (!leaves) children[j] = child;
        }
        ArcTreeNode *t = parents;
        parents = children, children = t;
    }
}
// kicp_arc_tree_best: arcs_host::best over the leaves' rows with n_steps = the path's steps -> the leaf's in-level index, n_leaves when
// none is admissible; path[e] is the primitive its path takes at level e + 1 (filled when a leaf was found)
inline size_t best(const uint32_t *results, const ArcTreeShape &shape, const unsigned int *branch, uint32_t w_potential, uint32_t w_cost, uint32_t w_blocked,
                   uint32_t min_free_steps, unsigned int *path) {
    const size_t leaf = arcs_host::best(results + 4 * shape.offset[shape.depth - 1u], shape.n_leaves, w_potential, w_cost, w_blocked, shape.total_steps, min_free_steps);
    if (leaf < shape.n_leaves) {
        size_t j = leaf;
        for (uint32_t e = shape.depth; e-- > 0u; j /= branch[e]) path[e] = static_cast<unsigned int>(j % branch[e]);
    }
    return leaf;
}
}  // namespace arc_tree_host

}  // namespace kicp
