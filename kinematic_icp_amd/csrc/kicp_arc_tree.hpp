// kicp_arc_tree.hpp -- the kernel that scores a tree of arc segments on the grid's plan (kicp_grid_score_arc_tree; C-ABI:
// kicp_grid_arc_tree.hip, arithmetic: kicp_arc_tree_host.hpp).  One launch per level on the grid's stream, and stream order is all
// that joins the levels: a level reads the records the level above wrote and nothing of its own.
//   k_arc_tree_level  one wave per node of the level, four nodes per 256-lane workgroup.  Node j hangs under the parent j / branch and
//                     takes the level's primitive j % branch, so the waves of a workgroup are siblings as a rule and read the same
//                     48-byte record; level 1 has no records above it and takes the root from the launch's arguments.  Every lane
//                     reads the record and the primitive at the same address.  A parent that is not alive: lane 0 copies its four
//                     words (and its record, for the levels below) and the wave leaves without a look at the footprint.  Otherwise
//                     the wave rolls the segment as k_arcs_score rolls an arc - the recurrence in every lane, the lanes striding the
//                     samples, a collision a ballot, the largest weight a butterfly of shuffles - and lane 0 stores the record and,
//                     with one 16-byte store, the row.  The last level passes children == nullptr: nobody reads a leaf's record.
// No LDS, no atomics, no barrier of any kind.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_arc_tree_host.hpp"

namespace kicp {

constexpr uint32_t kArcTreeBlock = 256, kArcTreeWave = 64, kArcTreePerBlock = kArcTreeBlock / kArcTreeWave;

// parents: the records of the level above (nullptr at level 1: `root`), parent_rows: that level's rows of results; primitives: this
// level's branch x 4 doubles; children: n_nodes records to write (nullptr at the last level), out: this level's n_nodes x 4 words,
// 16-byte aligned
static __global__ __launch_bounds__(kArcTreeBlock) void k_arc_tree_level(const uint8_t *__restrict__ q, const uint32_t *__restrict__ potential, ArcGeom g, ArcTreeNode root,
                                                                         const ArcTreeNode *__restrict__ parents, const uint32_t *__restrict__ parent_rows,
                                                                         const double *__restrict__ primitives, uint32_t n_nodes, uint32_t branch, uint32_t n_steps,
                                                                         const double *__restrict__ footprint_xy, uint32_t n_samples, ArcTreeNode *__restrict__ children,
                                                                         uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x % kArcTreeWave, j = blockIdx.x * kArcTreePerBlock + threadIdx.x / kArcTreeWave;
    if (j >= n_nodes) return;  // (a whole wave)
    const uint32_t up = j / branch, b = j - up * branch;
    const ArcTreeNode parent = parents ? parents[up] : root;
    if (!parent.alive) {  // (wave-uniform; never at level 1: the root is alive)
        if (lane == 0u) {
            reinterpret_cast<uint4 *>(out)[j] = reinterpret_cast<const uint4 *>(parent_rows)[up];
            if (children) children[j] = parent;
        }
        return;
    }
    ArcTreeNode child;
    uint32_t r[4];
    arc_tree_segment(g, potential, parent, primitives + 4 * static_cast<size_t>(b), n_steps,
                     [&](const ArcPose &p) {
                         uint32_t largest;
                         const bool collides = arc_pose_part(g, q, p, footprint_xy, n_samples, lane, kArcTreeWave, largest);
                         if (__ballot(collides) != 0ull) return 0u;
                         for (int o = 32; o > 0; o >>= 1) {
                             const uint32_t other = __shfl_xor(largest, o);
                             largest = other > largest ? other : largest;
                         }
                         return largest;
                     },
                     child, r);
    if (lane == 0u) {
        if (children) children[j] = child;
        reinterpret_cast<uint4 *>(out)[j] = make_uint4(r[0], r[1], r[2], r[3]);
    }
}

}  // namespace kicp
