// kicp_grid_internal.hpp -- what the translation units of the 2-D occupancy grid (kicp_grid*.hip) share: the handle behind kicp_grid,
// the rules its entries keep, and the argument checks that more than one of them makes.  include/kicp.h states the semantics.  The
// pieces, each the only translation unit that includes its kernel headers (the arithmetic they share with the host: *_host.hpp):
//   kicp_grid.hip          the grid itself (kicp_grid.hpp): create / destroy / info / clear, integrate, counts / set_counts and their
//                          rectangles, the occupancy readout, last_window, write_map / save_map, fill_unknown and its host twin, and
//                          the window that follows the robot (kicp_scroll.hpp - the second kernel header two units include:
//                          kicp_elev.hip scrolls its columns with it): scroll, follow, kicp_shift_plane, kicp_follow_shift
//   kicp_grid_plan.hip     what a planner plans on (kicp_clear.hpp, kicp_nav.hpp): clearance and costmap with their host twins,
//                          kicp_grid_cost_table_nav2, kicp_plan_weights, the three potential entries, kicp_potential_path, kicp_plan_q,
//                          kicp_grid_has_plan - one file because kicp_grid_potential queues the costmap's launches in front of the field's
//   kicp_grid_arcs.hip     a fan of arcs scored on the plan (kicp_arcs.hpp): kicp_grid_score_arcs, its host twin, kicp_arc_steps,
//                          kicp_footprint_box, kicp_arcs_best
//   kicp_grid_arc_tree.hip a tree of arc segments scored on the plan (kicp_arc_tree.hpp): kicp_grid_score_arc_tree, its host twin,
//                          kicp_arc_tree_nodes, kicp_arc_tree_best
//   kicp_grid_explore.hip  where to go while mapping (kicp_front.hpp, kicp_gain.hpp): the frontiers and the viewpoints' gain, each
//                          with its host twin
//   kicp_grid_transient.hip what stands in known free space right now (kicp_transient.hpp, and kicp_front.hpp once more for its
//                          union-find - the one kernel header two units include): kicp_grid_transients and its host twin, the
//                          transient plane and the switch that makes its cells sources of the clearance
#pragma once
#include "kicp_clear_host.hpp"
#include "kicp_internal.hpp"

// (an internal header of six translation units that all begin this way)
using namespace kicp;
using namespace kicp::host;
namespace kicp {
struct ArcTreeNode;  // kicp_arc_tree_host.hpp: the handle only holds a buffer of them
}

// CONST ENTRIES.  The C-ABI takes `const kicp_grid *` wherever a call leaves the map as it was: info, counts, occupancy, clearance,
// costmap, the two potential entries, has_plan, score_arcs, score_arc_tree, frontiers, gain, last_window, save_map.  Such an entry reads the top-level
// members - the counters among them - and writes only the groups declared `mutable` below: scratch whose contents no later call
// relies on, but for the plan, which is the one thing a const entry leaves behind on purpose.  kicp_grid_transients* and
// kicp_grid_use_transients take the handle non-const: the transient plane and the switch are top-level state that clearance, costmap
// and potential read; kicp_grid_transient_plane and kicp_grid_uses_transients only read them.
//
// THE STREAM RULE.  Every entry returns with the handle's stream drained, so the next one finds it idle and may let a buffer grow
// (DevBuf::reserve frees the old memory) without a synchronisation of its own.  The one exception: kicp_grid_potential queues the
// costmap's launches and goes on without waiting for them (clear_on_device with out == nullptr, kicp_grid_plan.hip).  What grows
// behind them is the `plan` group alone, which those launches do not touch; clear.d_cost, which they write and the field reads, has
// its size by then.  (The frame's buffers - FrameUpload::put, frame.d_rays - synchronise before they grow all the same.)
struct kicp_grid {
    int device = 0;
    kicp_grid_config cfg{};
    GridGeom geom{};
    size_t cells = 0;
    DevBuf<uint16_t> d_counts;  // the map: cells x 2, hits and misses
    hipStream_t stream = nullptr;
    unsigned long long frames = 0;
    bool has_window = false;  // a frame has been integrated since creation or the last clear: (win_x0, win_y0) is its window's lower corner
    int32_t win_x0 = 0, win_y0 = 0;
    // THE TRANSIENT PLANE, a byte per cell: 1 on the cells of the last kicp_grid_transients call's transients that passed min_size.  Not
    // allocated (and read as all 0) until the first such call.  use_transients is the switch: clear_on_device ORs the plane into its sources.
    DevBuf<uint8_t> d_transient_plane;
    bool use_transients = false;
    // kicp_grid_scroll: the buffers a shift writes into, swapped with d_counts and d_transient_plane afterwards.  Not allocated until
    // the first shift that needs them, then kept: a scrolled handle holds its counters (and its plane, if it has one) twice.
    DevBuf<uint16_t> d_counts_spare;
    DevBuf<uint8_t> d_transient_spare;
    // kicp_grid_integrate*: the two frame-local planes over the window, zero between frames, and the frame in flight
    struct {
        uint32_t plane_words = 0;       // ceil((2 reach + 1)^2 / 4)
        DevBuf<uint32_t> d_hit, d_miss, d_rays;  // d_rays: the ray list, the window cells that became HIT (room for one per point)
        DevBuf<unsigned int> d_stats;   // used, cells HIT, cells MISS, and the length of d_rays
        PinnedBuf<unsigned int> h_stats;
        FrameUpload upload;             // kicp_grid_integrate's points
    } frame;
    mutable struct { DevBuf<int8_t> d_occupancy; } readout;  // kicp_grid_occupancy
    // kicp_grid_fill_unknown (this handle the destination): the seven counts in their shards
    struct {
        DevBuf<unsigned int> d_counts;
        PinnedBuf<unsigned int> h_counts;
    } fill;
    // kicp_grid_clearance / kicp_grid_costmap: the column distances, the caller's table and the two results
    mutable struct {
        DevBuf<uint8_t> d_coldist, d_cost_table, d_cost;
        DevBuf<uint16_t> d_clearance;
    } clear;
    // kicp_grid_potential*.  THE PLAN is d_q (= weight[costmap]) and d_pot as the last potential call left them, and `valid` says
    // that it succeeded: what kicp_grid_score_arcs, kicp_grid_score_arc_tree and kicp_grid_frontiers(use_plan) read.  The costmap is not part of it.  Beside
    // it the call's scratch: the weight table, the goal list, the tiles' activity flags (two planes) and the counters - raised flags
    // of each round of a batch, then the cells below and at max_potential.
    mutable struct {
        bool valid = false;
        DevBuf<uint8_t> d_q, d_weight, d_flags;
        DevBuf<uint32_t> d_pot, d_goals, d_ctr;
        PinnedBuf<uint32_t> h_ctr;
    } plan;
    // kicp_grid_score_arcs: its uploads, its results and the pinned buffer they come back through
    mutable struct {
        DevBuf<double> d_arcs, d_footprint;
        DevBuf<uint32_t> d_out;
        PinnedBuf<uint32_t> h_out;
    } arcs;
    // kicp_grid_score_arc_tree: its uploads, the records of two levels (each level's nodes read the half the level above wrote), the
    // rows of all levels and the pinned buffer they come back through
    mutable struct {
        DevBuf<double> d_primitives, d_footprint;
        DevBuf<ArcTreeNode> d_records;
        DevBuf<uint32_t> d_out;
        PinnedBuf<uint32_t> h_out;
    } arc_tree;
    // kicp_grid_frontiers: a byte per cell, the parent plane that becomes the label plane, the roots' row numbers, the count of
    // roots, the rows and where they and the count land
    mutable struct {
        DevBuf<uint8_t> d_flags;
        DevBuf<uint32_t> d_parent, d_row_of, d_ctr;
        DevBuf<unsigned long long> d_rows;
        PinnedBuf<uint32_t> h_ctr;
        std::vector<unsigned long long> h_rows;
    } front;
    // kicp_grid_transients*: the returns and the flags per cell (both zero between calls), the touched list (room for one entry per
    // point), the parent plane that becomes the label plane, the roots' row numbers, the statistics and the count of roots (word 4),
    // the rows and where they land
    struct {
        bool ready = false;  // the planes are allocated and zero
        DevBuf<uint32_t> d_returns, d_touched, d_parent, d_row_of;
        DevBuf<uint8_t> d_flags;
        DevBuf<unsigned int> d_stats;
        PinnedBuf<unsigned int> h_stats;
        DevBuf<unsigned long long> d_rows;
        std::vector<unsigned long long> h_rows;
    } transient;
    // kicp_grid_gain: a byte per cell, the viewpoints' upload, their rows and the pinned buffer the rows come back through
    mutable struct {
        DevBuf<uint8_t> d_classes;
        DevBuf<uint32_t> d_views, d_out;
        PinnedBuf<uint32_t> h_out;
    } gain;
    ~kicp_grid() {
        if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
    }
};

namespace kicp {
namespace host {
// ---- the checks that more than one entry makes -------------------------------------------------------------------
// how a call sorts the cells into occupied, free and unknown: min_observations and occupied_thresh, the latter as the kernels take it
inline int check_cell_classes(unsigned int min_observations, double occupied_thresh, int32_t &source_min) {
    if (min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    if (!(0.0 <= occupied_thresh && occupied_thresh <= 1.0)) return fail(KICP_ERR_ARG, "occupied_thresh must lie in [0, 1]");
    source_min = clear_source_min(occupied_thresh);
    return KICP_OK;
}
// the dimensions a pure-host entry is given (kicp_grid_create words its own limit)
inline int check_grid_dims(unsigned int width, unsigned int height) {
    if (width == 0 || height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    if (static_cast<unsigned long long>(width) * height > kGridMaxCells) return fail(KICP_ERR_CAPACITY, "width * height exceeds 2^28 = " + std::to_string(kGridMaxCells));
    return KICP_OK;
}
inline int check_cell_origin(double cell, double origin_x, double origin_y) {
    if (!(cell > 0.0) || !std::isfinite(cell) || !std::isfinite(origin_x) || !std::isfinite(origin_y)) return fail(KICP_ERR_ARG, "cell must be positive and finite, the origin finite");
    return KICP_OK;
}
inline int check_has_plan(const kicp_grid *grid) {
    if (!grid->plan.valid)
        return fail(KICP_ERR_ARG, "the handle holds no plan: call kicp_grid_potential or kicp_grid_potential_of_costmap first (a call of theirs that failed left none)");
    return KICP_OK;
}
inline void copy_stats(unsigned long long out_stats[4], const unsigned long long stats[4]) {
    if (out_stats)
        for (int k = 0; k < 4; ++k) out_stats[k] = stats[k];
}
}  // namespace host
}  // namespace kicp
