// kicp_bridge.hpp -- glue between the reference's C++ value types and the C-ABI of include/kicp.h.
// With the real Eigen/Sophus the same code compiles: only the two param-conversion helpers differ.
#pragma once
#include <Eigen/Core>
#include <Eigen/Geometry>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <sophus/se3.hpp>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "kicp.h"

namespace kicp_bridge {
// Sophus::SE3d <-> the C-ABI's 7 parameters [qx qy qz qw tx ty tz] (Sophus' own parameter order; Eigen::Quaterniond's
// constructor takes w first).  The same code for the real Sophus and for cpp/compat.  from_params goes through Sophus'
// normalising quaternion constructor, like any SE3d a caller builds from a quaternion.
inline void to_params(const Sophus::SE3d &T, double p[7]) {
    const auto &q = T.unit_quaternion();
    p[0] = q.x(), p[1] = q.y(), p[2] = q.z(), p[3] = q.w();
    p[4] = T.translation().x(), p[5] = T.translation().y(), p[6] = T.translation().z();
}
inline Sophus::SE3d from_params(const double p[7]) {
    return Sophus::SE3d(Eigen::Quaterniond(p[3], p[0], p[1], p[2]), Eigen::Vector3d(p[4], p[5], p[6]));
}
// what tbb::this_task_arena::max_concurrency() answers in the reference's constructors (Registration.cpp:141-142): the hardware
// threads of this machine, at least one
inline int hardware_threads() {
    const unsigned n = std::thread::hardware_concurrency();
    return n > 0u ? static_cast<int>(n) : 1;
}
inline const double *xyz(const std::vector<Eigen::Vector3d> &v) {
    static_assert(sizeof(Eigen::Vector3d) == 3 * sizeof(double), "Eigen::Vector3d must be 3 packed doubles");
    return v.empty() ? nullptr : v.front().data();
}
// Candidate poses for KinematicICP::Relocalize / KinematicRegistration::Relocalize (kicp.h kicp_planar_grid): center * planar(dx, dy,
// dyaw) for every offset i * step within the half extents, offsets in the centre's body frame, x slowest, yaw fastest.
inline std::vector<Sophus::SE3d> planar_grid(const Sophus::SE3d &center, double half_x, double half_y, double half_yaw, double step_x, double step_y,
                                             double step_yaw) {
    double c[7];
    to_params(center, c);
    std::vector<double> flat(7 * kicp_planar_grid(c, half_x, half_y, half_yaw, step_x, step_y, step_yaw, nullptr, 0));
    kicp_planar_grid(c, half_x, half_y, half_yaw, step_x, step_y, step_yaw, flat.data(), flat.size() / 7);
    std::vector<Sophus::SE3d> poses;
    poses.reserve(flat.size() / 7);
    for (size_t k = 0; k < flat.size() / 7; ++k) poses.push_back(from_params(&flat[7 * k]));
    return poses;
}
inline std::vector<double> to_params(const std::vector<Sophus::SE3d> &poses) {
    std::vector<double> flat(7 * poses.size());
    for (size_t k = 0; k < poses.size(); ++k) to_params(poses[k], &flat[7 * k]);
    return flat;
}
// Which GPU the drop-in classes use: the reference API has no notion of a device, so the choice travels out of band -
// KICP_DEVICE in the environment (default 0), read once per process.
inline int default_device() {
    static const int device = [] {
        const char *e = std::getenv("KICP_DEVICE");
        return e && *e ? std::atoi(e) : 0;
    }();
    return device;
}
// The record layout of the FLOAT32 clouds the backend writes (VoxelHashMap::PointcloudF32, KinematicICP::LocalMapF32 /
// RegisterFrameF32 / RegisterIngestedFrameF32): what EigenToPointCloud2 (ros/.../utils/RosUtils.cpp:40-63) declares in the message,
// so a ROS-side caller fills msg->fields, point_step, height, width and is_bigendian from it and hands msg->data to the backend.
struct PointCloud2Xyz32 {
    static constexpr const char *field_names[3] = {"x", "y", "z"};
    static constexpr uint32_t field_offsets[3] = {0, 4, 8};
    static constexpr uint8_t datatype = KICP_FIELD_FLOAT32;  // sensor_msgs::msg::PointField::FLOAT32
    static constexpr uint32_t count = 1;                     // per field
    static constexpr uint32_t point_step = 12;
    static constexpr uint32_t height = 1;                    // width = number of points, row_step = 12 * width
    static constexpr bool is_bigendian = false;
};
// The reference's core throws nothing; a backend failure must not return garbage silently.
inline int check(int rc, const char *what) {
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + kicp_last_error());
    return rc;  // (> 0: a warning code of include/kicp.h; the result still follows the reference's convention)
}
// The occupancy pyramid of a map for KinematicRegistration::RelocalizeSearch (kicp.h kicp_occ_build): a snapshot that owns its device
// memory and does not follow later map updates; shared, because nothing changes it once it is built.
inline std::shared_ptr<kicp_occ> build_occupancy(kicp_map *map, double cell, int dilate = 1, int levels = 4, int device = -1) {
    kicp_occ *occ = nullptr;
    check(kicp_occ_build(map, device < 0 ? default_device() : device, cell, dilate, levels, &occ), "kicp_bridge::build_occupancy");
    return std::shared_ptr<kicp_occ>(occ, kicp_occ_destroy);
}
// The search window around a point of the map, or - with half extents <= 0 - over the pyramid's whole footprint (kicp.h
// kicp_search_window_around); z: the base frame's height, yaw_step: the spacing of the full circle of yaws.
inline kicp_search_window search_window_around(const kicp_occ *occ, const Eigen::Vector2d &center, double half_x, double half_y, double z, double yaw_step) {
    const double c[2] = {center.x(), center.y()};
    kicp_search_window w{};
    check(kicp_search_window_around(occ, c, half_x, half_y, z, yaw_step, &w), "kicp_bridge::search_window_around");
    return w;
}
// The 2-D occupancy grid a mapping run draws for a planner (kicp.h kicp_grid_*): KinematicICP::EnableGrid takes a GridConfig and holds
// the handle shared, so a node can keep KinematicICP::Grid() for its map publisher.  clone_grid is the deep copy a copied pipeline
// gets: a grid of the same configuration with the same counters (its frame count and its last window start again).
// GridClearanceConfig and GridRect are what KinematicICP::GridClearance / GridCostmap take: the classes and the radius, and a rectangle
// of cells (x0, y0, w, h) - GridLastWindow returns one, grown() is that rectangle R cells larger on every side and clipped.
using GridConfig = kicp_grid_config;
using GridClearanceConfig = kicp_grid_clearance_config;
struct GridRect {
    unsigned int x0 = 0, y0 = 0, w = 0, h = 0;
    bool empty() const { return w == 0 || h == 0; }
    GridRect grown(unsigned int cells, unsigned int width, unsigned int height) const {
        GridRect g;
        g.x0 = x0 > cells ? x0 - cells : 0u, g.y0 = y0 > cells ? y0 - cells : 0u;
        const unsigned long long x1 = static_cast<unsigned long long>(x0) + w + cells, y1 = static_cast<unsigned long long>(y0) + h + cells;
        g.w = static_cast<unsigned int>(x1 < width ? x1 : width) - g.x0, g.h = static_cast<unsigned int>(y1 < height ? y1 : height) - g.y0;
        return g;
    }
};
// PlanConfig, plan_weights and potential_path go with KinematicICP::GridPotential / GridPotentialOfCostmap / PotentialPath (kicp.h
// kicp_plan_weights .. kicp_grid_potential): the clamp of the cost-to-go field, NavFn's weight per cost, and the walk down a potential.
using PlanConfig = kicp_plan_config;
inline std::array<uint8_t, 256> plan_weights(unsigned int neutral = 50, unsigned int factor_num = 4, unsigned int factor_den = 5, unsigned int lethal_from = 253,
                                             unsigned int unknown_weight = 0) {
    std::array<uint8_t, 256> weight{};
    check(kicp_plan_weights(neutral, factor_num, factor_den, lethal_from, unknown_weight, weight.data()), "kicp_bridge::plan_weights");
    return weight;
}
inline std::vector<std::array<unsigned int, 2>> potential_path(const std::vector<uint32_t> &potential, const std::vector<uint8_t> &costmap, unsigned int width,
                                                               unsigned int height, const std::array<uint8_t, 256> &weight, const std::array<unsigned int, 2> &start) {
    if (potential.size() != static_cast<size_t>(width) * height || costmap.size() != potential.size())
        throw std::runtime_error("kicp_bridge::potential_path: the potential and the costmap must have width * height cells");
    std::vector<std::array<unsigned int, 2>> cells(static_cast<size_t>(width) + height);
    size_t n = 0;
    int rc = kicp_potential_path(potential.data(), costmap.data(), width, height, weight.data(), start[0], start[1], cells.front().data(), cells.size(), &n);
    if (rc == KICP_ERR_CAPACITY && n > cells.size()) {  // the path is longer: its length came back
        cells.resize(n);
        rc = kicp_potential_path(potential.data(), costmap.data(), width, height, weight.data(), start[0], start[1], cells.front().data(), cells.size(), &n);
    }
    check(rc, "kicp_bridge::potential_path");
    cells.resize(n);
    return cells;
}
// ArcStart, ArcStep, ArcResult, arc_start, arc_steps, footprint_box and best_arc go with KinematicICP::ScoreArcs (kicp.h kicp_plan_q ..
// kicp_grid_score_arcs): where the rollout starts (x, y, cosine, sine), one step of an arc (dx, dy, dc, ds), what an arc scores
// (free_steps, cost_sum, cost_max, end_potential), the arcs of a list of commands, a box footprint's samples and the ranking.
using ArcStart = std::array<double, 4>;
using ArcStep = std::array<double, 4>;
using ArcResult = std::array<uint32_t, 4>;
using FootprintSample = std::array<double, 2>;
// the start of a pose: its translation's x and y, and the base frame's x axis projected into the world's plane as a unit vector
inline ArcStart arc_start(const Sophus::SE3d &pose) {
    const auto &q = pose.unit_quaternion();
    const double c = 1.0 - 2.0 * (q.y() * q.y() + q.z() * q.z()), s = 2.0 * (q.x() * q.y() + q.z() * q.w()), n = std::sqrt(c * c + s * s);
    if (!(n > 0.0)) throw std::runtime_error("kicp_bridge::arc_start: the pose's x axis has no heading in the plane");
    return {pose.translation().x(), pose.translation().y(), c / n, s / n};
}
inline std::vector<ArcStep> arc_steps(const std::vector<double> &v, const std::vector<double> &omega, double dt) {
    if (v.size() != omega.size()) throw std::runtime_error("kicp_bridge::arc_steps: v and omega must have the same length");
    std::vector<ArcStep> arcs(v.size());
    check(kicp_arc_steps(v.data(), omega.data(), dt, v.size(), arcs.empty() ? nullptr : arcs.front().data()), "kicp_bridge::arc_steps");
    return arcs;
}
inline std::vector<FootprintSample> footprint_box(double x_min, double x_max, double y_min, double y_max, double spacing) {
    size_t n = 0;
    const int rc = kicp_footprint_box(x_min, x_max, y_min, y_max, spacing, nullptr, 0, &n);
    if (rc != KICP_ERR_CAPACITY || n == 0) check(rc, "kicp_bridge::footprint_box");  // the count came back with KICP_ERR_CAPACITY
    std::vector<FootprintSample> samples(n);
    check(kicp_footprint_box(x_min, x_max, y_min, y_max, spacing, samples.front().data(), samples.size(), &n), "kicp_bridge::footprint_box");
    return samples;
}
// the index of the best arc, results.size() when none is admissible
inline size_t best_arc(const std::vector<ArcResult> &results, unsigned int n_steps, unsigned int w_potential = 1, unsigned int w_cost = 0, unsigned int w_blocked = 0,
                       unsigned int min_free_steps = 1) {
    size_t index = results.size();
    check(kicp_arcs_best(results.empty() ? nullptr : results.front().data(), results.size(), w_potential, w_cost, w_blocked, n_steps, min_free_steps, &index),
          "kicp_bridge::best_arc");
    return index;
}
// ArcTree, ArcTreeCounts, ArcTreeLeaf, arc_tree_nodes and best_arc_tree_leaf go with KinematicICP::ScoreArcTree (kicp.h
// kicp_arc_tree_nodes .. kicp_grid_score_arc_tree): a tree of arc segments - level d + 1 offers branch[d] primitives, each held for
// steps[d] steps; primitives holds the levels' rows one after the other, level 1's first - the counts that size its results, and the
// leaf a ranking picks with the primitive its path takes at every level (path[0] is the command to execute now).
struct ArcTree {
    std::vector<unsigned int> branch, steps;
    std::vector<ArcStep> primitives;
};
struct ArcTreeCounts {
    size_t n_nodes = 0, n_leaves = 0;
    unsigned int total_steps = 0;
    std::vector<size_t> level_offset;  // the row each level's nodes begin at
};
struct ArcTreeLeaf {
    bool found = false;
    size_t leaf = 0;  // the in-level index at the last level; n_leaves when none is admissible
    std::vector<unsigned int> path;
};
inline ArcTreeCounts arc_tree_nodes(const ArcTree &tree) {
    if (tree.branch.size() != tree.steps.size()) throw std::runtime_error("kicp_bridge::arc_tree_nodes: branch and steps must have the same length");
    ArcTreeCounts counts;
    counts.level_offset.resize(tree.branch.size());
    check(kicp_arc_tree_nodes(static_cast<unsigned int>(tree.branch.size()), tree.branch.data(), tree.steps.data(), &counts.n_nodes, &counts.n_leaves, &counts.total_steps,
                              counts.level_offset.data()),
          "kicp_bridge::arc_tree_nodes");
    size_t rows = 0;
    for (unsigned int b : tree.branch) rows += b;
    if (tree.primitives.size() != rows) throw std::runtime_error("kicp_bridge::arc_tree_nodes: the tree needs " + std::to_string(rows) + " primitives, one row per entry of branch");
    return counts;
}
inline ArcTreeLeaf best_arc_tree_leaf(const std::vector<ArcResult> &results, const ArcTree &tree, unsigned int w_potential = 1, unsigned int w_cost = 0,
                                      unsigned int w_blocked = 0, unsigned int min_free_steps = 1) {
    const ArcTreeCounts counts = arc_tree_nodes(tree);
    if (results.size() != counts.n_nodes) throw std::runtime_error("kicp_bridge::best_arc_tree_leaf: the tree has " + std::to_string(counts.n_nodes) + " nodes, one result each");
    ArcTreeLeaf best;
    best.path.resize(tree.branch.size());
    check(kicp_arc_tree_best(results.front().data(), static_cast<unsigned int>(tree.branch.size()), tree.branch.data(), tree.steps.data(), w_potential, w_cost, w_blocked,
                             min_free_steps, &best.leaf, best.path.data()),
          "kicp_bridge::best_arc_tree_leaf");
    best.found = best.leaf < counts.n_leaves;
    if (!best.found) best.path.clear();
    return best;
}
// FrontierConfig and Frontier go with KinematicICP::GridFrontiers (kicp.h kicp_grid_frontiers): the classes' thresholds and the least
// size of a frontier that is output, and one frontier - the ten words of its row by name.  The centroid is in cells, as doubles: the
// middle of cell (x, y) lies at origin + (x + 0.5, y + 0.5) * cell in the world.
using FrontierConfig = kicp_frontier_config;
struct Frontier {
    uint32_t label = 0;  // the least cell index y * width + x of its cells
    uint64_t size = 0, sum_x = 0, sum_y = 0;
    uint32_t min_x = 0, max_x = 0, min_y = 0, max_y = 0;
    uint32_t best_potential = 0xFFFFFFFFu, best_cell = 0;  // the least potential of the plan over its cells (0xFFFFFFFF: none reached, or no plan asked for) and where
    double centroid_x() const { return static_cast<double>(sum_x) / static_cast<double>(size); }
    double centroid_y() const { return static_cast<double>(sum_y) / static_cast<double>(size); }
};
inline Frontier frontier_of_row(const unsigned long long *row) {
    Frontier f;
    f.label = static_cast<uint32_t>(row[0]), f.size = row[1], f.sum_x = row[2], f.sum_y = row[3];
    f.min_x = static_cast<uint32_t>(row[4]), f.max_x = static_cast<uint32_t>(row[5]), f.min_y = static_cast<uint32_t>(row[6]), f.max_y = static_cast<uint32_t>(row[7]);
    f.best_potential = static_cast<uint32_t>(row[8]), f.best_cell = static_cast<uint32_t>(row[9]);
    return f;
}
// TransientConfig and Transient go with KinematicICP::EnableTransients and ::Transients (kicp.h kicp_grid_transients): what makes a cell
// of known free space a transient cell and the least size of a transient that counts, and one transient - the ten words of its row by
// name.  The centroid is weighted by the returns, in cells, as doubles; nearest_d2 is the squared distance in cells from the sensor's
// cell to nearest_cell, the transient's cell closest to it.
using TransientConfig = kicp_transient_config;
struct Transient {
    uint32_t label = 0;  // the least cell index y * width + x of its cells
    uint64_t size = 0, returns = 0, sum_nx = 0, sum_ny = 0;
    uint32_t min_x = 0, max_x = 0, min_y = 0, max_y = 0;
    uint32_t nearest_d2 = 0, nearest_cell = 0;
    double centroid_x() const { return static_cast<double>(sum_nx) / static_cast<double>(returns); }
    double centroid_y() const { return static_cast<double>(sum_ny) / static_cast<double>(returns); }
};
inline Transient transient_of_row(const unsigned long long *row) {
    Transient t;
    t.label = static_cast<uint32_t>(row[0]), t.size = row[1], t.returns = row[2], t.sum_nx = row[3], t.sum_ny = row[4];
    t.min_x = static_cast<uint32_t>(row[5]), t.max_x = static_cast<uint32_t>(row[6]), t.min_y = static_cast<uint32_t>(row[7]), t.max_y = static_cast<uint32_t>(row[8]);
    t.nearest_d2 = static_cast<uint32_t>(row[9] >> 32), t.nearest_cell = static_cast<uint32_t>(row[9] & 0xFFFFFFFFull);
    return t;
}
// GainConfig and Gain go with KinematicICP::GridGain (kicp.h kicp_grid_gain): the classes' thresholds and the sensor's range in cells,
// and what one candidate viewpoint would see - the four words of its row by name.
using GainConfig = kicp_gain_config;
struct Gain {
    uint32_t seen = 0;        // distinct unknown cells the rays cross
    uint32_t blocked = 0;     // rays that end at an occupied cell
    uint32_t left = 0;        // rays that leave the grid
    uint32_t view_class = 0;  // the viewpoint's own cell: 0 clear, 1 unknown, 2 occupied - then no ray was walked
};
inline Gain gain_of_row(const unsigned int *row) { return Gain{row[0], row[1], row[2], row[3]}; }
inline std::shared_ptr<kicp_grid> make_grid(const GridConfig &config, int device = -1) {
    kicp_grid *grid = nullptr;
    check(kicp_grid_create(&config, device < 0 ? default_device() : device, &grid), "kicp_bridge::make_grid");
    return std::shared_ptr<kicp_grid>(grid, kicp_grid_destroy);
}
inline std::shared_ptr<kicp_grid> clone_grid(const kicp_grid *grid, int device = -1) {
    if (!grid) return nullptr;
    GridConfig config{};
    check(kicp_grid_info(grid, &config, nullptr, nullptr), "kicp_bridge::clone_grid");
    const size_t cells = static_cast<size_t>(config.width) * config.height;
    std::vector<unsigned short> counts(2 * cells);
    check(kicp_grid_counts(grid, counts.data(), cells), "kicp_bridge::clone_grid");
    auto copy = make_grid(config, device);
    check(kicp_grid_set_counts(copy.get(), counts.data(), cells), "kicp_bridge::clone_grid");
    check(kicp_grid_use_transients(copy.get(), kicp_grid_uses_transients(grid)), "kicp_bridge::clone_grid");  // the switch; the copy's transient plane starts empty
    return copy;
}
// Following (kicp.h FOLLOWING): what KinematicICP::EnableGridFollow and EnableElevationFollow keep - the band's margin and the step, in
// cells, and the shift the last frame applied.  make_follow checks the pair against the handle's width and height by
// kicp_follow_shift's own rule (std::invalid_argument).
struct Follow {
    bool enabled = false;
    unsigned int margin_cells = 0, step_cells = 0;
    std::array<int, 2> last{{0, 0}};  // (dx, dy) of the last frame; (0, 0) before the first and while following is off
};
inline Follow make_follow(unsigned int width, unsigned int height, unsigned int margin_cells, unsigned int step_cells, const char *what) {
    long long d = 0;
    if (kicp_follow_shift(0, width, margin_cells, step_cells, &d) != KICP_OK || kicp_follow_shift(0, height, margin_cells, step_cells, &d) != KICP_OK)
        throw std::invalid_argument(std::string(what) + ": " + kicp_last_error());
    return Follow{true, margin_cells, step_cells, {{0, 0}}};
}
// The height columns a mapping run keeps for uneven ground (kicp.h kicp_elev_*): KinematicICP::EnableElevation takes an ElevationConfig
// and holds the handle shared, so a node can keep KinematicICP::Elevation() - for kicp_elev_to_grid into its planner's grid, say.
// clone_elevation is the deep copy a copied pipeline gets: a layer of the same configuration with the same columns (its frame count
// and its last window start again).  ElevationTraversabilityConfig is what KinematicICP::ElevationTraversability takes: the highest
// step and the robot's height, in slabs.  ElevationStats: the six words of a frame.
using ElevationConfig = kicp_elev_config;
using ElevationTraversabilityConfig = kicp_elev_traversability_config;
using ElevationStats = std::array<unsigned long long, KICP_ELEV_STATS>;  // used, skipped, outside_grid, outside_column, new_bits, new_cells
// what KinematicICP::EnableElevationCarving takes - margin_steps, widen_slabs, keep_ground - and the nine words of an update: the six
// above, then carve_points, bits_cleared, cells_emptied
using ElevationCarveConfig = kicp_elev_carve_config;
using ElevationCarveStats = std::array<unsigned long long, KICP_ELEV_UPDATE_STATS>;
// what KinematicICP::ElevationTraversabilitySlope takes beside the traversability configuration: radius_cells, gate_slabs, min_cells,
// rise_slabs, run_cells of the plane fit (kicp.h THE SLOPE LIMIT); KinematicICP::ElevationSlopeLimit fills the last two from a tangent
using ElevationSlopeConfig = kicp_elev_slope_config;
// what KinematicICP::ElevationTraversabilityRough adds to that: num / den slabs^2, the limit of the fit's mean squared residual (kicp.h
// ROUGH); KinematicICP::ElevationRoughLimit makes one from an r.m.s. residual in metres.  GridFillConfig is what
// KinematicICP::ElevationIntoGrid takes to fill the planner's grid from the pipeline's own (kicp.h THE FILL), GridFillCounts its seven words.
using ElevationRoughConfig = kicp_elev_rough_config;
using GridFillConfig = kicp_grid_fill_config;
using GridFillCounts = std::array<unsigned long long, KICP_GRID_FILL_COUNTS>;
inline std::shared_ptr<kicp_elev> make_elevation(const ElevationConfig &config, int device = -1) {
    kicp_elev *elev = nullptr;
    check(kicp_elev_create(&config, device < 0 ? default_device() : device, &elev), "kicp_bridge::make_elevation");
    return std::shared_ptr<kicp_elev>(elev, kicp_elev_destroy);
}
inline std::shared_ptr<kicp_elev> clone_elevation(const kicp_elev *elev, int device = -1) {
    if (!elev) return nullptr;
    ElevationConfig config{};
    check(kicp_elev_info(elev, &config, nullptr, nullptr), "kicp_bridge::clone_elevation");
    const size_t cells = static_cast<size_t>(config.width) * config.height;
    std::vector<unsigned long long> columns(cells);
    check(kicp_elev_columns(elev, columns.data(), cells), "kicp_bridge::clone_elevation");
    auto copy = make_elevation(config, device);
    check(kicp_elev_set_columns(copy.get(), columns.data(), cells), "kicp_bridge::clone_elevation");
    return copy;
}
// The depth view behind KinematicICP::EnableSeeThroughRemoval (kicp.h kicp_view_*): the image of the frame just registered, against
// which the map is swept.  clone_view is what a copied pipeline gets: a view of the same configuration (the image is per frame: the
// copy renders its own).
using ViewConfig = kicp_view_config;
inline std::shared_ptr<kicp_view> make_view(const ViewConfig &config, int device = -1) {
    kicp_view *view = nullptr;
    check(kicp_view_create(&config, device < 0 ? default_device() : device, &view), "kicp_bridge::make_view");
    return std::shared_ptr<kicp_view>(view, kicp_view_destroy);
}
inline std::shared_ptr<kicp_view> clone_view(const kicp_view *view, int device = -1) {
    if (!view) return nullptr;
    ViewConfig config{};
    check(kicp_view_info(view, &config, nullptr, nullptr), "kicp_bridge::clone_view");
    return make_view(config, device);
}
// a warning the reference has no channel for: once per process on stderr
inline void warn_once(const char *message) {
    static bool said = false;
    if (!said) std::fprintf(stderr, "[kicp] warning: %s\n", message);
    said = true;
}
// KICP_TRACE=1: host-side sections of the drop-in headers report their wall time on stderr, next to the library's own
// per-call lines (debugging aid; a getenv once per process otherwise)
struct Trace {
    static bool enabled() {
        static const bool on = [] {
            const char *e = std::getenv("KICP_TRACE");
            return e && *e && *e != '0';
        }();
        return on;
    }
    const char *name;
    std::chrono::steady_clock::time_point t0;
    explicit Trace(const char *n) : name(n) {
        if (enabled()) t0 = std::chrono::steady_clock::now();
    }
    void lap(const char *next) {
        if (!enabled()) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[kicp host] %-30s %9.3f ms\n", name, std::chrono::duration<double, std::milli>(t1 - t0).count());
        name = next, t0 = t1;
    }
    ~Trace() { lap(""); }
};
}  // namespace kicp_bridge
