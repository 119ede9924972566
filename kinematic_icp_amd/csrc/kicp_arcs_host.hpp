// kicp_arcs_host.hpp -- the arithmetic of scoring a fan of arc trajectories on a plan (kicp_grid_score_arcs,
// kicp_score_arcs_from_plan; include/kicp.h states the semantics): one step of the rollout, the cell of a footprint sample, a pose's
// weight and the loop over one arc's poses; and of the pure-host helpers around it (kicp_arc_steps, kicp_footprint_box,
// kicp_arcs_best).  ONE text for the kernel (kicp_arcs.hpp), for the host entries (kicp_grid_arcs.hip) and for the stand-alone program that
// runs arcs_host:: under sanitizers (tests/cpp/arcs_host_test.cpp).  fp64 + - * / floor only, every operation rounded on its own
// (-ffp-contract=off); no transcendental except in arcs_host::steps, which fills the arcs on the host.
//
// The plan is q per cell (a byte, 0 impassable) and the potential (kicp_nav_host.hpp).  The cell of a world coordinate is the grid's
// own grid_cell (kicp_grid_host.hpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "kicp_grid_host.hpp"
#include "kicp_nav_host.hpp"

namespace kicp {

constexpr uint32_t kArcsMaxK = 1u << 20;  // arcs per call
constexpr uint32_t kArcsMaxT = 1024u;     // steps per arc: cost_sum <= 1024 * 255
constexpr uint32_t kArcsMaxP = 4096u;     // footprint samples

struct ArcPose {
    double x, y, c, s;  // the base frame's origin in world metres, its heading as cosine and sine
};
struct ArcGeom {
    double cell, origin_x, origin_y;
    uint32_t width, height;
};

// one step (dx, dy, dc, ds) of an arc, expressed in the robot's frame, from pose p
KICP_HD ArcPose arc_step(const ArcPose &p, double dx, double dy, double dc, double ds) {
    ArcPose n;
    n.x = p.x + (p.c * dx - p.s * dy);
    n.y = p.y + (p.s * dx + p.c * dy);
    n.c = p.c * dc - p.s * ds;
    n.s = p.s * dc + p.c * ds;
    return n;
}
// The cell of a world point: false when it lies outside the grid or a coordinate is not finite (a comparison with a NaN is false, and
// an infinite quotient is no cell of any grid).
KICP_HD bool arc_cell(const ArcGeom &g, double wx, double wy, size_t &cell_index) {
    const double cx = grid_cell(wx, g.origin_x, g.cell), cy = grid_cell(wy, g.origin_y, g.cell);
    if (!(cx >= 0.0 && cx < static_cast<double>(g.width) && cy >= 0.0 && cy < static_cast<double>(g.height))) return false;
    cell_index = static_cast<size_t>(cy) * g.width + static_cast<size_t>(cx);
    return true;
}
// the weight of the footprint sample (fx, fy), base frame, at pose p: q of its cell, 0 outside the grid
KICP_HD uint32_t arc_sample_weight(const ArcGeom &g, const uint8_t *q, const ArcPose &p, double fx, double fy) {
    const double wx = p.x + (p.c * fx - p.s * fy), wy = p.y + (p.s * fx + p.c * fy);
    size_t c;
    return arc_cell(g, wx, wy, c) ? q[c] : 0u;
}
// The samples first, first + stride, ... (below n_samples) of a footprint at pose p: does one of them collide, and the largest weight
// among them (0 when there is none).  The host takes (0, 1); lane l of a wave takes (l, 64).
KICP_HD bool arc_pose_part(const ArcGeom &g, const uint8_t *q, const ArcPose &p, const double *footprint_xy, uint32_t n_samples, uint32_t first, uint32_t stride,
                           uint32_t &largest) {
    bool collides = false;
    largest = 0u;
    for (uint32_t i = first; i < n_samples; i += stride) {
        const uint32_t w = arc_sample_weight(g, q, p, footprint_xy[2 * i], footprint_xy[2 * i + 1]);
        collides = collides || w == 0u;
        largest = w > largest ? w : largest;
    }
    return collides;
}
// One arc.  pose_weight(pose) is 0 when the pose collides, else the largest weight under the footprint; the loop leaves at the first
// colliding pose.  out: free_steps, cost_sum, cost_max, end_potential.
template <class PoseWeight>
KICP_HD void arc_score(const ArcGeom &g, const uint32_t *potential, const ArcPose &start, const double *arc, uint32_t n_steps, PoseWeight &&pose_weight,
                       uint32_t out[4]) {
    const double dx = arc[0], dy = arc[1], dc = arc[2], ds = arc[3];
    ArcPose last = start;
    uint32_t free_steps = 0u, cost_sum = 0u, cost_max = 0u;
    while (free_steps < n_steps) {
        const ArcPose next = arc_step(last, dx, dy, dc, ds);
        const uint32_t m = pose_weight(next);
        if (m == 0u) break;
        last = next, ++free_steps, cost_sum += m, cost_max = m > cost_max ? m : cost_max;
    }
    size_t c;
    out[0] = free_steps, out[1] = cost_sum, out[2] = cost_max, out[3] = arc_cell(g, last.x, last.y, c) ? potential[c] : kNavUnreached;
}

namespace arcs_host {
// kicp_score_arcs_from_plan (arguments checked): every arc in turn
inline void score(const ArcGeom &g, const uint8_t *q, const uint32_t *potential, const double start[4], const double *arcs, size_t n_arcs, uint32_t n_steps,
                  const double *footprint_xy, uint32_t n_samples, uint32_t *out) {
    const ArcPose s{start[0], start[1], start[2], start[3]};
    for (size_t k = 0; k < n_arcs; ++k)
        arc_score(g, potential, s, arcs + 4 * k, n_steps,
                  [&](const ArcPose &p) {
                      uint32_t largest;
                      return arc_pose_part(g, q, p, footprint_xy, n_samples, 0u, 1u, largest) ? 0u : largest;
                  },
                  out + 4 * k);
}
// kicp_arc_steps: the arc a command (v, omega) drives in dt.  The branch stands where the reference adds an epsilon to theta
// (Registration.cpp's motion model), which divides by zero at theta = -epsilon.
// sin and cos are called through pointers the compiler does not see through: one that knows both merges them into a sincos call, and the
// C library's sincos differs from its sin and cos in the last bit for about one argument in a thousand.
inline void steps(const double *v, const double *omega, double dt, size_t n, double *out) {
    double (*volatile sine)(double) = static_cast<double (*)(double)>(std::sin);
    double (*volatile cosine)(double) = static_cast<double (*)(double)>(std::cos);
    for (size_t k = 0; k < n; ++k) {
        const double d = v[k] * dt, theta = omega[k] * dt;
        const double sn = sine(theta), cs = cosine(theta);
        if (std::fabs(theta) < 1e-9) {
            out[4 * k] = d, out[4 * k + 1] = 0.0;
        } else {
            out[4 * k] = d * sn / theta, out[4 * k + 1] = d * (1.0 - cs) / theta;
        }
        out[4 * k + 2] = cs, out[4 * k + 3] = sn;
    }
}
// the lattice's points along one axis: ceil((hi - lo) / spacing) + 1 (arguments checked: finite, lo <= hi, spacing > 0)
inline double box_count(double lo, double hi, double spacing) { return std::ceil((hi - lo) / spacing) + 1.0; }
inline double box_coordinate(double lo, double hi, size_t i, size_t n) { return n > 1 ? lo + (hi - lo) * static_cast<double>(i) / static_cast<double>(n - 1) : lo; }
// kicp_footprint_box: nx * ny points, row-major in y (x runs fastest); the first min(nx * ny, cap) are stored
inline void box(double x_min, double x_max, double y_min, double y_max, size_t nx, size_t ny, double *out_xy, size_t cap) {
    for (size_t j = 0, i = 0; j < ny && i < cap; ++j)
        for (size_t k = 0; k < nx && i < cap; ++k, ++i) out_xy[2 * i] = box_coordinate(x_min, x_max, k, nx), out_xy[2 * i + 1] = box_coordinate(y_min, y_max, j, ny);
}
// kicp_arcs_best: the admissible arc of least score, lowest index on a tie; n_arcs when none is admissible
inline size_t best(const uint32_t *results, size_t n_arcs, uint32_t w_potential, uint32_t w_cost, uint32_t w_blocked, uint32_t n_steps, uint32_t min_free_steps) {
    size_t at = n_arcs;
    uint64_t least = 0;
    for (size_t k = 0; k < n_arcs; ++k) {
        const uint32_t *r = results + 4 * k;
        if (r[0] < min_free_steps || r[3] == kNavUnreached) continue;
        const uint64_t blocked = n_steps > r[0] ? n_steps - r[0] : 0u;
        const uint64_t score = static_cast<uint64_t>(w_potential) * r[3] + static_cast<uint64_t>(w_cost) * r[1] + static_cast<uint64_t>(w_blocked) * blocked;
        if (at == n_arcs || score < least) at = k, least = score;
    }
    return at;
}
}  // namespace arcs_host

}  // namespace kicp
