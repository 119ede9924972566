// kicp_planar_host.hpp -- the host's side of the planar 3-DoF refinement (kicp_refine_poses_planar): one Gauss-Newton step from the
// eight sums k_planar_poses forms per pose (kicp_planar.hpp).  Plain C++ without any device header, so that a stand-alone program
// can include it (tests/cpp/planar_step_test.cpp).
//
// sums = {N, S_x, S_y, S_ss, S_a, S_b, S_c, ssr}: the number of accepted correspondences, sum s.x, sum s.y, sum (s.x^2 + s.y^2),
// sum a, sum b, sum (s.x b - s.y a), sum |r|^2 (a = c0 . r, b = c1 . r).  The step is free in the plane of the body frame and takes
// neither an odometry prior nor a regularisation: it serves relocalisation, not ComputeRobotMotion.
#pragma once
#include <cmath>

namespace kicp {

constexpr int kPlanarSums = 8;

// dx = -A^-1 g with A = [[N, 0, -S_y], [0, N, S_x], [-S_y, S_x, S_ss]] and g = (S_a, S_b, S_c), in closed form: the first two rows
// give dx and dy from dtheta, the third then reads  dtheta (N S_ss - S_x^2 - S_y^2) = S_x S_b - S_y S_a - N S_c.
// Returns false and leaves dx untouched when N < 1, when a sum or the result is not finite, or when D = N S_ss - S_x^2 - S_y^2 is zero:
// D = N sum |s_xy - mean|^2, zero when all accepted points share one (x, y) - the only degenerate case (A is positive definite
// otherwise).  "Zero" is meant to within what the sums themselves carry: every term of S_x, S_y and S_ss was rounded to 2^-40 before
// it was added (|error| <= N 2^-41 per sum), so D is known to N 2^-41 (N + 2 |S_x| + 2 |S_y|), plus the rounding of the expression
// in fp64; a D at or below that bound is refused (for exact sums of one point the bound is never reached: D is 0).  A real frame is
// ten orders of magnitude above it.
inline bool planar_solve(const double sums[kPlanarSums], double dx[3]) {
    for (int i = 0; i < kPlanarSums; ++i)
        if (!std::isfinite(sums[i])) return false;
    const double n = sums[0], sx = sums[1], sy = sums[2], sss = sums[3], ga = sums[4], gb = sums[5], gc = sums[6];
    if (!(n >= 1.0)) return false;
    const double det = n * sss - sx * sx - sy * sy;
    const double det_error = n * 0x1p-41 * (n + 2.0 * (std::fabs(sx) + std::fabs(sy))) + 4.0 * 2.220446049250313e-16 * n * std::fabs(sss);
    if (!(det > det_error)) return false;
    const double dtheta = (sx * gb - sy * ga - n * gc) / det;
    const double d0 = (sy * dtheta - ga) / n, d1 = (-sx * dtheta - gb) / n;
    if (!std::isfinite(d0) || !std::isfinite(d1) || !std::isfinite(dtheta)) return false;
    dx[0] = d0, dx[1] = d1, dx[2] = dtheta;
    return true;
}
// the twist of the step for pose_exp (kicp_se3.hpp): T <- T * pose_exp({dx, dy, 0, 0, 0, dtheta})
inline void planar_twist(const double dx[3], double xi[6]) { xi[0] = dx[0], xi[1] = dx[1], xi[2] = 0.0, xi[3] = 0.0, xi[4] = 0.0, xi[5] = dx[2]; }
// what the refinement compares with its convergence criterion
inline double planar_step_norm(const double dx[3]) { return std::sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]); }

}  // namespace kicp
