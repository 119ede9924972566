// planar_solve (kicp_planar_host.hpp) and the pose update it feeds (pose_exp / pose_mul of kicp_se3.hpp) in a stand-alone program:
//   * dx = -A^-1 g against a Gaussian elimination with partial pivoting on random well-conditioned sums (formed from random points, so
//     that A is the J^T J of a real configuration), residual |A dx + g| at the level of rounding;
//   * the degenerate rows - N = 0, one point, all points on one (x, y), NaN and infinite sums - return false and leave dx untouched;
//   * a zero gradient gives a zero step and the pose it started from; a step's pose is pose * (yaw, V (dx, dy)) in closed form.
// Built by tests/test_planar_host.py with g++ -fsanitize=address,undefined; prints "ok <checks>".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "kicp_planar_host.hpp"
#include "kicp_se3.hpp"

using namespace kicp;

static long checks = 0, bad = 0;
static void expect(bool ok, const char *what) {
    ++checks;
    if (!ok) ++bad, std::printf("FAILED: %s\n", what);
}
static void eliminate(double A[3][3], double b[3], double x[3]) {
    for (int c = 0; c < 3; ++c) {
        int piv = c;
        for (int r = c + 1; r < 3; ++r)
            if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
        for (int k = 0; k < 3; ++k) std::swap(A[c][k], A[piv][k]);
        std::swap(b[c], b[piv]);
        for (int r = c + 1; r < 3; ++r) {
            const double f = A[r][c] / A[c][c];
            for (int k = c; k < 3; ++k) A[r][k] -= f * A[c][k];
            b[r] -= f * b[c];
        }
    }
    for (int r = 2; r >= 0; --r) {
        double v = b[r];
        for (int k = r + 1; k < 3; ++k) v -= A[r][k] * x[k];
        x[r] = v / A[r][r];
    }
}

int main() {
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> coord(-30.0, 30.0), resid(-0.5, 0.5), angle(-3.0, 3.0);
    const double untouched[3] = {7.0, 8.0, 9.0};
    for (int trial = 0; trial < 200; ++trial) {
        const int n = 3 + static_cast<int>(rng() % 400);
        double s[kPlanarSums] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < n; ++i) {
            const double x = coord(rng), y = coord(rng), a = resid(rng), b = resid(rng), c = resid(rng);
            s[0] += 1.0, s[1] += x, s[2] += y, s[3] += x * x + y * y, s[4] += a, s[5] += b, s[6] += x * b - y * a, s[7] += a * a + b * b + c * c;
        }
        double dx[3] = {untouched[0], untouched[1], untouched[2]};
        expect(planar_solve(s, dx), "a well-conditioned row is solved");
        double A[3][3] = {{s[0], 0.0, -s[2]}, {0.0, s[0], s[1]}, {-s[2], s[1], s[3]}}, g[3] = {-s[4], -s[5], -s[6]}, want[3];
        eliminate(A, g, want);
        for (int k = 0; k < 3; ++k) expect(std::fabs(dx[k] - want[k]) <= 1e-11 * (std::fabs(want[k]) + 1e-3), "dx equals the elimination's");
        // the pose update against the closed form of a planar twist
        const double yaw = angle(rng);
        const Pose T{0.0, 0.0, std::sin(0.5 * yaw), std::cos(0.5 * yaw), coord(rng) * 0.25, coord(rng) * 0.25, 0.3};
        double xi[6];
        planar_twist(dx, xi);
        const Pose next = pose_mul(T, pose_exp(xi));
        const double th = dx[2], va = std::fabs(th) < 1e-10 ? 1.0 : std::sin(th) / th, vb = std::fabs(th) < 1e-10 ? 0.5 * th : (1.0 - std::cos(th)) / th;
        const double bx = va * dx[0] - vb * dx[1], by = vb * dx[0] + va * dx[1];
        expect(std::fabs(next.tx - (T.tx + std::cos(yaw) * bx - std::sin(yaw) * by)) < 1e-13 && std::fabs(next.ty - (T.ty + std::sin(yaw) * bx + std::cos(yaw) * by)) < 1e-13 &&
                   next.tz == T.tz,
               "translation of the updated pose");
        const double qz = std::sin(0.5 * (yaw + th)), qw = std::cos(0.5 * (yaw + th));
        const double sign = (qz * next.qz + qw * next.qw) < 0 ? -1.0 : 1.0;
        expect(std::fabs(sign * next.qz - qz) < 1e-14 && std::fabs(sign * next.qw - qw) < 1e-14 && next.qx == 0.0 && next.qy == 0.0, "rotation of the updated pose");
        expect(std::fabs(planar_step_norm(dx) - std::sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2])) == 0.0, "step norm");
    }
    // degenerate rows: false, dx untouched
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double rows[][kPlanarSums] = {
        {0, 0, 0, 0, 0, 0, 0, 0},                                             // no correspondence
        {1, 1.5, -2.0, 6.25, 0.1, 0.2, 0.7, 0.05},                           // one point
        {5, 7.5, -10.0, 31.25, 0.5, 1.0, 3.5, 0.25},                         // five points on (1.5, -2)
        {3, nan, 1, 9, 0, 0, 0, 1},     {3, 1, 1, 9, inf, 0, 0, 1},     {nan, 1, 1, 9, 0, 0, 0, 1},     {3, 1, 1, 9, 0, 0, 0, nan},
        {0.5, 0.1, 0.1, 9, 0, 0, 0, 1},                                       // N < 1
    };
    for (const auto &row : rows) {
        double dx[3] = {untouched[0], untouched[1], untouched[2]};
        expect(!planar_solve(row, dx), "a degenerate row is refused");
        expect(std::memcmp(dx, untouched, sizeof dx) == 0, "and dx is left as it was");
    }
    // a zero gradient: a zero step, the same pose
    {
        const double row[kPlanarSums] = {4, 2.0, -1.0, 30.0, 0.0, 0.0, 0.0, 0.5};
        double dx[3] = {1, 1, 1}, xi[6];
        expect(planar_solve(row, dx) && dx[0] == 0.0 && dx[1] == 0.0 && dx[2] == 0.0, "zero gradient, zero step");
        planar_twist(dx, xi);
        const Pose T{0.0, 0.0, 0.6, 0.8, 3.0, -4.0, 0.5};
        const Pose next = pose_mul(T, pose_exp(xi));
        expect(next.qx == T.qx && next.qy == T.qy && std::fabs(next.qz - T.qz) < 2e-16 && std::fabs(next.qw - T.qw) < 2e-16 && next.tx == T.tx && next.ty == T.ty &&
                   next.tz == T.tz,
               "a zero step leaves the pose");
    }
    std::printf("%s %ld\n", bad ? "bad" : "ok", checks);
    return bad ? 1 : 0;
}
