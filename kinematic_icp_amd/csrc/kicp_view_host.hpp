// kicp_view_host.hpp -- the geometry and the verdict of the depth view (kicp_view_*, kicp_map_remove_seen_through; include/kicp.h
// states the semantics): the cube-map pixel of an offset from the sensor, the depth a frame point writes there, and whether a world
// point is SEEN THROUGH by the frame the view holds.  ONE text for the kernels (kicp_view.hpp), for the host fall-back of the sweep
// (a map that lives on the host) and for view_host::render / classify / sweep, the host restatement that a stand-alone program runs
// under sanitizers (tests/cpp/view_host_test.cpp).  No atan2, no sqrt: subtractions, divisions, floor and comparisons, every
// operation rounded on its own (-ffp-contract=off), so that numpy restates it bit for bit (tests/view_ref.py).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "kicp_host_map.hpp"
#include "kicp_se3.hpp"

namespace kicp {

constexpr uint32_t kViewMinRes = 8, kViewMaxRes = 1024;  // pixels per face edge (even)
constexpr int32_t kViewMaxWindow = 4;                    // the verdict looks at (2 window + 1)^2 pixels
constexpr uint32_t kViewEmptyBits = 0x7F800000u;         // +inf: a pixel no used point fell into
constexpr uint8_t kViewSeenThrough = 1u, kViewInRange = 2u;  // bits of a verdict

struct ViewGeom {
    uint32_t res;
    int32_t window;
    uint32_t min_rays;
    double max_ray, margin, margin_per_metre;
};
// One frame's constants: the pose the points go through and the sensor's world position c = pose * sensor_xyz (NaN when the pose or
// the sensor is not finite, and before the first frame: no point is used or in range then, a comparison with a NaN being false).
struct ViewFrame {
    Pose pose;
    double cx, cy, cz;
};

KICP_HD bool view_finite(double v) { return fabs(v) <= DBL_MAX; }
inline ViewFrame view_no_frame() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    return ViewFrame{Pose{0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, nan, nan, nan};
}
inline ViewFrame view_frame(const double pose_qt[7], const double sensor_xyz[3]) {
    ViewFrame f = view_no_frame();
    for (int i = 0; i < 7; ++i)
        if (!view_finite(pose_qt[i])) return f;
    for (int i = 0; i < 3; ++i)
        if (!view_finite(sensor_xyz[i])) return f;
    f.pose = Pose{pose_qt[0], pose_qt[1], pose_qt[2], pose_qt[3], pose_qt[4], pose_qt[5], pose_qt[6]};
    double rx, ry, rz;
    quat_rotate(f.pose, sensor_xyz[0], sensor_xyz[1], sensor_xyz[2], rx, ry, rz);
    f.cx = rx + f.pose.tx, f.cy = ry + f.pose.ty, f.cz = rz + f.pose.tz;
    return f;
}

// The offset v = w - c of a world point from the sensor -> its depth m = max(|v.x|, |v.y|, |v.z|) (Chebyshev), its face (the first
// axis in the order x, y, z whose |v| equals m: 2 axis + (negative ? 1 : 0)) and its pixel (u, w) on that face.  False when m is not
// finite, not positive or beyond max_ray: the point is then not used / not in range.
KICP_HD bool view_project(const ViewGeom &g, double vx, double vy, double vz, double &m, uint32_t &face, int32_t &u, int32_t &w) {
    const double ax = fabs(vx), ay = fabs(vy), az = fabs(vz);
    m = fmax(fmax(ax, ay), az);
    if (!(ax <= DBL_MAX && ay <= DBL_MAX && az <= DBL_MAX)) return false;  // (fmax would hide a NaN)
    if (!(0.0 < m && m <= g.max_ray)) return false;
    double a, b;
    if (ax == m) face = vx < 0.0 ? 1u : 0u, a = vy, b = vz;
    else if (ay == m) face = vy < 0.0 ? 3u : 2u, a = vx, b = vz;
    else face = vz < 0.0 ? 5u : 4u, a = vx, b = vy;
    const double half = static_cast<double>(g.res) / 2.0;
    const int32_t last = static_cast<int32_t>(g.res) - 1;
    const int32_t iu = static_cast<int32_t>(floor((a / m + 1.0) * half)), iw = static_cast<int32_t>(floor((b / m + 1.0) * half));
    u = iu < last ? iu : last, w = iw < last ? iw : last;
    return true;
}
KICP_HD size_t view_pixel_index(const ViewGeom &g, uint32_t face, int32_t u, int32_t w) {
    return (static_cast<size_t>(face) * g.res + static_cast<size_t>(w)) * g.res + static_cast<size_t>(u);
}
// A frame point p (base frame): used iff p, w = pose * p (quat_rotate + t, the map update's own transform) and m are finite and
// 0 < m <= max_ray; then `pixel` is its place in the image and `bits` the float it offers, (float)m, as its bit pattern - positive
// floats order like their bits, so the image's minimum is a minimum of unsigned integers.
KICP_HD bool view_render_point(const ViewGeom &g, const ViewFrame &f, double px, double py, double pz, size_t &pixel, uint32_t &bits) {
    if (!(view_finite(px) && view_finite(py) && view_finite(pz))) return false;
    double rx, ry, rz;
    quat_rotate(f.pose, px, py, pz, rx, ry, rz);
    const double wx = rx + f.pose.tx, wy = ry + f.pose.ty, wz = rz + f.pose.tz;
    if (!(view_finite(wx) && view_finite(wy) && view_finite(wz))) return false;
    double m;
    uint32_t face;
    int32_t u, w;
    if (!view_project(g, wx - f.cx, wy - f.cy, wz - f.cz, m, face, u, w)) return false;
    pixel = view_pixel_index(g, face, u, w);
    const float d = static_cast<float>(m);  // round to nearest even
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __float_as_uint(d);
#else
    std::memcpy(&bits, &d, 4);
#endif
    return true;
}
KICP_HD float view_bits_to_float(uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(bits);
#else
    float d;
    std::memcpy(&d, &bits, 4);
    return d;
#endif
}
// The window of a verdict: of the pixels (u + du, w + dw), |du|, |dw| <= W, inside the face, how many hold a return and the smallest value
// among them.  W is a template parameter so that the (2 W + 1)^2 loads are unrolled and issued together - they are independent, their
// latency overlaps; a pixel outside the face is loaded at its clamped place and not looked at, so no load hides behind a branch.
template <int W>
KICP_HD void view_window(const ViewGeom &g, const uint32_t *depth, uint32_t face, int32_t u, int32_t w, uint32_t &seen, uint32_t &nearest) {
    const int32_t last = static_cast<int32_t>(g.res) - 1;
    const uint32_t *plane = depth + static_cast<size_t>(face) * g.res * g.res;
    seen = 0, nearest = kViewEmptyBits;
#pragma unroll
    for (int32_t dj = -W; dj <= W; ++dj) {
        const int32_t j = w + dj, jc = j < 0 ? 0 : (j > last ? last : j);
#pragma unroll
        for (int32_t di = -W; di <= W; ++di) {
            const int32_t i = u + di, ic = i < 0 ? 0 : (i > last ? last : i);
            const uint32_t at = plane[static_cast<size_t>(jc) * g.res + static_cast<size_t>(ic)];
            const uint32_t d = (i == ic && j == jc) ? at : kViewEmptyBits;
            seen += d != kViewEmptyBits ? 1u : 0u;
            nearest = d < nearest ? d : nearest;
        }
    }
}
// The verdict for a world point q against the image `depth` (6 res^2 float bit patterns, face-major): kViewInRange when 0 < m <=
// max_ray, and with it kViewSeenThrough when at least min_rays of the pixels (u + du, w + dw), |du|, |dw| <= window, inside the SAME
// face hold a return and m + (margin + margin_per_metre m) < (double)D for the smallest D among them (fp64, strict).
KICP_HD uint8_t view_verdict(const ViewGeom &g, const ViewFrame &f, const uint32_t *depth, double qx, double qy, double qz) {
    double m;
    uint32_t face;
    int32_t u, w;
    if (!view_project(g, qx - f.cx, qy - f.cy, qz - f.cz, m, face, u, w)) return 0u;
    uint32_t seen, nearest;
    switch (g.window) {  // (0 .. kViewMaxWindow, checked at creation)
        case 0: view_window<0>(g, depth, face, u, w, seen, nearest); break;
        case 1: view_window<1>(g, depth, face, u, w, seen, nearest); break;
        case 2: view_window<2>(g, depth, face, u, w, seen, nearest); break;
        case 3: view_window<3>(g, depth, face, u, w, seen, nearest); break;
        default: view_window<4>(g, depth, face, u, w, seen, nearest); break;
    }
    if (seen < g.min_rays) return kViewInRange;
    const bool through = m + (g.margin + g.margin_per_metre * m) < static_cast<double>(view_bits_to_float(nearest));
    return through ? static_cast<uint8_t>(kViewInRange | kViewSeenThrough) : kViewInRange;
}

// what kicp_view_create checks, for the restatement's callers too: nullptr when the configuration is fine
inline const char *view_config_error(uint32_t res, int32_t window, uint32_t min_rays, double max_ray, double margin, double margin_per_metre) {
    if (res < kViewMinRes || res > kViewMaxRes || (res & 1u)) return "res must be even and within 8 .. 1024";
    if (window < 0 || window > kViewMaxWindow) return "window must be within 0 .. 4";
    if (min_rays < 1u || min_rays > static_cast<uint32_t>((2 * window + 1) * (2 * window + 1))) return "min_rays must be within 1 .. (2 window + 1)^2";
    if (!(max_ray > 0.0) || !view_finite(max_ray)) return "max_ray must be positive and finite";
    if (!(margin >= 0.0) || !view_finite(margin) || !(margin_per_metre >= 0.0) || !view_finite(margin_per_metre)) return "both margins must be finite and not negative";
    return nullptr;
}

namespace view_host {
// One frame on the host, as k_view_render does it: the image is emptied, every used point offers its depth to its pixel, the minimum
// stays.  depth: 6 res^2 bit patterns.  stats: points used, points skipped.
inline ViewFrame render(const ViewGeom &g, uint32_t *depth, const double *xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                        unsigned long long stats[2]) {
    const ViewFrame f = view_frame(pose_qt, sensor_xyz);
    const size_t pixels = 6 * static_cast<size_t>(g.res) * g.res;
    for (size_t i = 0; i < pixels; ++i) depth[i] = kViewEmptyBits;
    stats[0] = stats[1] = 0;
    for (size_t i = 0; i < n; ++i) {
        size_t pixel;
        uint32_t bits;
        if (!view_render_point(g, f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], pixel, bits)) {
            ++stats[1];
            continue;
        }
        ++stats[0];
        if (bits < depth[pixel]) depth[pixel] = bits;
    }
    return f;
}
inline void classify(const ViewGeom &g, const ViewFrame &f, const uint32_t *depth, const double *xyz, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; ++i) out[i] = view_verdict(g, f, depth, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}
// The sweep over a host map: every point of every occupied voxel gets the verdict, seen-through points leave their bucket.
// stats: points in range, points removed, voxels that lost at least one point, voxels erased.
inline void sweep(const ViewGeom &g, const ViewFrame &f, const uint32_t *depth, HostMap &map, unsigned long long stats[4]) {
    unsigned long long in_range = 0, removed[3];
    map.RemovePointsIf(
        [&](const double *p) {
            const uint8_t v = view_verdict(g, f, depth, p[0], p[1], p[2]);
            in_range += (v & kViewInRange) ? 1u : 0u;
            return (v & kViewSeenThrough) != 0;
        },
        removed);
    stats[0] = in_range, stats[1] = removed[0], stats[2] = removed[1], stats[3] = removed[2];
}
}  // namespace view_host

}  // namespace kicp
