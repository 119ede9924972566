// kicp_scroll_host.hpp -- the arithmetic of scrolling a plane of cells so that the map follows the robot (kicp_grid_scroll,
// kicp_elev_scroll, kicp_*_follow, kicp_shift_plane, kicp_follow_shift; include/kicp.h states the semantics): which destination cells
// of a shifted plane have a source, the shift itself on the host, the origin after a shift and the shift that brings a cell back
// into the band.  ONE text for the kernel (kicp_scroll.hpp), for the entries (kicp_grid.hip, kicp_elev.hip) and for the stand-alone
// program that runs it under sanitizers (tests/cpp/scroll_host_test.cpp).  No HIP here: the file compiles on its own.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#ifndef KICP_HD  // (the library's units include kicp_common.hpp first, which says __host__ __device__)
#define KICP_HD inline
#endif

namespace kicp {

// The destination cells of a plane shifted by (dx, dy) that have a source inside the plane: x0 <= ix < x1 and y0 <= iy < y1, empty
// (x0 >= x1 or y0 >= y1) when |dx| >= width or |dy| >= height.  Destination (ix, iy) reads source (ix + dx, iy + dy).
struct ScrollValid {
    int64_t x0, x1, y0, y1;
};
KICP_HD ScrollValid scroll_valid(uint32_t width, uint32_t height, int32_t dx, int32_t dy) {
    const int64_t w = width, h = height, sx = dx, sy = dy;
    ScrollValid v;
    v.x0 = sx < 0 ? -sx : 0, v.x1 = sx > 0 ? w - sx : w;
    v.y0 = sy < 0 ? -sy : 0, v.y1 = sy > 0 ? h - sy : h;
    return v;
}
KICP_HD bool scroll_empties(uint32_t width, uint32_t height, int32_t dx, int32_t dy) {
    const ScrollValid v = scroll_valid(width, height, dx, dy);
    return v.x0 >= v.x1 || v.y0 >= v.y1;
}

namespace scroll_host {
// The shift on the host: `out` = `in` shifted by (dx, dy), zero where the source lies outside; the two do not overlap.
inline void shift_plane(const void *in, void *out, uint32_t width, uint32_t height, uint32_t elem_bytes, int32_t dx, int32_t dy) {
    const size_t row_bytes = static_cast<size_t>(width) * elem_bytes;
    std::memset(out, 0, row_bytes * height);
    const ScrollValid v = scroll_valid(width, height, dx, dy);
    if (v.x0 >= v.x1 || v.y0 >= v.y1) return;
    const size_t run = static_cast<size_t>(v.x1 - v.x0) * elem_bytes;
    for (int64_t iy = v.y0; iy < v.y1; ++iy)
        std::memcpy(static_cast<unsigned char *>(out) + static_cast<size_t>(iy) * row_bytes + static_cast<size_t>(v.x0) * elem_bytes,
                    static_cast<const unsigned char *>(in) + static_cast<size_t>(iy + dy) * row_bytes + static_cast<size_t>(v.x0 + dx) * elem_bytes, run);
}
// origin + (double)d * cell: the product rounded, then the sum (-ffp-contract=off; the volatile keeps a compiler without that flag
// from fusing the two)
inline double scroll_origin(double origin, int32_t d, double cell) {
    volatile double step = static_cast<double>(d) * cell;
    return origin + step;
}
// One axis of the follow rule: the shift d that brings cell c into [margin, size - margin), 0 when it is there already, else the
// least multiple of `step` that does.  false: margin < 1, step < 1, 2 margin + step > size, or a d outside 64 bits.
inline bool follow_shift(long long c, uint32_t size, uint32_t margin, uint32_t step, long long *d) {
    if (margin < 1u || step < 1u || 2ull * margin + step > size) return false;
    const __int128 cc = c, lo = margin, hi = static_cast<__int128>(size) - margin, s = step;
    __int128 r = 0;
    if (cc < lo) r = -s * ((lo - cc + s - 1) / s);
    else if (cc >= hi) r = s * ((cc - hi + 1 + s - 1) / s);
    if (r < static_cast<__int128>(INT64_MIN) || r > static_cast<__int128>(INT64_MAX)) return false;
    *d = static_cast<long long>(r);
    return true;
}
// Both axes for a position (x, y): its cell by the grid's own arithmetic (grid_cell, kicp_grid_host.hpp: floor((x - origin) / cell)),
// then the rule.  0: *dx and *dy are set; 1: the position is not finite or its cell lies beyond +-2^30; 2: a bad margin or step.
// (|d| <= 2^30 + size + step < 2^31: size <= 2^28.)
inline int follow_shifts(double x, double y, double origin_x, double origin_y, double cell, uint32_t width, uint32_t height, uint32_t margin, uint32_t step,
                         int32_t *dx, int32_t *dy) {
    const double cx = floor((x - origin_x) / cell), cy = floor((y - origin_y) / cell);
    if (!(fabs(cx) <= 1073741824.0 && fabs(cy) <= 1073741824.0)) return 1;  // (a NaN fails both)
    long long sx, sy;
    if (!follow_shift(static_cast<long long>(cx), width, margin, step, &sx) || !follow_shift(static_cast<long long>(cy), height, margin, step, &sy)) return 2;
    *dx = static_cast<int32_t>(sx), *dy = static_cast<int32_t>(sy);
    return 0;
}
// The last window's corner after a shift by (dx, dy): the corner minus the shift.  false: a corner has left +-2^30 - no plane (at most
// 2^28 cells) can hold a cell of a window (at most 8191 cells wide) from there, so the handle then forgets the window (has_window),
// which is exact and keeps kicp_*_last_window's arithmetic inside 32-bit corners.
inline bool scroll_window(int32_t &win_x0, int32_t &win_y0, int32_t dx, int32_t dy) {
    const int64_t x = static_cast<int64_t>(win_x0) - dx, y = static_cast<int64_t>(win_y0) - dy, far = 1ll << 30;
    if (x < -far || x > far || y < -far || y > far) return false;
    win_x0 = static_cast<int32_t>(x), win_y0 = static_cast<int32_t>(y);
    return true;
}
}  // namespace scroll_host

}  // namespace kicp
