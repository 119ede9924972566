// kicp_elev_host.hpp -- the arithmetic of the height columns (kicp_elev_*, include/kicp.h): the class of one point, the ground of one
// column, BODY and STEP of one cell, the slope limit - one window cell into the nine sums of a plane fit, its determinants and the
// 128-bit comparison -, ROUGH - a tenth sum, the fit's residual and its comparison -, and the carve along a frame's rays: which points
// carve, the slab of a ray at a step, a step's mask and what it clears of a column.  ONE text for the kernels (kicp_elev.hpp), for the
// pure-host entries (kicp_elev_traversability_from_columns, .._slope_from_columns, .._rough_from_columns, kicp_elev_update_columns) and
// for elev_host::integrate / carve / update / classify / classify_fit (behind classify_slope and classify_rough), the host restatements that stand-alone
// programs run under sanitizers (tests/cpp/elev_host_test.cpp, elev_carve_host_test.cpp, elev_slope_host_test.cpp, elev_rough_host_test.cpp).
// Everything is exact and integer from the floor on.
#pragma once
#include "kicp_grid_host.hpp"

namespace kicp {

constexpr uint32_t kElevSlabs = 64;      // bits of a column
constexpr uint8_t kElevNoGround = 255u;  // the ground byte of an empty column
constexpr uint32_t kElevMaxStep = 62;    // step_slabs; step_slabs < robot_slabs <= 64

// the layer's geometry: the plane is the grid's (its band is not used: every return counts), the vertical is z_origin + b * slab
struct ElevGeom {
    GridGeom plane;
    double z_origin, slab;
};
// One frame's constants: the grid's (rows 0 and 1, the sensor's cell, the window's corner) and row 2 of pose_to_rt's R and t.
struct ElevFrame {
    GridFrame plane;
    double r2[3], t2;
};
struct ElevParams {
    uint32_t step_slabs, robot_slabs;  // S, H: 0 <= S <= 62, S < H <= 64
};
struct ElevRect {
    uint32_t x0, y0, w, h;
};

enum ElevClass : int { kElevSkipped = 0, kElevOutsideGrid = 1, kElevOutsideColumn = 2, kElevUsed = 3 };

// What the class of a point and its ray share: is the point SKIPPED (-> false), and if not, its cell (integer valued doubles) and its
// world height.  Every comparison is made on doubles before any conversion, and a comparison with a NaN is false: a sensor cell that
// is not finite skips everything.
KICP_HD bool elev_locate(const ElevGeom &g, const ElevFrame &f, double px, double py, double pz, double &cx, double &cy, double &wz) {
    if (!(fabs(px) <= DBL_MAX && fabs(py) <= DBL_MAX && fabs(pz) <= DBL_MAX)) return false;
    const double wx = grid_world(f.plane.r, f.plane.t[0], px, py, pz), wy = grid_world(f.plane.r + 3, f.plane.t[1], px, py, pz);
    wz = grid_world(f.r2, f.t2, px, py, pz);
    if (!(fabs(wx) <= DBL_MAX && fabs(wy) <= DBL_MAX && fabs(wz) <= DBL_MAX)) return false;
    cx = grid_cell(wx, g.plane.origin_x, g.plane.cell), cy = grid_cell(wy, g.plane.origin_y, g.plane.cell);
    const double reach = static_cast<double>(g.plane.reach);
    return fabs(cx - f.plane.sx) <= reach && fabs(cy - f.plane.sy) <= reach;
}
// The class of one point, tested in the header's order; for a used point the cell's index and the slab.
KICP_HD ElevClass elev_point(const ElevGeom &g, const ElevFrame &f, double px, double py, double pz, size_t &cell_index, uint32_t &slab) {
    double cx, cy, wz;
    if (!elev_locate(g, f, px, py, pz, cx, cy, wz)) return kElevSkipped;
    if (!(cx >= 0.0 && cx < static_cast<double>(g.plane.width) && cy >= 0.0 && cy < static_cast<double>(g.plane.height))) return kElevOutsideGrid;
    const double s = floor((wz - g.z_origin) / g.slab);
    if (!(s >= 0.0 && s <= 63.0)) return kElevOutsideColumn;
    cell_index = static_cast<size_t>(cy) * g.plane.width + static_cast<size_t>(cx);
    slab = static_cast<uint32_t>(s);
    return kElevUsed;
}

// the frame constants of a pose and a sensor origin (host: pose_to_rt is evaluated here, once per frame)
inline ElevFrame elev_frame(const ElevGeom &g, const double pose_qt[7], const double sensor_xyz[3]) {
    const Rt m = pose_to_rt(Pose{pose_qt[0], pose_qt[1], pose_qt[2], pose_qt[3], pose_qt[4], pose_qt[5], pose_qt[6]});
    ElevFrame f;
    f.plane = grid_frame(g.plane, pose_qt, sensor_xyz);
    f.r2[0] = m.r[6], f.r2[1] = m.r[7], f.r2[2] = m.r[8], f.t2 = m.t[2];
    return f;
}

// bits lo .. 63 of a column; lo reaches 64 and beyond (g + S + 1, g + H + 1), where a shift is undefined in C++ and modulo 64 on the
// hardware: there the set is empty
KICP_HD uint64_t elev_bits_from(uint32_t lo) { return lo >= kElevSlabs ? 0ull : ~0ull << lo; }
// the ground of a column: the index of its lowest set bit, 255 for an empty one
KICP_HD uint8_t elev_ground(uint64_t column) { return column ? static_cast<uint8_t>(__builtin_ctzll(column)) : kElevNoGround; }
// BODY: some bit b of the column with g + S < b <= g + H (g its ground; the column is not empty)
KICP_HD bool elev_body(uint64_t column, uint32_t ground, const ElevParams &p) {
    return (column & elev_bits_from(ground + p.step_slabs + 1u) & ~elev_bits_from(ground + p.robot_slabs + 1u)) != 0ull;
}
// STEP against one neighbour: it is known and its ground lies more than S slabs below this cell's
KICP_HD bool elev_step(uint32_t ground, uint8_t neighbour_ground, const ElevParams &p) {
    return neighbour_ground != kElevNoGround && ground > static_cast<uint32_t>(neighbour_ground) + p.step_slabs;
}
// the value of a cell and the count it adds to: 0 unknown, 1 traversable, 2 BODY, 3 STEP only, 4 SLOPE only, 5 ROUGH only; the plain
// classification passes neither slope nor rough, the slope limit no rough.  The count as a chain of overrides from the weakest reason
// to the strongest: written so, the plain kernels compile to the code they had with a function of their own.
KICP_HD int8_t elev_value(uint32_t &which, bool known, bool body, bool step, bool slope = false, bool rough = false) {
    which = 1u;
    if (rough) which = 5u;
    if (slope) which = 4u;
    if (step) which = 3u;
    if (body) which = 2u;
    if (!known) which = 0u;
    return !known ? static_cast<int8_t>(-1) : static_cast<int8_t>((body || step || slope || rough) ? 100 : 0);
}

// ---- the slope limit: a least-squares plane through the known grounds of a window (kicp_elev_traversability_slope*) ---------------
constexpr uint32_t kElevSlopeMaxRadius = 8, kElevSlopeMaxGate = 63, kElevSlopeMinCells = 3, kElevSlopeMaxRatio = 65535;

struct ElevSlopeParams {
    uint32_t radius, gate, min_cells, rise, run;  // L, K, the fewest cells of a fit, and the limit: rise slabs per run cells
};
// The nine sums over a cell's FIT SET, z = g_n - g.  At L = 8: n <= 289, Sxx, Syy <= 6 936, |Sxy| <= 5 184, |Sz| <= 18 207, |Sxz|, |Syz| <=
// 77 112 - 32 bits with room.  ROUGH's tenth, Szz = sum z^2 <= 289 * 63^2 = 1 147 041 over the same set, stays zero for the slope limit.
struct ElevFitSums {
    int32_t n, sx, sy, sxx, sxy, syy, sz, sxz, syz, szz;
};
// One window cell (dx, dy) with ground byte neighbour_ground into the sums of a cell with ground g, when it belongs: known and
// |g_n - g| <= K.  ONE unsigned comparison does both: K <= 63 and g <= 63, so the 255 of an unknown cell (or of one outside the grid)
// gives 255 - g + K >= 192 + K > 2 K.  Rough: z^2 too.
template <bool Rough>
KICP_HD void elev_fit_add(ElevFitSums &s, uint32_t ground, uint8_t neighbour_ground, int32_t dx, int32_t dy, uint32_t gate) {
    if (static_cast<uint32_t>(neighbour_ground) - ground + gate > 2u * gate) return;
    const int32_t z = static_cast<int32_t>(neighbour_ground) - static_cast<int32_t>(ground);
    s.n += 1, s.sx += dx, s.sy += dy, s.sxx += dx * dx, s.sxy += dx * dy, s.syy += dy * dy, s.sz += z, s.sxz += dx * z, s.syz += dy * z;
    if constexpr (Rough) s.szz += z * z;
}
// Cramer's rule on the normal equations of z ~ a dx + b dy + c: the gradient is (Da / D, Db / D) slabs per cell.  D is a Gram
// determinant: >= 0, and 0 when the set lies on one line.  D < 2^34, |Da|, |Db| < 2^41, every product below 2^42: 64 bits.
KICP_HD void elev_slope_determinants(const ElevFitSums &s, int64_t &d, int64_t &da, int64_t &db) {
    const int64_t n = s.n, sx = s.sx, sy = s.sy, sxx = s.sxx, sxy = s.sxy, syy = s.syy, sz = s.sz, sxz = s.sxz, syz = s.syz;
    d = sxx * (syy * n - sy * sy) - sxy * (sxy * n - sy * sx) + sx * (sxy * sy - syy * sx);
    da = sxz * (syy * n - sy * sy) - sxy * (syz * n - sy * sz) + sx * (syz * sy - syy * sz);
    db = sxx * (syz * n - sz * sy) - sxz * (sxy * n - sy * sx) + sx * (sxy * sz - syz * sx);
}
// the cell HAS A FIT
KICP_HD bool elev_slope_has_fit(const ElevFitSums &s, int64_t d, const ElevSlopeParams &p) { return static_cast<uint32_t>(s.n) >= p.min_cells && d > 0; }
// SLOPE of a cell that has a fit: (Da^2 + Db^2) run^2 > rise^2 D^2, strictly, on exact integers: the left side stays below 2^115, the
// right below 2^100 - 128-bit products, no division, no floating point.
KICP_HD bool elev_slope_exceeds(int64_t d, int64_t da, int64_t db, const ElevSlopeParams &p) {
    typedef unsigned __int128 u128;
    const u128 a = static_cast<uint64_t>(da < 0 ? -da : da), b = static_cast<uint64_t>(db < 0 ? -db : db), dd = static_cast<uint64_t>(d);
    const uint64_t run2 = static_cast<uint64_t>(p.run) * p.run, rise2 = static_cast<uint64_t>(p.rise) * p.rise;
    return (a * a + b * b) * run2 > dd * dd * rise2;
}

// ---- ROUGH: the residual of that plane fit (kicp_elev_traversability_rough*) ------------------------------------------------------
constexpr uint32_t kElevRoughMaxRatio = 65535;

struct ElevRoughParams {
    uint32_t num, den;  // the limit: a mean squared residual of num / den slabs^2
};
// what a cell's fit and the counts hold: D, Da, Db and five classes; with ROUGH also Q, n and a sixth
template <bool Rough>
constexpr uint32_t kElevFitValues = Rough ? 5u : 3u;
template <bool Rough>
constexpr uint32_t kElevFitCounts = Rough ? 6u : 5u;
// Q = D Szz - Da Sxz - Db Syz - Dc Sz: D times the residual sum of squares of the fit set to its least-squares plane, Dc the intercept's
// determinant (the third column of the normal equations replaced).  IN 64 BITS, by these bounds at L = 8, K = 63: |Sx|, |Sy| <= 17 * 36 =
// 612 < 2^10, Sxx, Syy, |Sxy| < 2^13, |Sz| < 2^15, |Sxz|, |Syz| < 2^17, Szz < 2^21.  The three terms of Dc: |Sxx (Syy Sz - Sy Syz)| <
// 2^13 (2^28 + 2^27) < 2^42, |Sxy (Sxy Sz - Sx Syz)| < 2^42 likewise, |Sxz (Sxy Sy - Syy Sx)| < 2^17 * 2^24 = 2^41: |Dc| < 2^44.  The four
// products: D Szz < 2^34 * 2^21 = 2^55, |Da Sxz|, |Db Syz| < 2^41 * 2^17 = 2^58, |Dc Sz| < 2^44 * 2^15 = 2^59; their absolute values sum
// to less than 2^61, so no partial sum leaves 63 bits.  In exact arithmetic 0 <= Q <= D Szz < 2^55.
KICP_HD int64_t elev_rough_residual(const ElevFitSums &s, int64_t d, int64_t da, int64_t db, int64_t &dc) {
    const int64_t sx = s.sx, sy = s.sy, sxx = s.sxx, sxy = s.sxy, syy = s.syy, sz = s.sz, sxz = s.sxz, syz = s.syz;
    dc = sxx * (syy * sz - sy * syz) - sxy * (sxy * sz - sx * syz) + sxz * (sxy * sy - syy * sx);
    return d * static_cast<int64_t>(s.szz) - da * sxz - db * syz - dc * sz;
}
// ROUGH of a cell that has a fit: Q den > num n D, strictly, on exact integers: the left side reaches 2^71 - a 128-bit product -, the
// right stays below 2^16 * 2^9 * 2^34 = 2^59.  No division, no floating point.
KICP_HD bool elev_rough_exceeds(int64_t q, int64_t d, int32_t n, const ElevRoughParams &p) {
    typedef unsigned __int128 u128;
    return static_cast<u128>(static_cast<uint64_t>(q)) * p.den > static_cast<u128>(static_cast<uint64_t>(p.num) * static_cast<uint64_t>(n) * static_cast<uint64_t>(d));
}

// ---- carving along the frame's rays (kicp_elev_update*) --------------------------------------------------------------------------
constexpr uint32_t kElevMaxWiden = 64;                     // widen_slabs
constexpr double kElevSlabMin = -32768.0, kElevSlabMax = 32767.0;  // the slabs a ray may start or end in

struct ElevCarveParams {
    uint32_t margin_steps, widen_slabs, keep_ground;  // G, W (0 .. 64), 0 or 1
};
// The carve's constants of a frame: the sensor's slab, and whether it lies in range - out of range (a NaN too) carves nothing.
struct ElevCarveFrame {
    int32_t ss;
    bool carves;
};
inline ElevCarveFrame elev_carve_frame(const ElevGeom &g, const ElevFrame &f, const double sensor_xyz[3]) {
    const double s = floor((grid_world(f.r2, f.t2, sensor_xyz[0], sensor_xyz[1], sensor_xyz[2]) - g.z_origin) / g.slab);
    const bool ok = s >= kElevSlabMin && s <= kElevSlabMax;
    return ElevCarveFrame{ok ? static_cast<int32_t>(s) : 0, ok};
}
// Is the point ELIGIBLE - its class not SKIPPED and -32768 <= s <= 32767, on doubles - and if so where does its ray end: the endpoint
// cell relative to the sensor's (|dx|, |dy| <= reach) and the endpoint's slab.
KICP_HD bool elev_carve_point(const ElevGeom &g, const ElevFrame &f, double px, double py, double pz, int32_t &dx, int32_t &dy, int32_t &es) {
    double cx, cy, wz;
    if (!elev_locate(g, f, px, py, pz, cx, cy, wz)) return false;
    const double s = floor((wz - g.z_origin) / g.slab);
    if (!(s >= kElevSlabMin && s <= kElevSlabMax)) return false;
    dx = static_cast<int32_t>(cx - f.plane.sx), dy = static_cast<int32_t>(cy - f.plane.sy), es = static_cast<int32_t>(s);
    return true;
}
// the steps a ray of length m takes: k = 0 .. m - 1 - G
KICP_HD uint32_t elev_carve_steps(uint32_t m, uint32_t margin_steps) { return m > margin_steps ? m - margin_steps : 0u; }
// The slab of the ray at parameter j / (2 m), 0 <= j <= 2 m, m >= 1: u(0) = ss, u(2 m) = es.  An integer division of non-negative
// numbers; j |d| + m < 2^29 for j <= 8191 and |d| <= 65535.
KICP_HD int32_t elev_ray_slab(int32_t ss, int32_t es, uint32_t m, uint32_t j) {
    const int32_t d = es - ss;
    const uint32_t a = static_cast<uint32_t>(d < 0 ? -d : d);
    const int32_t q = static_cast<int32_t>((j * a + m) / (2u * m));
    return d < 0 ? ss - q : ss + q;
}
// bits max(lo, 0) .. min(hi, 63) of a column, lo <= hi; empty when the span lies wholly outside it.  No shift reaches 64.
KICP_HD uint64_t elev_span_mask(int32_t lo, int32_t hi) {
    if (hi < 0 || lo > 63) return 0ull;
    const uint32_t first = lo < 0 ? 0u : static_cast<uint32_t>(lo), past = hi >= 63 ? kElevSlabs : static_cast<uint32_t>(hi) + 1u;
    return elev_bits_from(first) & ~elev_bits_from(past);
}
// the mask of step k of that ray: the slabs between parameters (2 k - 1) / (2 m) and (2 k + 1) / (2 m), widened by W on both sides
KICP_HD uint64_t elev_step_mask(int32_t ss, int32_t es, uint32_t m, uint32_t k, uint32_t widen_slabs) {
    const int32_t a = elev_ray_slab(ss, es, m, k ? 2u * k - 1u : 0u), b = elev_ray_slab(ss, es, m, 2u * k + 1u);
    const int32_t w = static_cast<int32_t>(widen_slabs);
    return elev_span_mask((a < b ? a : b) - w, (a < b ? b : a) + w);
}
// what a mask clears of a column: with keep_ground everything but the column's lowest set bit
KICP_HD uint64_t elev_clear_mask(uint64_t column, uint64_t mask, uint32_t keep_ground) {
    return keep_ground ? mask & ~(column & (~column + 1ull)) : mask;
}

namespace elev_host {
// The carve of one frame on the host, as k_elev_list and k_elev_carve do it.  Masks are applied one by one: with keep_ground the lowest
// set bit of a column never changes, so that equals clearing the OR of all masks at once.  stats[0 .. 3): carve_points, bits_cleared,
// cells_emptied.
inline void carve(const ElevGeom &g, uint64_t *columns, const double *xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                  const ElevCarveParams &p, unsigned long long stats[3]) {
    const ElevFrame f = elev_frame(g, pose_qt, sensor_xyz);
    const ElevCarveFrame cf = elev_carve_frame(g, f, sensor_xyz);
    stats[0] = stats[1] = stats[2] = 0;
    if (!cf.carves) return;
    for (size_t i = 0; i < n; ++i) {
        int32_t dx, dy, es;
        if (!elev_carve_point(g, f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], dx, dy, es)) continue;
        ++stats[0];
        const uint32_t m = grid_walk_length(dx, dy), steps = elev_carve_steps(m, p.margin_steps);
        for (uint32_t k = 0; k < steps; ++k) {
            int32_t ox, oy;
            grid_step(dx, dy, m, k, ox, oy);
            size_t c;
            if (!grid_inside(g.plane, f.plane, static_cast<uint32_t>(ox + g.plane.reach), static_cast<uint32_t>(oy + g.plane.reach), c)) continue;
            const uint64_t clear = columns[c] & elev_clear_mask(columns[c], elev_step_mask(cf.ss, es, m, k, p.widen_slabs), p.keep_ground);
            if (!clear) continue;
            stats[1] += static_cast<unsigned long long>(__builtin_popcountll(clear));
            columns[c] &= ~clear;
            if (!columns[c]) ++stats[2];
        }
    }
}
// One frame on the host, as k_elev_mark does it.  columns: one 64-bit word per cell.  stats: used, skipped, outside_grid,
// outside_column, new_bits, new_cells.
inline void integrate(const ElevGeom &g, uint64_t *columns, const double *xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                      unsigned long long stats[6]) {
    const ElevFrame f = elev_frame(g, pose_qt, sensor_xyz);
    for (int k = 0; k < 6; ++k) stats[k] = 0;
    for (size_t i = 0; i < n; ++i) {
        size_t c = 0;
        uint32_t s = 0;
        switch (elev_point(g, f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], c, s)) {
            case kElevSkipped: ++stats[1]; break;
            case kElevOutsideGrid: ++stats[2]; break;
            case kElevOutsideColumn: ++stats[3]; break;
            case kElevUsed: {
                ++stats[0];
                const uint64_t bit = 1ull << s;
                if (!(columns[c] & bit)) ++stats[4];
                if (!columns[c]) ++stats[5];
                columns[c] |= bit;
            }
        }
    }
}
// An UPDATE: the carve, then the mark - a frame's own returns survive it.  stats: integrate's six, counted relative to the carved
// columns, then carve's three.
inline void update(const ElevGeom &g, uint64_t *columns, const double *xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                   const ElevCarveParams &p, unsigned long long stats[9]) {
    carve(g, columns, xyz, n, pose_qt, sensor_xyz, p, stats + 6);
    integrate(g, columns, xyz, n, pose_qt, sensor_xyz, stats);
}
// The classes of a rectangle (inside the grid; checked by the caller), as k_elev_classify computes them: out and ground (nullable) are
// h * w values, row-major from (x0, y0); counts (nullable): unknown, traversable, BODY, STEP only.
inline void classify(const uint64_t *columns, uint32_t width, uint32_t height, const ElevParams &p, const ElevRect &r, int8_t *out, uint8_t *ground,
                     unsigned long long counts[4]) {
    unsigned long long sums[4] = {0, 0, 0, 0};
    for (uint32_t ry = 0; ry < r.h; ++ry)
        for (uint32_t rx = 0; rx < r.w; ++rx) {
            const uint32_t x = r.x0 + rx, y = r.y0 + ry;
            const uint64_t c = columns[static_cast<size_t>(y) * width + x];
            const uint8_t gr = elev_ground(c);
            bool body = false, step = false;
            if (c) {
                body = elev_body(c, gr, p);
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int64_t nx = static_cast<int64_t>(x) + dx, ny = static_cast<int64_t>(y) + dy;
                        if ((dx == 0 && dy == 0) || nx < 0 || ny < 0 || nx >= static_cast<int64_t>(width) || ny >= static_cast<int64_t>(height)) continue;
                        step = step || elev_step(gr, elev_ground(columns[static_cast<size_t>(ny) * width + static_cast<size_t>(nx)]), p);
                    }
            }
            uint32_t which;
            const size_t o = static_cast<size_t>(ry) * r.w + rx;
            out[o] = elev_value(which, c != 0ull, body, step);
            if (ground) ground[o] = gr;
            ++sums[which];
        }
    if (counts)
        for (int k = 0; k < 4; ++k) counts[k] = sums[k];
}
// The same with a plane fit, as k_elev_fit<L, Rough> computes it: the slope limit and, with Rough, the class ROUGH.  fit (nullable) takes
// kElevFitValues<Rough> values per cell - D, Da, Db, with Rough also Q, n -, zeros where the cell has no fit; counts (nullable):
// kElevFitCounts<Rough> words - unknown, traversable, BODY, STEP only, SLOPE only, with Rough also ROUGH only.  rp is read with Rough only.
template <bool Rough>
inline void classify_fit(const uint64_t *columns, uint32_t width, uint32_t height, const ElevParams &p, const ElevSlopeParams &sp, const ElevRoughParams &rp,
                         const ElevRect &r, int8_t *out, uint8_t *ground, long long *fit, unsigned long long *counts) {
    constexpr uint32_t values = kElevFitValues<Rough>;
    unsigned long long sums[kElevFitCounts<Rough>] = {};
    const int32_t L = static_cast<int32_t>(sp.radius);
    for (uint32_t ry = 0; ry < r.h; ++ry)
        for (uint32_t rx = 0; rx < r.w; ++rx) {
            const uint32_t x = r.x0 + rx, y = r.y0 + ry;
            const uint64_t c = columns[static_cast<size_t>(y) * width + x];
            const uint8_t gr = elev_ground(c);
            bool body = false, step = false, slope = false, rough = false;
            int64_t v[5] = {0, 0, 0, 0, 0};  // D, Da, Db, Q, n
            if (c) {
                body = elev_body(c, gr, p);
                ElevFitSums s{};
                for (int32_t dy = -L; dy <= L; ++dy)
                    for (int32_t dx = -L; dx <= L; ++dx) {
                        const int64_t nx = static_cast<int64_t>(x) + dx, ny = static_cast<int64_t>(y) + dy;
                        if (nx < 0 || ny < 0 || nx >= static_cast<int64_t>(width) || ny >= static_cast<int64_t>(height)) continue;
                        const uint8_t gn = elev_ground(columns[static_cast<size_t>(ny) * width + static_cast<size_t>(nx)]);
                        elev_fit_add<Rough>(s, gr, gn, dx, dy, sp.gate);
                        if ((dx || dy) && dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) step = step || elev_step(gr, gn, p);
                    }
                elev_slope_determinants(s, v[0], v[1], v[2]);
                if (elev_slope_has_fit(s, v[0], sp)) {
                    slope = elev_slope_exceeds(v[0], v[1], v[2], sp);
                    if constexpr (Rough) {
                        int64_t dc;
                        v[3] = elev_rough_residual(s, v[0], v[1], v[2], dc), v[4] = s.n;
                        rough = elev_rough_exceeds(v[3], v[0], s.n, rp);
                    }
                } else {
                    v[0] = v[1] = v[2] = 0;
                }
            }
            uint32_t which;
            const size_t o = static_cast<size_t>(ry) * r.w + rx;
            out[o] = elev_value(which, c != 0ull, body, step, slope, rough);
            if (ground) ground[o] = gr;
            if (fit)
                for (uint32_t k = 0; k < values; ++k) fit[values * o + k] = v[k];
            ++sums[which];
        }
    if (counts)
        for (uint32_t k = 0; k < kElevFitCounts<Rough>; ++k) counts[k] = sums[k];
}
// the two names the stand-alone programs call
inline void classify_slope(const uint64_t *columns, uint32_t width, uint32_t height, const ElevParams &p, const ElevSlopeParams &sp, const ElevRect &r, int8_t *out,
                           uint8_t *ground, long long *fit, unsigned long long counts[5]) {
    classify_fit<false>(columns, width, height, p, sp, ElevRoughParams{}, r, out, ground, fit, counts);
}
inline void classify_rough(const uint64_t *columns, uint32_t width, uint32_t height, const ElevParams &p, const ElevSlopeParams &sp, const ElevRoughParams &rp,
                           const ElevRect &r, int8_t *out, uint8_t *ground, long long *fit, unsigned long long counts[6]) {
    classify_fit<true>(columns, width, height, p, sp, rp, r, out, ground, fit, counts);
}
}  // namespace elev_host

}  // namespace kicp
