// PointToVoxel without a division (kicp_pass_visit.hpp::voxel_coord, voxel_coord_offset) on the HOST - the functions are __host__
// __device__, the device runs the same operations.  For voxel sizes 1, 0.5, 0.3, 0.1 and 0.05, at coordinates k vs -+ j ulps (j = 0 .. 4;
// k = 0, +-1, ... +-2^20), at random coordinates, at fractions on either side of the guard and at |c / vs| just below 2^31:
//   * voxel_coord and voxel_coord_offset give the integer of the formula they replaced, kept below as text (parent_voxel_coord), and
//     of the reference's static_cast<int>(floor(c / vs)) wherever that formula did;
//   * the offset inside the voxel, in mirror units, differs from (c - v vs) upm evaluated in long double by less than the bound stated
//     above start_lane - 0.004 for the fp32 rounding plus 1.5e-5 for the two roundings of c (1 / vs) - wherever |c / vs| <= 2^20;
//   * 0 <= offset < 65536 everywhere.
// Built by tests/test_voxel_coord.py with `hipcc --cuda-host-only` and the host's address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

#include "kicp_pass_visit.hpp"

using namespace kicp;

// the formula before the constant guard: a guard relative to |t|
static int32_t parent_voxel_coord(double c, double vs, double inv_vs) {
    const double t = c * inv_vs;
    const double f = floor(t);
    const double frac = t - f;
    const double guard = 4.0e-16 * fabs(t) + 1.0e-300;
    if (frac < guard || 1.0 - frac < guard) return static_cast<int32_t>(floor(c / vs));
    return static_cast<int32_t>(f);
}

static long bad = 0, checked = 0, divided = 0, divided_only_now = 0, bounded = 0;
static double worst = 0.0;
constexpr double kOffsetBound = 0.004 + 1.5e-5;  // units, |c / vs| <= 2^20

static void check(double c, double vs) {
    const double inv_vs = 1.0 / vs, upm = mirror_units_per_metre(vs);
    const int32_t want = parent_voxel_coord(c, vs, inv_vs);
    const int32_t v = voxel_coord(c, vs, inv_vs);
    const VoxelCoord vo = voxel_coord_offset(c, vs, inv_vs, upm);
    ++checked;
    if (v != want || vo.v != want) ++bad, std::printf("voxel: c %a vs %a -> %d / %d, the parent's formula %d\n", c, vs, v, vo.v, want);
    if (want != static_cast<int32_t>(floor(c / vs))) ++bad, std::printf("reference: c %a vs %a -> %d\n", c, vs, want);
    const double t = c * inv_vs, frac = t - floor(t);
    if (!voxel_frac_is_safe(frac)) {
        ++divided;
        const double guard = 4.0e-16 * fabs(t) + 1.0e-300;
        if (!(frac < guard || 1.0 - frac < guard)) ++divided_only_now;
    }
    if (!(vo.off >= 0.f && vo.off < 65536.f)) ++bad, std::printf("range: c %a vs %a -> offset %a\n", c, vs, vo.off);
    if (fabs(t) <= 1048576.0) {
        const long double exact = (static_cast<long double>(c) - static_cast<long double>(vo.v) * static_cast<long double>(vs)) * static_cast<long double>(upm);
        const double err = static_cast<double>(fabsl(static_cast<long double>(vo.off) - exact));
        ++bounded;
        if (err > worst) worst = err;
        if (!(err < kOffsetBound)) ++bad, std::printf("offset: c %a vs %a -> %a, exact %La (off by %g)\n", c, vs, vo.off, exact, err);
    }
}

static void around(double c, double vs) {  // c and its four neighbours on either side
    double up = c, down = c;
    check(c, vs);
    for (int j = 1; j <= 4; ++j) {
        up = nextafter(up, INFINITY), down = nextafter(down, -INFINITY);
        check(up, vs), check(down, vs);
    }
}

int main() {
    const double sizes[5] = {1.0, 0.5, 0.3, 0.1, 0.05};
    std::mt19937_64 rng(20261020u);
    for (double vs : sizes) {
        // voxel faces: small k one by one, powers of two and their neighbours up to 2^20, random k in between
        for (int64_t k = -300; k <= 300; ++k) around(static_cast<double>(k) * vs, vs);
        for (int e = 8; e <= 20; ++e)
            for (int64_t d = -2; d <= 2; ++d) {
                const int64_t k = (int64_t{1} << e) + d;
                if (k <= 1048576) around(static_cast<double>(k) * vs, vs);
                if (-k >= -1048576) around(static_cast<double>(-k) * vs, vs);
            }
        std::uniform_int_distribution<int64_t> face(-1048576, 1048576);
        for (int r = 0; r < 20000; ++r) around(static_cast<double>(face(rng)) * vs, vs);
        // either side of the constant guard (1e-6 of a voxel from a face), inside a voxel, mid-voxel
        const double fractions[10] = {0.9e-6, 1.1e-6, 1.0 - 0.9e-6, 1.0 - 1.1e-6, 2.0e-7, 1.0 - 2.0e-7, 0.5, 0.25, 1.0e-3, 1.0 - 1.0e-3};
        for (int r = 0; r < 4000; ++r) {
            const double k = static_cast<double>(face(rng) / (r % 2 ? 1 : 4096));
            for (double f : fractions) check((k + f) * vs, vs);
        }
        // random coordinates: a room, a site, the whole range of the lane offsets' bound
        const double spans[3] = {10.0, 1000.0, 1048575.0 * vs};
        for (double span : spans) {
            std::uniform_real_distribution<double> any(-span, span);
            for (int r = 0; r < 60000; ++r) check(any(rng), vs);
        }
        // |c / vs| just below 2^31: the guard must still cover the old one, the conversion is still in range
        for (int64_t d = 2; d <= 6; ++d) {
            around(static_cast<double>(2147483648LL - d) * vs, vs);
            around(static_cast<double>(-2147483648LL + d) * vs, vs);
            check((static_cast<double>(2147483648LL - d) + 0.5) * vs, vs);
            check((static_cast<double>(-2147483648LL + d) + 0.5) * vs, vs);
        }
    }
    std::printf("voxel coord: %ld checked, %ld by division (%ld of them inside the new guard alone), %ld offsets held to %g units, worst %g\n", checked, divided,
                divided_only_now, bounded, kOffsetBound, worst);
    if (divided < 1000 || divided_only_now < 1000 || bounded < 1000000) ++bad, std::printf("the cases do not enter the regimes they were built for\n");
    std::printf("voxel coord: %ld bad\n", bad);
    return bad ? 1 : 0;
}
