// kicp_pass_fixed.hpp -- the exact accumulation of the pass kernels and the per-correspondence terms that go into it: every term is
// rounded once to a multiple of 2^-40 (to_fixed, terms_to_fixed) and added as a 128-bit integer (I128), so the sums do not depend on
// summation order, kernel variant, binning order or the number of GPUs.  What a lane keeps of a correspondence (Acc, ScoreAcc, PlanarAcc)
// and the terms themselves (correspondence_terms, accumulate) are here too: one function for every pass kernel, the same doubles.
// to_fixed, terms_to_fixed, basis_of and set_pose are __host__ __device__: the host forms the basis it sends, and tests/cpp runs them.
#pragma once
#include "kicp_common.hpp"
#include "kicp_pass_params.hpp"
#include "kicp_se3.hpp"

namespace kicp {

// ------------------------------------------------------------------------------------------------------------
// exact accumulation
// ------------------------------------------------------------------------------------------------------------
struct I128 {
    unsigned long long lo;
    long long hi;
};
__device__ __forceinline__ void i128_add(I128 &a, const I128 &b) {
    const unsigned long long old = a.lo;
    a.lo += b.lo;
    a.hi += b.hi + (a.lo < old ? 1 : 0);
}
// T = l0 + l1*2^40 + l2*2^80 with 0 <= l0,l1 < 2^40, l2 signed
__device__ __forceinline__ void i128_to_limbs(const I128 &t, long long l[3]) {
    const unsigned long long m40 = (1ull << 40) - 1;
    l[0] = static_cast<long long>(t.lo & m40);
    l[1] = static_cast<long long>(((t.lo >> 40) | (static_cast<unsigned long long>(t.hi) << 24)) & m40);
    l[2] = t.hi >> 16;
}
__device__ __forceinline__ double limbs_to_double(const long long l[3]) {
    // recombine (limb sums may exceed 40 bits and be negative), then convert the 128-bit magnitude
    I128 t{static_cast<unsigned long long>(l[0]), l[0] >> 63};
    I128 a{static_cast<unsigned long long>(l[1]) << 40, l[1] >> 24};
    I128 b{0ull, static_cast<long long>(static_cast<unsigned long long>(l[2]) << 16)};
    i128_add(t, a), i128_add(t, b);
    const bool neg = t.hi < 0;
    if (neg) {
        t.lo = ~t.lo + 1ull;
        t.hi = ~t.hi + (t.lo == 0ull ? 1 : 0);
    }
    const double mag = static_cast<double>(static_cast<unsigned long long>(t.hi)) * 18446744073709551616.0 + static_cast<double>(t.lo);
    return (neg ? -mag : mag) / kFixScale;
}

// A lane's contribution to the seven sums of one pass: every lane serves at most ONE correspondence per block of queries (tile),
// so per tile each sum is a single fixed-point term x * 2^40 with |x| < 2^43, held as four 21-bit limbs (the top one signed).  A
// lane adds its limbs over the at most kMaxPassTiles tiles of its workgroup (pass_tiles_loop), and a wave's 64 values of a limb
// then add up in int32 (finish_pass): 4 * 64 * 2^21 = 2^29.  The term is formed without leaving the integers' range: x = ip + fr with
// ip = rint(x) (exact in int64) and fr = x - ip (exact, |fr| <= 1/2), so round(x * 2^40) = ip * 2^40 + round(fr * 2^40)
// - the same integer the single conversion gives wherever that one fits (ties included: ip * 2^40 is even).
constexpr int kTermLimbs = 4;
constexpr int kWaveLimbs = kTermLimbs * kNumSums;
// what a lane keeps of an accepted correspondence (resolve_and_accumulate): the seven terms of a registration pass, the squared
// residual alone, or the terms of the planar 3-DoF normal equations
enum class AccKind { Pass, Score, Planar };
struct Acc {
    static constexpr AccKind kKind = AccKind::Pass;
    int limb[kWaveLimbs];
    int range_error;
};
// What kicp_score_poses keeps of a correspondence (kicp_score.hpp): the squared residual - the term of sum 5, through the same
// to_fixed - and the fact that there is one.  No basis, no Jacobian terms, no 28-limb row.
struct ScoreAcc {
    static constexpr AccKind kKind = AccKind::Score;
    int limb[kTermLimbs];  // to_fixed(|T s - nn|^2)
    int hit;               // 1: this lane holds a correspondence
    int range_error;
};
// What kicp_planar_sums keeps (kicp_planar.hpp): the terms of the normal equations of a step that is free in the plane (x, y, yaw in
// the body frame) - s.x, -s.y, s.x^2 + s.y^2, a = c0 . r, b = c1 . r, s.x b - s.y a, |r|^2, in this order, each through to_fixed.  Five
// of them are the pass kernels' terms (correspondence_terms: the same doubles); s.x and b are the two a pass does not sum.
constexpr int kPlanarTerms = 7;
struct PlanarAcc {
    static constexpr AccKind kKind = AccKind::Planar;
    int limb[kTermLimbs * kPlanarTerms];
    int hit;  // 1: this lane holds a correspondence
    int range_error;
};
// The term as an integer, T = rint(x 2^40) (|T| < 2^83; x 2^40 is exact, rint of a double beyond 2^52 is the double itself), split
// into four SIGNED limbs of 21 bits by truncating divisions carried out in fp64 - every step exact: q = trunc(t 2^-k) and
// t - q 2^k = fma(q, -2^k, t) are representable (the remainder keeps t's granularity and is shorter than t).
//   T = l0 + l1 2^21 + l2 2^42 + l3 2^63,  |lk| < 2^21, every limb with T's sign
// (round 4 built the same integer from two 64-bit conversions and split it with 128-bit integer arithmetic: ~30 instructions
// against ~18; the limbs were non-negative below the top one - any split of the same integer adds up to the same sums).
KICP_HD void to_fixed(double x, int *limb, int &range_error) {
    const bool ok = fabs(x) < kFixLimit;
    if (!ok) range_error = 1;
    const double t = rint((ok ? x : 0.0) * kFixScale);
    const double q3 = trunc(t * 0x1p-63);
    const double r3 = fma(q3, -0x1p63, t);
    const double q2 = trunc(r3 * 0x1p-42);
    const double r2 = fma(q2, -0x1p42, r3);
    const double q1 = trunc(r2 * 0x1p-21);
    const double r1 = fma(q1, -0x1p21, r2);
    limb[0] = static_cast<int>(r1), limb[1] = static_cast<int>(q1), limb[2] = static_cast<int>(q2), limb[3] = static_cast<int>(q3);
}
// The five terms of a correspondence (correspondence_terms) into limb[0 .. 5 kTermLimbs): the limbs and the range flag of five to_fixed
// calls, bit for bit.  Where all five are below 2^22 in magnitude - every term of a scan whose points lie within 2 048 m of the base
// frame - the integer T = rint(x 2^40) is at most 2^62 in magnitude, so to_fixed's q3 = trunc(T 2^-63) is +-0, its r3 is T itself and
// its range test cannot fail: the short path leaves out the top limb's division, the range selects and the flag, and writes 0 for the
// limb (static_cast<int>(-0.0) is 0 too).  The five compares are false for a NaN, which therefore takes to_fixed and raises the flag
// there.  A lane's branch: a wave whose lanes all take the short side skips the general one with scalar instructions alone.
constexpr double kShortTermLimit = 0x1p22;
KICP_HD bool terms_are_short(const double (&term)[5]) {
    bool is_short = true;
#pragma unroll
    for (int i = 0; i < 5; ++i) is_short = is_short && fabs(term[i]) < kShortTermLimit;
    return is_short;
}
KICP_HD void terms_to_fixed(const double (&term)[5], int *limb, int &range_error) {
    if (terms_are_short(term)) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double t = rint(term[i] * kFixScale);
            const double q2 = trunc(t * 0x1p-42);
            const double r2 = fma(q2, -0x1p42, t);
            const double q1 = trunc(r2 * 0x1p-21);
            const double r1 = fma(q1, -0x1p21, r2);
            int *l = limb + i * kTermLimbs;
            l[0] = static_cast<int>(r1), l[1] = static_cast<int>(q1), l[2] = static_cast<int>(q2), l[3] = 0;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 5; ++i) to_fixed(term[i], limb + i * kTermLimbs, range_error);
    }
}
KICP_HD PassBasis basis_of(const Pose &T) {
    PassBasis b;
    quat_rotate(T, 1.0, 0.0, 0.0, b.c0x, b.c0y, b.c0z);  // J.col(0) = R * UnitX (Registration.cpp:90)
    quat_rotate(T, 0.0, 1.0, 0.0, b.c1x, b.c1y, b.c1z);
    int range_error = 0;  // (|c0|^2 is 1 to rounding for a unit quaternion; a NaN pose leaves zeros - its passes add nothing)
    to_fixed(b.c0x * b.c0x + b.c0y * b.c0y + b.c0z * b.c0z, b.jtj00, range_error);
    return b;
}
KICP_HD void set_pose(SolveParams &f, const Pose &T) { f.pose0 = T, f.basis = basis_of(T); }
// the 128-bit sum of one term's limb sums s[0..3] (each a sum of at most 2^10 limbs)
__device__ __forceinline__ void i128_add_limb_sums(I128 &t, long long s0, long long s1, long long s2, long long s3) {
    const long long low = s0 + s1 * 2097152ll;  // |.| < 2^53 (limb sums are signed)
    i128_add(t, I128{static_cast<unsigned long long>(low), low >> 63});
    i128_add(t, I128{static_cast<unsigned long long>(s2) << 42, s2 >> 22});
    i128_add(t, I128{static_cast<unsigned long long>(s3) << 63, s3 >> 1});
}
// (kMaxPassTiles and limb_sums_to_words - a workgroup's limb sums as row words - live in kicp_pass_tiles.hpp, which a host program can include)

// ------------------------------------------------------------------------------------------------------------
// per-correspondence terms (Registration.cpp:86-93,108-113)
// ------------------------------------------------------------------------------------------------------------
// The reference forms J = [R UnitX | R (-s.y, s.x, 0)] and r = T s - t per correspondence and adds J^T J and J^T r.  With R
// orthogonal those products have a closed form, which is what is evaluated here:
//   JTJ(0,0) = |c0|^2 (the pose's alone: PassBasis::jtj00)     JTJ(0,1) = -s.y     JTJ(1,1) = s.x^2 + s.y^2
//   JTr(0)   = c0 . r                                           JTr(1)   = s.x (c1 . r) - s.y (c0 . r)
// It differs from the literal products by their own rounding (a few 1e-16 relative: tests/test_closed_form.py holds the two to
// 1e-12 on random data, the parity suite holds the sums and poses to the oracle's, which keeps the literal form); nothing here
// takes part in a decision - every term is rounded to 2^-40 right afterwards - so the multiply-adds are fused.
// One function for every pass kernel: their terms are the same doubles.
// |r|^2 of a residual, the term of sum 5: ONE expression for the pass kernels and for k_score_poses (kicp_score.hpp)
__device__ __forceinline__ double squared_residual(double rx, double ry, double rz) { return fma(rx, rx, fma(ry, ry, rz * rz)); }
// `b` = c1 . r leaves the function too: the planar sums (PlanarAcc) add it up, a pass only uses it inside term[3]
__device__ __forceinline__ void correspondence_terms(const PassBasis &B, double sx, double sy, double qx, double qy, double qz, double tx, double ty, double tz,
                                                     double (&term)[5], double &b) {
    const double rx = qx - tx, ry = qy - ty, rz = qz - tz;  // residual = T*source - target (Registration.cpp:88)
    const double a = fma(B.c0x, rx, fma(B.c0y, ry, B.c0z * rz));
    b = fma(B.c1x, rx, fma(B.c1y, ry, B.c1z * rz));
    term[0] = -sy;
    term[1] = fma(sx, sx, sy * sy);
    term[2] = a;
    term[3] = fma(sx, b, -(sy * a));
    term[4] = squared_residual(rx, ry, rz);
}
__device__ __forceinline__ void correspondence_terms(const PassBasis &B, double sx, double sy, double qx, double qy, double qz, double tx, double ty, double tz,
                                                     double (&term)[5]) {
    double b;
    correspondence_terms(B, sx, sy, qx, qy, qz, tx, ty, tz, term, b);
}
// the same residual as correspondence_terms forms it, and nothing else (kicp_score_poses)
__device__ __forceinline__ void accumulate(ScoreAcc &a, double qx, double qy, double qz, double tx, double ty, double tz) {
    const double rx = qx - tx, ry = qy - ty, rz = qz - tz;
    to_fixed(squared_residual(rx, ry, rz), a.limb, a.range_error);
    a.hit = 1;
}
// SHORT: the terms go through terms_to_fixed and its short path.  Not in the EXPORT twins: the second path's live ranges cost the split
// one (k_pass_gather32<256, 2, 4, true, false, true>) two vector registers it does not have - it spilled - and nobody times them.
// (Like query_from's COMPONENTS this parameter only keeps an untimed kernel's registers where they were; it can go when that twin has two to spare.)
template <bool SHORT>
__device__ __forceinline__ void accumulate(Acc &a, const PassBasis &B, double sx, double sy, double qx, double qy, double qz, double tx, double ty, double tz) {
    double term[5];
    correspondence_terms(B, sx, sy, qx, qy, qz, tx, ty, tz, term);
#pragma unroll
    for (int k = 0; k < kTermLimbs; ++k) a.limb[k] = B.jtj00[k];
    if constexpr (SHORT) {
        terms_to_fixed(term, a.limb + kTermLimbs, a.range_error);
    } else {
#pragma unroll
        for (int i = 0; i < 5; ++i) to_fixed(term[i], a.limb + (i + 1) * kTermLimbs, a.range_error);
    }
    a.limb[6 * kTermLimbs + 1] = 1 << 19;  // the count: 1.0 = 2^40 = 2^19 * 2^21 (the other limbs stay 0)
}
// the pass kernels' terms from their own function, s.x and b next to them (kicp_planar_sums)
__device__ __forceinline__ void accumulate(PlanarAcc &a, const PassBasis &B, double sx, double sy, double qx, double qy, double qz, double tx, double ty, double tz) {
    double term[5], b;
    correspondence_terms(B, sx, sy, qx, qy, qz, tx, ty, tz, term, b);
    to_fixed(sx, a.limb, a.range_error);
    to_fixed(term[0], a.limb + 1 * kTermLimbs, a.range_error);
    to_fixed(term[1], a.limb + 2 * kTermLimbs, a.range_error);
    to_fixed(term[2], a.limb + 3 * kTermLimbs, a.range_error);
    to_fixed(b, a.limb + 4 * kTermLimbs, a.range_error);
    to_fixed(term[3], a.limb + 5 * kTermLimbs, a.range_error);
    to_fixed(term[4], a.limb + 6 * kTermLimbs, a.range_error);
    a.hit = 1;
}

}  // namespace kicp
