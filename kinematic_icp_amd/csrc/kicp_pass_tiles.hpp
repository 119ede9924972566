// kicp_pass_tiles.hpp -- what the tiles of the four-waves pass kernel rest on, free of HIP so that a stand-alone C++ program can
// check it on the host (tests/cpp/pass_tiles_test.cpp): the row words of a workgroup's limb sums, and the automatic tile count.
//
// A workgroup of the one-lane-per-query four-waves build searches `tiles` blocks of 256 queries and runs ONE epilogue
// (kicp_kernels.hpp: pass_tiles_loop; kicp_pass_finish.hpp: finish_pass).  The sums are exact integers, so the tile count changes no bit of a result -
// only how often the epilogue's fixed cost is paid, and how many workgroups a pass has.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define KICP_TILES_HD __host__ __device__ __forceinline__
#else
#define KICP_TILES_HD inline
#endif

namespace kicp {
// Tiles of 256 queries one workgroup may serve before its one epilogue (PassParams::tiles).  Four is what the limb sums allow: a
// limb is below 2^21 in magnitude, so a lane's sum over 4 tiles and a wave's 64 lanes stay below 2^29 (int32, finish_pass), and
// the workgroup's 1024 terms below 2^31 - the bound limb_sums_to_words' row words rest on.
constexpr int kMaxPassTiles = 4;
// The three row words of one term from a WORKGROUP's four limb sums, in 64-bit arithmetic only: any w with
//   w0 + w1 2^40 + w2 2^80 = s0 + s1 2^21 + s2 2^42 + s3 2^63   and   |w| < 2^40
// serves - the group's accumulator and the host add words, and the host recombines the sums exactly (limbs_to_double), so the
// words need not be the canonical limbs of the 128-bit total.  With |s| < 2^31 (at most kMaxPassTiles * 256 terms of |limb| < 2^21):
//   low = s0 + s1 2^21               |low| < 2^31 + 2^52 < 2^53
//   s3  = s3h 2^17 + s3l             s3l in [-2^16, 2^16), |s3h| <= 2^14          (2^63 = 2^23 2^40 = 2^80 / 2^17)
//   w0  = low mod 2^40               in [0, 2^40)
//   w1  = floor(low / 2^40) + 4 s2 + s3l 2^23        |w1| <= 2^13 + 2^33 + 2^39 < 2^40
//   w2  = s3h                        |w2| <= 2^14
KICP_TILES_HD void limb_sums_to_words(long long s0, long long s1, long long s2, long long s3, long long w[3]) {
    const long long low = s0 + s1 * 2097152ll;
    const long long s3h = (s3 + 65536ll) >> 17, s3l = s3 - s3h * 131072ll;
    w[0] = low & ((1ll << 40) - 1ll);
    w[1] = (low >> 40) + s2 * 4ll + s3l * 8388608ll;
    w[2] = s3h;
}

namespace host {
// The automatic tile count (option "pass_tiles" = 0) of a pass of `blocks` blocks of 256 queries while `in_flight` scans of
// that size share a device of `cus` compute units.  The four-waves build holds four workgroups per compute unit, so the device
// has 4 * cus workgroup slots.  Tiles save the epilogue's instructions, but they make a workgroup T times longer and leave T times
// fewer of them to even out the slots' loads: they pay only while the passes in flight still have well more workgroups than the
// device has slots.  Measured on MI355X (256 CUs, 1024 slots; profiles/pass_tiles_ab.txt; us per scan, in-process A/B, `x`: the
// workgroups in flight as a multiple of the slots):
//                                         T = 1          T = 2          T = 4
//   cfg2, 512 blocks, 8 in flight      5.27 (x 4.0)   4.88 (x 2.0)   5.44 (x 1.0)
//   cfg5, 1954 blocks, 8 in flight    30.62 (x 15)   28.71 (x 7.6)  27.99 (x 3.8)
//   cfg5, single calls                50.90 (x 1.9)  50.43 (x 0.95) 61.28 (x 0.48)
//   40 000 points, 8 in flight         2.53 (x 1.2)   3.04 (x 0.62)  4.17 (x 0.31)
// Every count that left at least twice the slots won, every count that left the slots or fewer lost or made no difference; nothing
// was measured in between.  The rule takes the middle: the largest T of 4, 2, 1 whose workgroups in flight are at least 1.5 times
// the slots - and 1 whenever more tiles would leave the device short of workgroups.
inline uint32_t auto_pass_tiles(size_t blocks, int in_flight, int cus) {
    const size_t slots = 4u * static_cast<size_t>(std::max(1, cus)), scans = static_cast<size_t>(std::max(1, in_flight));
    for (uint32_t t = static_cast<uint32_t>(kMaxPassTiles); t > 1u; t /= 2u)
        if (2u * ((blocks + t - 1u) / t) * scans >= 3u * slots) return t;
    return 1u;
}
// what option "pass_tiles" accepts: 0 (automatic), 1, 2, 4; anything else is clamped to the nearest of these below it
inline int clamp_pass_tiles(double value) { return value >= 4.0 ? 4 : (value >= 2.0 ? 2 : (value >= 1.0 ? 1 : 0)); }
}  // namespace host
}  // namespace kicp
