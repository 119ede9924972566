// The host-checkable parts of the pass kernel's tiles (kinematic_icp_amd/csrc/kicp_pass_tiles.hpp), on the CPU:
//  - limb_sums_to_words: for limb sums anywhere in the range a workgroup can produce (|s| < 2^31: at most 4 x 256 terms of limbs
//    below 2^21) - the corners and random values - the three words add up to s0 + s1 2^21 + s2 2^42 + s3 2^63 exactly (128-bit
//    arithmetic here), every word is below 2^40 in magnitude, and 32 biased words fit the accumulator's 56-bit field;
//  - auto_pass_tiles: 1, 2 or 4; never a count that leaves fewer than 1.5 workgroups in flight per slot; the measured rows the rule was derived from;
//  - clamp_pass_tiles: what option "pass_tiles" accepts.
// Stand-alone (own main), built with -fsanitize=address,undefined by tests/test_pass_tiles.py.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "kicp_pass_tiles.hpp"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

static void check_words(long long s0, long long s1, long long s2, long long s3) {
    long long w[3];
    kicp::limb_sums_to_words(s0, s1, s2, s3, w);
    const __int128 one = 1;  // (multiplications: the values are signed)
    const __int128 want = s0 + s1 * (one << 21) + s2 * (one << 42) + s3 * (one << 63);
    const __int128 got = w[0] + w[1] * (one << 40) + w[2] * (one << 80);
    CHECK(got == want);
    const long long bias = 1ll << 41;  // (kAccBias; the accumulator's sum field is 56 bits wide, a group has 32 workgroups)
    for (int j = 0; j < 3; ++j) {
        CHECK(w[j] > -(1ll << 40) && w[j] < (1ll << 40));
        CHECK(w[j] + bias > 0 && 32 * (w[j] + bias) < (1ll << 56));
    }
}

int main() {
    const long long top = (1ll << 31) - 1024;  // 1024 limbs of magnitude 2^21 - 1
    const long long corner[] = {-top, -(1ll << 17), -65537, -65536, -65535, -1, 0, 1, 65535, 65536, 65537, 1ll << 17, top};
    for (long long a : corner)
        for (long long b : corner)
            for (long long c : corner)
                for (long long d : corner) check_words(a, b, c, d);
    std::mt19937_64 rng(7);
    std::uniform_int_distribution<long long> any(-top, top), narrow(-70000, 70000);
    for (int i = 0; i < 2000000; ++i) check_words(any(rng), any(rng), any(rng), i % 3 ? any(rng) : narrow(rng));

    using kicp::host::auto_pass_tiles;
    for (int cus : {1, 64, 256, 304})
        for (int in_flight : {0, 1, 2, 4, 8, 16})
            for (size_t blocks = 0; blocks < 9000; blocks += (blocks < 600 ? 1 : 37)) {
                const uint32_t t = auto_pass_tiles(blocks, in_flight, cus);
                CHECK(t == 1u || t == 2u || t == 4u);
                const size_t scans = in_flight < 1 ? 1 : static_cast<size_t>(in_flight);
                const size_t slots = 4u * static_cast<size_t>(cus);
                if (t > 1u) CHECK(2u * ((blocks + t - 1) / t) * scans >= 3u * slots);  // at least 1.5 workgroups in flight per slot: never short of them
                if (t < 4u) CHECK(2u * ((blocks + 2 * t - 1) / (2 * t)) * scans < 3u * slots);  // ... and the next count would leave fewer
            }
    CHECK(auto_pass_tiles(512, 8, 256) == 2u);   // cfg2 (131 072 points), eight scans in flight
    CHECK(auto_pass_tiles(512, 1, 256) == 1u);   // ... one at a time
    CHECK(auto_pass_tiles(1954, 8, 256) == 4u);  // cfg5 (500 000 points), eight in flight
    CHECK(auto_pass_tiles(1954, 1, 256) == 1u);  // ... single calls
    CHECK(auto_pass_tiles(157, 8, 256) == 1u);   // 40 000 points, eight in flight

    using kicp::host::clamp_pass_tiles;
    CHECK(clamp_pass_tiles(-3.0) == 0 && clamp_pass_tiles(0.0) == 0 && clamp_pass_tiles(1.0) == 1 && clamp_pass_tiles(2.0) == 2);
    CHECK(clamp_pass_tiles(3.0) == 2 && clamp_pass_tiles(4.0) == 4 && clamp_pass_tiles(100.0) == 4);
    std::printf("OK\n");
    return 0;
}
