// terms_to_fixed of kicp_pass_fixed.hpp on the HOST (__host__ __device__: the device runs the same operations): the twenty limbs and the
// range flag it leaves for five terms must be those of five to_fixed calls, whichever path it takes.
//   * 0 and -0, ties of the 2^-41 grid and their neighbours, the short path's last value 2^22 - 2^-30 and its first excluded one 2^22
//     (terms_are_short says which path a set of terms takes), 2^43 - 1 and the range error at 2^43, NaN and the infinities - each of
//     them in every one of the five positions, beside small terms and beside one another;
//   * 10^5 random values for every binade from 2^-45 to 2^44, both signs, five of one binade per call;
//   * mixtures: four small terms and one large one (2^22 .. 2^44) in every position.
// Built by tests/test_terms_fixed.py with `hipcc --cuda-host-only` and the host's address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "kicp_pass_fixed.hpp"

using namespace kicp;

static long bad = 0, checked = 0, short_sets = 0, general_sets = 0, flagged = 0;

static void check(const double (&term)[5]) {
    int want[5 * kTermLimbs], got[5 * kTermLimbs], want_flag = 0, got_flag = 0;
    for (int k = 0; k < 5 * kTermLimbs; ++k) want[k] = 7, got[k] = -7;
    for (int i = 0; i < 5; ++i) to_fixed(term[i], want + i * kTermLimbs, want_flag);
    terms_to_fixed(term, got, got_flag);
    ++checked;
    bool all_below = true;
    for (int i = 0; i < 5; ++i) all_below = all_below && std::fabs(term[i]) < 4194304.0;  // (false for a NaN)
    if (terms_are_short(term) != all_below) ++bad, std::printf("path: %a %a %a %a %a -> short %d\n", term[0], term[1], term[2], term[3], term[4], terms_are_short(term));
    if (all_below) ++short_sets;
    else ++general_sets;
    if (want_flag) ++flagged;
    if (got_flag != want_flag || std::memcmp(want, got, sizeof(want)) != 0) {
        ++bad;
        std::printf("limbs: %a %a %a %a %a -> flag %d (to_fixed %d)\n", term[0], term[1], term[2], term[3], term[4], got_flag, want_flag);
        for (int k = 0; k < 5 * kTermLimbs; ++k)
            if (want[k] != got[k]) std::printf("    limb %d: %d, to_fixed %d\n", k, got[k], want[k]);
    }
}

int main() {
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> mant(1.0, 2.0);
    const double last_short = 4194304.0 - std::ldexp(1.0, -30), top = 8796093022207.0;  // 2^22 - 2^-30, 2^43 - 1
    const double special[] = {0.0, -0.0, std::ldexp(1.0, -41), -std::ldexp(1.0, -41), std::ldexp(3.0, -41), -std::ldexp(3.0, -41), std::ldexp(1.0, -42), -std::ldexp(1.0, -42),
                              1.0 + std::ldexp(1.0, -41), -1.0 - std::ldexp(1.0, -41), 4194303.0 + std::ldexp(1.0, -41), -4194303.0 - std::ldexp(5.0, -41),
                              last_short, -last_short, 4194304.0, -4194304.0, std::nextafter(4194304.0, 0.0), -std::nextafter(4194304.0, 0.0),
                              top, -top, kFixLimit, -kFixLimit, std::nextafter(kFixLimit, 0.0), NAN, -NAN, INFINITY, -INFINITY, 5e-324, -5e-324, 1e300};
    const double small[] = {0.0, 0.25, -3.5, 1234.5678, -99999.000001, 4194303.999};
    constexpr int kSpecial = sizeof(special) / sizeof(special[0]), kSmall = sizeof(small) / sizeof(small[0]);
    // every special value in every position, beside small terms ...
    for (int a = 0; a < kSpecial; ++a)
        for (int pos = 0; pos < 5; ++pos)
            for (int f = 0; f < kSmall; ++f) {
                double t[5];
                for (int i = 0; i < 5; ++i) t[i] = small[(f + i) % kSmall];
                t[pos] = special[a];
                check(t);
            }
    // ... beside another special value in every other position, and five times itself
    for (int a = 0; a < kSpecial; ++a) {
        const double same[5] = {special[a], special[a], special[a], special[a], special[a]};
        check(same);
        for (int b = 0; b < kSpecial; ++b)
            for (int pa = 0; pa < 5; ++pa)
                for (int pb = 0; pb < 5; ++pb) {
                    if (pa == pb) continue;
                    double t[5] = {0.5, -0.5, 2.0, -1e-3, 100.0};
                    t[pa] = special[a], t[pb] = special[b];
                    check(t);
                }
    }
    // ties of the 2^-41 grid and their neighbours around 0, 1, 2^20 and the short path's end
    for (long long k = -500; k <= 500; ++k)
        for (double base : {0.0, 1.0, 1048576.0, 4194304.0, -4194304.0}) {
            const double x = base + std::ldexp(static_cast<double>(k), -41);
            const double t[5] = {x, std::nextafter(x, 1e300), std::nextafter(x, -1e300), -x, 0.0};
            check(t);
        }
    // 10^5 random values per binade [2^e, 2^(e+1)), e = -45 .. 43 (the top one lies beyond the range), signs at random
    for (int e = -45; e <= 43; ++e)
        for (int k = 0; k < 20000; ++k) {
            double t[5];
            for (int i = 0; i < 5; ++i) t[i] = std::ldexp(mant(rng), e) * ((rng() & 1u) ? -1.0 : 1.0);
            check(t);
        }
    // four terms of a scan near the base frame, one large term in every position
    std::uniform_real_distribution<double> near(-10000.0, 10000.0);
    for (int e = 21; e <= 43; ++e)
        for (int k = 0; k < 2000; ++k) {
            double t[5];
            for (int i = 0; i < 5; ++i) t[i] = near(rng);
            t[k % 5] = std::ldexp(mant(rng), e) * ((rng() & 1u) ? -1.0 : 1.0);
            check(t);
        }
    std::printf("terms fixed: %ld bad of %ld sets checked, %ld on the short path, %ld on the general one, %ld with the range flag\n", bad, checked, short_sets, general_sets,
                flagged);
    return bad == 0 ? 0 : 1;
}
