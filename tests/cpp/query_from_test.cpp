// axis_from of kicp_pass_visit.hpp on the HOST (__host__ __device__: the device runs the same operations): the query's offset as seen from
// the corner of neighbour voxel s, l - d 65536 with d the component of shift s, from the order packed as the top bits of the float
// -2 d.  It must be THE SAME FLOAT as the form it replaced - the integer component extracted (shift_component), converted and
// multiplied, then subtracted - for all 27 shifts on all three axes and
//   * every integer offset 0 .. 65 535,
//   * every integer offset plus 1/2, 1/4, 1/256 (the finest fraction an offset above 32 768 has) and the floats next to each,
//   * 2 000 000 random offsets in [0, 65 536), and the largest float below 65 536.
// Also: the packed words hold the order's components (d = -1, 0, 1 <-> 2.0, 0, -2.0) and nothing above shift 26.
// Built by tests/test_query_from.py with `hipcc --cuda-host-only` and the host's address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "kicp_pass_visit.hpp"

using namespace kicp;

static long bad = 0, checked = 0;

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof(u));
    return u;
}
static void check(float l) {
    const uint64_t from[3] = {kFromX, kFromY, kFromZ}, order[3] = {kShiftX, kShiftY, kShiftZ};
    for (int axis = 0; axis < 3; ++axis)
        for (int s = 0; s < 27; ++s) {
            const int d = shift_component(order[axis], s);
            const float want = l - d * kCell;  // the form before
            const float got = axis_from(l, from[axis], s);
            ++checked;
            if (bits(want) != bits(got)) ++bad, std::printf("axis %d shift %d (d %d): l %a -> %a, before %a\n", axis, s, d, l, got, want);
        }
}

int main() {
    const uint64_t from[3] = {kFromX, kFromY, kFromZ};
    for (int axis = 0; axis < 3; ++axis) {
        if (from[axis] >> 54) ++bad, std::printf("axis %d: bits above shift 26\n", axis);
        for (int s = 0; s < 27; ++s) {
            const uint32_t word = static_cast<uint32_t>(from[axis] >> (2 * s)) << 30;
            float f;
            std::memcpy(&f, &word, sizeof(f));
            if (f != -2.0f * kShiftTable[s][axis]) ++bad, std::printf("axis %d shift %d: packed %a, component %d\n", axis, s, f, kShiftTable[s][axis]);
        }
    }
    for (int k = 0; k < 65536; ++k) {
        const float l = static_cast<float>(k);
        check(l);
        for (float frac : {0.5f, 0.25f, 0.00390625f}) {
            const float x = l + frac;
            check(x), check(std::nextafter(x, 0.0f)), check(std::nextafter(x, 65536.0f));
        }
    }
    check(std::nextafter(65536.0f, 0.0f)), check(std::nextafter(0.0f, 1.0f)), check(1.0e-30f);
    std::mt19937_64 rng(99);
    std::uniform_real_distribution<double> frac(0.0, 1.0);
    for (int k = 0; k < 2000000; ++k) {
        const float l = static_cast<float>(frac(rng)) * kCell;  // (as voxel_coord_offset forms it)
        if (l < kCell) check(l);
    }
    std::printf("query from: %ld bad of %ld checked\n", bad, checked);
    return bad == 0 ? 0 : 1;
}
