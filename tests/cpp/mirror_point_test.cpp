// The 16-bit mirror's point format (kicp_common.hpp::MirrorPoint) on the HOST - the helpers are __host__ __device__, the device runs the
// same operations:
//   * for all 65 536 quantised z values the second word, read as a float, is static_cast<float> of the integer, reads back as the same
//     integer, and the slot counts as a point (z = 0, whose word is 0x00000000, and z = 65 535 included); word 0 is x | y << 16;
//   * mirror_empty() reads as exactly 4 294 901 760.0f - what the integer word 0xFFFF0000 of the earlier format converted to - and as
//     "no point"; every point's word is below the empty pattern as an unsigned integer (the kernels' one-compare test);
//   * mirror_point clamps offsets below 0 to 0 and offsets at or above the voxel's far face to 65 535, on every axis.
// Built by tests/test_mirror_point.py with `hipcc --cuda-host-only`.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "kicp_common.hpp"

using namespace kicp;

static float as_float(uint32_t w) {
    float f;
    std::memcpy(&f, &w, 4);
    return f;
}
static uint32_t as_word(float f) {
    uint32_t w;
    std::memcpy(&w, &f, 4);
    return w;
}

int main() {
    long bad = 0;
    const double vs = 1.0, upm = mirror_units_per_metre(vs);
    // every quantised z: the centre of its unit, and both ends of the interval that rounds to it
    for (uint32_t q = 0; q < 65536u; ++q) {
        const double offsets[3] = {q / upm, (q - 0.5) / upm, (q + 0.49) / upm};
        for (double o : offsets) {
            if (o < 0.0) continue;
            const uint32_t qx = (q * 7u + 3u) & 0xffffu, qy = 65535u - q;
            const MirrorPoint m = mirror_point(qx / upm, qy / upm, o, upm);
            if (mirror_quant(o, upm) != q) ++bad, std::printf("quant: offset %a -> %u, expected %u\n", o, mirror_quant(o, upm), q);
            const float want = static_cast<float>(q);
            if (m.y != as_word(want) || as_float(m.y) != want) ++bad, std::printf("word: z %u -> %08x\n", q, m.y);
            if (mirror_z(m) != want || mirror_word_z(m.y) != want) ++bad, std::printf("z as float: z %u -> %a\n", q, mirror_z(m));
            if (mirror_qz(m) != q) ++bad, std::printf("z as integer: z %u -> %u\n", q, mirror_qz(m));
            if (!mirror_is_point(m) || !mirror_word_is_point(m.y) || !(m.y < mirror_empty().y)) ++bad, std::printf("point: z %u reads as empty\n", q);
            if (m.x != (qx | (qy << 16))) ++bad, std::printf("word 0: z %u -> %08x\n", q, m.x);
        }
    }
    {  // the two ends, spelled out
        const MirrorPoint lo = mirror_point(0.5, 0.5, 0.0, upm), hi = mirror_point(0.5, 0.5, 65535.0 / upm, upm);
        if (lo.y != 0x00000000u || !mirror_is_point(lo) || mirror_z(lo) != 0.0f) ++bad, std::printf("z = 0: %08x\n", lo.y);
        if (hi.y != 0x477FFF00u || !mirror_is_point(hi) || mirror_z(hi) != 65535.0f) ++bad, std::printf("z = 65535: %08x\n", hi.y);
    }
    {  // the empty slot
        const MirrorPoint e = mirror_empty();
        const float was = static_cast<float>(0xFFFF0000u);  // the earlier format's word, converted as the kernel converted it
        if (mirror_z(e) != 4294901760.0f || mirror_z(e) != was || mirror_z(e) != kMirrorEmptyZ) ++bad, std::printf("empty: reads %a\n", mirror_z(e));
        if (e.y != as_word(4294901760.0f) || e.y != kMirrorEmptyWord || e.x != 0u) ++bad, std::printf("empty: words %08x %08x\n", e.x, e.y);
        if (mirror_is_point(e) || mirror_word_is_point(e.y)) ++bad, std::printf("empty: reads as a point\n");
    }
    // clamping: below 0 and at or above the far face, on every axis
    const double below[4] = {-1e-9, -0.25, -3.0, -1e30}, above[5] = {vs, vs * (1.0 + 1e-12), vs - 0.4 / upm, 2.5 * vs, 1e30};
    for (double o : below) {
        const MirrorPoint m = mirror_point(o, o, o, upm);
        if (mirror_quant(o, upm) != 0u || m.x != 0u || m.y != 0u || mirror_qz(m) != 0u || !mirror_is_point(m)) ++bad, std::printf("clamp below: %a -> %08x %08x\n", o, m.x, m.y);
    }
    for (double o : above) {
        const MirrorPoint m = mirror_point(o, o, o, upm);
        if (mirror_quant(o, upm) != 65535u || m.x != 0xFFFFFFFFu || mirror_qz(m) != 65535u || mirror_z(m) != 65535.0f || !mirror_is_point(m))
            ++bad, std::printf("clamp above: %a -> %08x %08x\n", o, m.x, m.y);
    }
    // another voxel size: the units follow it
    const double upm2 = mirror_units_per_metre(0.3);
    if (mirror_qz(mirror_point(0.0, 0.0, 0.15, upm2)) != 32768u || mirror_qz(mirror_point(0.0, 0.0, 0.3, upm2)) != 65535u) ++bad, std::printf("voxel size 0.3\n");
    std::printf("mirror point: %ld bad\n", bad);
    return bad ? 1 : 0;
}
