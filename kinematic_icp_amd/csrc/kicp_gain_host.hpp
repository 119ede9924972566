// kicp_gain_host.hpp -- the arithmetic of the grid's information gain (kicp_grid_gain, kicp_gain_from_occupancy; include/kicp.h states
// the semantics): the 8 R perimeter offsets by a ray index, the decision at one step of one ray - the four tests in their order, on
// top of kicp_grid_host.hpp's grid_step and kicp_clear_host.hpp's clear_class - the row of one viewpoint and the host entry's walk.
// ONE text for the kernels (kicp_gain.hpp), for the entries (kicp_grid_explore.hip) and for the stand-alone program that runs gain_host::
// under sanitizers (tests/cpp/gain_host_test.cpp).  Everything is integer.
//
// THE WINDOW of a viewpoint is the (2 R + 1)^2 square of offsets around it; offset (ox, oy) has the bit (oy + R) (2 R + 1) + ox + R of
// a bit plane of ceil((2 R + 1)^2 / 32) words.  A cell that is SEEN sets its bit, so a cell that several rays cross counts once: word
// 0 of the row is the plane's population count.
#pragma once
#include <vector>

#include "kicp_clear_host.hpp"

namespace kicp {

constexpr uint32_t kGainWords = 4;       // KICP_GAIN_WORDS
constexpr uint32_t kGainMaxRange = 361;  // cells: the bit plane of the window stays within 64 KiB of LDS (65 344 bytes)
constexpr size_t kGainMaxViews = 1u << 24;  // viewpoints per call: one workgroup each

// what one step of a ray comes to: the ray goes on (over a clear cell, or over an unknown one that is thereby SEEN) or ends
enum : uint32_t { kGainOn = 0u, kGainSeen = 1u, kGainEndDisc = 2u, kGainEndLeft = 3u, kGainEndBlocked = 4u };
KICP_HD bool gain_ends(uint32_t verdict) { return verdict >= kGainEndDisc; }

struct GainParams {
    uint32_t min_observations;
    int32_t source_min;  // clear_source_min(occupied_thresh)
    uint32_t range;      // R, 1 .. kGainMaxRange
};

KICP_HD uint32_t gain_rays(uint32_t R) { return 8u * R; }
KICP_HD uint32_t gain_side(uint32_t R) { return 2u * R + 1u; }
KICP_HD uint32_t gain_plane_words(uint32_t R) { return (gain_side(R) * gain_side(R) + 31u) / 32u; }
// Ray i of the 8 R: the offsets with max(|dx|, |dy|) == R, each once - four runs of 2 R round the square, from (-R, -R) along the
// lower side, up the right one, back along the upper one and down the left one.
KICP_HD void gain_ray(uint32_t R, uint32_t i, int32_t &dx, int32_t &dy) {
    const int32_t r = static_cast<int32_t>(R), t = static_cast<int32_t>(i % (2u * R));
    switch (i / (2u * R)) {
        case 0u: dx = -r + t, dy = -r; break;
        case 1u: dx = r, dy = -r + t; break;
        case 2u: dx = r - t, dy = r; break;
        default: dx = -r, dy = r - t; break;
    }
}
// Step k (1 <= k <= R) of ray (dx, dy) from the viewpoint (vx, vy): the four tests in the header's order.  class_of(cell index) is the
// class of a cell inside the grid (kClearClear / kClearUnknown / kClearSource) and is asked only for such a cell inside the disc.
// `bit` is the visited offset's bit in the window's plane, set whenever the cell was looked at (the verdicts from kGainOn to
// kGainSeen, and kGainEndBlocked).
template <class ClassOf>
KICP_HD uint32_t gain_step(int32_t dx, int32_t dy, uint32_t R, uint32_t k, uint32_t vx, uint32_t vy, uint32_t width, uint32_t height, ClassOf class_of, uint32_t &bit) {
    int32_t ox, oy;
    grid_step(dx, dy, R, k, ox, oy);  // |ox|, |oy| <= k <= R
    if (static_cast<uint32_t>(ox * ox + oy * oy) > R * R) return kGainEndDisc;
    const int64_t x = static_cast<int64_t>(vx) + ox, y = static_cast<int64_t>(vy) + oy;
    if (x < 0 || y < 0 || x >= static_cast<int64_t>(width) || y >= static_cast<int64_t>(height)) return kGainEndLeft;
    const uint32_t cls = class_of(static_cast<size_t>(y) * width + static_cast<size_t>(x));
    bit = static_cast<uint32_t>(oy + static_cast<int32_t>(R)) * gain_side(R) + static_cast<uint32_t>(ox + static_cast<int32_t>(R));
    return cls == kClearSource ? kGainEndBlocked : cls == kClearUnknown ? kGainSeen : kGainOn;
}
// the row of one viewpoint; a viewpoint that is not clear has walked no ray: seen = blocked = left = 0
KICP_HD void gain_row(uint32_t *row, uint32_t seen, uint32_t blocked, uint32_t left, uint32_t view_class) {
    row[0] = seen, row[1] = blocked, row[2] = left, row[3] = view_class;
}
KICP_HD uint32_t gain_popcount(uint32_t v) {
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
}

namespace gain_host {
// The sequential host entry: viewpoint by viewpoint (each below width * height), ray by ray, step by step, with the window's bit plane
// cleared per viewpoint that is clear.  out: n x kGainWords.
inline void gain(const int8_t *occupancy, uint32_t width, uint32_t height, int32_t source_min, uint32_t R, const uint32_t *views, size_t n, uint32_t *out) {
    std::vector<uint32_t> plane(gain_plane_words(R));
    auto class_of = [&](size_t cell) { return clear_class(occupancy[cell], source_min); };
    for (size_t v = 0; v < n; ++v) {
        const uint32_t view_class = class_of(views[v]);
        uint32_t seen = 0, blocked = 0, left = 0;
        if (view_class == kClearClear) {
            const uint32_t vx = views[v] % width, vy = views[v] / width;
            plane.assign(plane.size(), 0u);
            for (uint32_t i = 0; i < gain_rays(R); ++i) {
                int32_t dx, dy;
                gain_ray(R, i, dx, dy);
                for (uint32_t k = 1; k <= R; ++k) {
                    uint32_t bit = 0;
                    const uint32_t verdict = gain_step(dx, dy, R, k, vx, vy, width, height, class_of, bit);
                    if (verdict == kGainSeen) plane[bit >> 5] |= 1u << (bit & 31u);
                    if (!gain_ends(verdict)) continue;
                    blocked += verdict == kGainEndBlocked ? 1u : 0u, left += verdict == kGainEndLeft ? 1u : 0u;
                    break;
                }
            }
            for (uint32_t w : plane) seen += gain_popcount(w);
        }
        gain_row(out + v * kGainWords, seen, blocked, left, view_class);
    }
}
}  // namespace gain_host

}  // namespace kicp
