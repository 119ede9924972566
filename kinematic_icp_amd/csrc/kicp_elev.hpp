// kicp_elev.hpp -- the kernels of the height columns (kicp_elev_*; C-ABI: kicp_elev.hip, arithmetic: kicp_elev_host.hpp).
//
//   k_elev_mark      one lane per point: the transform, the cell, the reach and range tests and the slab, then the point's bit is set in
//                    its cell's 64-bit column - ONE launch per frame.  No frame-local planes: OR is idempotent, so the columns
//                    deduplicate the points themselves.  TEST BEFORE SET: the lane loads the column and issues the atomic OR only
//                    when it finds the bit clear.  A robot re-observes what it has seen, so in steady state nearly every lane finds its
//                    bit set, and a plain load is served by L2 while an atomic executes beyond it and drops the line from it
//   k_elev_list      (an UPDATE only, before the mark) one lane per point: the points whose rays carve are appended to a list
//   k_elev_carve     (an UPDATE only, before the mark) one wave per entry of that list, its lanes striding over the ray's steps as
//                    k_grid_rays' do: each step clears a span of slabs in the column of the cell it visits - TEST BEFORE CLEAR, a 64-bit
//                    atomic AND only where the loaded column has something to clear.  No frame-local plane: AND is idempotent too, so
//                    rays that share a triple repeat loads, not atomics
//   k_elev_classify  a tile of 16 x 16 cells per workgroup: each lane reduces its column to a ground byte, the tile's grounds and a
//                    one-cell halo go through LDS, BODY comes from the lane's own column by shifts and STEP from the eight
//                    neighbours in LDS; the classes, the optional ground bytes and per-wave sums of the four counts are written
//   k_elev_to_grid   the same classification (elev_classify_cell, one device function for both) written as the two 16-bit counters
//                    of a kicp_grid
//   k_elev_fit<L, Rough>  the same tile with a halo of L <= 8 cells in LDS: a lane whose cell is known also walks its (2 L + 1)^2 window
//                    of grounds into nine integer sums, and a least-squares plane through them - three 64-bit determinants, compared
//                    in 128-bit integers - adds the class SLOPE; the optional determinants and five counts are written.  With Rough
//                    a tenth sum, z^2: the residual of the fitted plane, Q, in 64-bit integers, compared as a 128-bit product, adds the
//                    class ROUGH; the optional D, Da, Db, Q, n and six counts are written.  One instantiation per L, so that the
//                    walk unrolls; ONE text for both classes (elev_fit_cell), `if constexpr (Rough)` around what ROUGH adds
//   k_elev_fit_to_grid<L, Rough>  that classification (elev_fit_cell, one device function for both) as a kicp_grid's counters
// The atomics besides the OR and the AND are the statistics and the list's length: one add per wave per word that has something to add.
// No kernel uses scratch; the mark, list and carve kernels use no LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "kicp_elev_host.hpp"

namespace kicp {

constexpr uint32_t kElevBlock = 256;
constexpr uint32_t kElevTile = 16;              // cells per side of a classification tile: kElevTile^2 lanes
constexpr uint32_t kElevHalo = kElevTile + 2u;  // its side with the halo
// A frame's statistics and the four counts of a classification are kept in kElevCountShards copies, each on a 128-byte line of its own,
// and summed on the host: one word takes an atomic add every 11 ns or so, whoever adds, and nearly every wave has something to add
// to the same few words - a frame that explores sets new bits in every wave, and most cells of a large layer are unknown
constexpr uint32_t kElevCountShards = 64, kElevCountStride = 32;
// this wave's shard of such a counter block
static __device__ __forceinline__ unsigned int *elev_shard(unsigned int *counters) {
    return counters + ((blockIdx.x * (kElevBlock / 64u) + threadIdx.x / 64u) % kElevCountShards) * kElevCountStride;
}

static __device__ __forceinline__ void elev_wave_add(unsigned int *counter, bool flag) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(counter, static_cast<unsigned int>(__popcll(b)));
}
// this lane's cell of a classification's tiles, relative to the rectangle's corner
static __device__ __forceinline__ void elev_lane_cell(uint32_t tiles_x, uint32_t &rx, uint32_t &ry) {
    rx = (blockIdx.x % tiles_x) * kElevTile + threadIdx.x % kElevTile, ry = (blockIdx.x / tiles_x) * kElevTile + threadIdx.x / kElevTile;
}
// a class as the (hits, misses) pair of a kicp_grid's cell, one 32-bit word: obstacle (1, 0), traversable (0, 1), unknown (0, 0)
static __device__ __forceinline__ uint32_t elev_grid_word(int8_t value) { return value < 0 ? 0u : value ? 1u : 0x10000u; }

// stats: kElevCountShards x kElevCountStride words; a wave adds skipped, outside_grid, outside_column, new_bits, new_cells to words
// 0 .. 4 of its shard.  The used points are what the host derives: in steady state nearly every point is used and nothing is new, and
// a wave with nothing to add issues no atomic at all.
static __global__ __launch_bounds__(kElevBlock) void k_elev_mark(const double *__restrict__ xyz, uint32_t n, ElevGeom g, ElevFrame f, unsigned long long *columns,
                                                                 unsigned int *__restrict__ stats) {
    const uint32_t i = blockIdx.x * kElevBlock + threadIdx.x;
    int cls = kElevUsed;  // (a lane beyond the frame counts as nothing: the used points are the ones that are not counted)
    bool new_bit = false, new_cell = false;
    size_t cell = 0;
    uint32_t slab = 0;
    const bool point = i < n;
    if (point) cls = elev_point(g, f, xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2], cell, slab);
    if (point && cls == kElevUsed) {  // cell < width * height: elev_point compared both coordinates with the grid's extent
        const unsigned long long bit = 1ull << slab;
        // A STALE VALUE IS SAFE HERE.  Within a launch a bit only ever goes from clear to set, so a load that misses another lane's OR
        // can only read the bit as clear, and that costs a redundant atomic, never a lost bit; a load can never read a bit as set
        // that is not.  Between entries the handle's stream is drained (the grid's stream rule), so a launch sees all that earlier
        // calls wrote.  The statistics do not rest on this load: they come from the atomic's returned value - exactly one atomic
        // sees each bit clear, and exactly one sees each column zero.
        if (!(columns[cell] & bit)) {
            const unsigned long long old = atomicOr(&columns[cell], bit);
            new_bit = !(old & bit), new_cell = old == 0ull;
        }
    }
    unsigned int *shard = elev_shard(stats);
    elev_wave_add(&shard[0], cls == kElevSkipped);
    elev_wave_add(&shard[1], cls == kElevOutsideGrid);
    elev_wave_add(&shard[2], cls == kElevOutsideColumn);
    elev_wave_add(&shard[3], new_bit);
    elev_wave_add(&shard[4], new_cell);
}

// ---- carving (kicp_elev_update*): two launches in front of k_elev_mark ---------------------------------------------------------------
// A record of the carve list: the endpoint cell relative to the sensor's, each offset by reach (13 bits each: reach <= 4095), and the
// endpoint's slab offset by 32768 (16 bits).
static __device__ __forceinline__ unsigned long long elev_ray_pack(int32_t dx, int32_t dy, int32_t es, int32_t reach) {
    return static_cast<unsigned long long>(static_cast<uint32_t>(dx + reach) | static_cast<uint32_t>(dy + reach) << 13) |
           static_cast<unsigned long long>(static_cast<uint32_t>(es + 32768)) << 26;
}
static __device__ __forceinline__ uint32_t elev_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
constexpr uint32_t kElevListWord = 7;  // word of shard 0 that holds the carve list's length; words 5 and 6 of a shard: bits_cleared, cells_emptied

// The eligible points append (dx, dy, es) to `rays` (room for n entries) by ballot compaction; stats[kElevListWord] becomes the list's
// length, the frame's carve_points.  A lane takes kElevListPoints points, 64 apart, so that a wave has ONE add to the list's length for
// 256 points: that word takes an add about every 11 ns, and with an add per 64 points a 131 072-point frame spent 23 of this
// kernel's 26 us queueing for it.
constexpr uint32_t kElevListPoints = 4;
static __global__ __launch_bounds__(kElevBlock) void k_elev_list(const double *__restrict__ xyz, uint32_t n, ElevGeom g, ElevFrame f, unsigned long long *__restrict__ rays,
                                                                 unsigned int *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = (blockIdx.x * (kElevBlock / 64u) + threadIdx.x / 64u) * (64u * kElevListPoints) + lane;  // (n <= 0x7FFFFFF0 / 3: no overflow)
    unsigned long long record[kElevListPoints], ballots[kElevListPoints];
    uint32_t total = 0;
#pragma unroll
    for (uint32_t t = 0; t < kElevListPoints; ++t) {
        const uint32_t i = first + 64u * t;
        bool eligible = false;
        int32_t dx = 0, dy = 0, es = 0;
        if (i < n) eligible = elev_carve_point(g, f, xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2], dx, dy, es);
        record[t] = elev_ray_pack(dx, dy, es, g.plane.reach);
        ballots[t] = __ballot(eligible);
        total += static_cast<uint32_t>(__popcll(ballots[t]));
    }
    uint32_t base = 0;
    if (lane == 0u && total) base = atomicAdd(&stats[kElevListWord], total);
    base = __shfl(base, 0, 64);
#pragma unroll
    for (uint32_t t = 0; t < kElevListPoints; ++t) {
        if ((ballots[t] >> lane) & 1ull) rays[base + static_cast<uint32_t>(__popcll(ballots[t] & ((1ull << lane) - 1ull)))] = record[t];  // < n: one per eligible point
        base += static_cast<uint32_t>(__popcll(ballots[t]));
    }
}

// rays[0 .. *n_rays): one wave per entry, striding; the lanes take the steps k = lane, lane + 64, .. of that ray, each its cell and its
// mask.  TEST BEFORE CLEAR: a lane loads the column and issues the atomic AND only when it finds something to clear.
// A STALE VALUE IS SAFE HERE.  Within this launch bits only go from set to clear, and with keep_ground the lowest set bit of a column
// never changes (no lane clears it, whichever value it computed it from), so a load that misses another lane's AND can only cost a
// redundant atomic: never a lost clear, never another `keep`.  The statistics come from the atomics' returned values - exactly one
// atomic sees each bit set, and exactly one takes a column to zero - summed per wave into words 5 and 6 of its shard.
static __global__ __launch_bounds__(kElevBlock) void k_elev_carve(const unsigned long long *__restrict__ rays, const unsigned int *__restrict__ n_rays, ElevGeom g, ElevFrame f,
                                                                  int32_t ss, ElevCarveParams p, unsigned long long *columns, unsigned int *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const int32_t reach = g.plane.reach;
    const uint32_t waves = gridDim.x * (kElevBlock / 64u), count = *n_rays;
    uint32_t cleared = 0, emptied = 0;
    for (uint32_t r = blockIdx.x * (kElevBlock / 64u) + threadIdx.x / 64u; r < count; r += waves) {
        const unsigned long long rec = rays[r];
        const int32_t dx = static_cast<int32_t>(static_cast<uint32_t>(rec) & 0x1FFFu) - reach, dy = static_cast<int32_t>(static_cast<uint32_t>(rec >> 13) & 0x1FFFu) - reach;
        const int32_t es = static_cast<int32_t>(static_cast<uint32_t>(rec >> 26) & 0xFFFFu) - 32768;
        const uint32_t m = grid_walk_length(dx, dy), steps = elev_carve_steps(m, p.margin_steps);  // steps <= m <= reach
        for (uint32_t k = lane; k < steps; k += 64u) {
            int32_t ox, oy;
            grid_step(dx, dy, m, k, ox, oy);
            size_t cell;
            if (!grid_inside(g.plane, f.plane, static_cast<uint32_t>(ox + reach), static_cast<uint32_t>(oy + reach), cell)) continue;  // every access is behind this test
            const unsigned long long mask = elev_step_mask(ss, es, m, k, p.widen_slabs);
            const unsigned long long c = columns[cell];
            const unsigned long long clear = elev_clear_mask(c, mask, p.keep_ground);
            if (!(c & clear)) continue;
            const unsigned long long old = atomicAnd(&columns[cell], ~clear);
            cleared += static_cast<uint32_t>(__popcll(old & clear));
            emptied += (old != 0ull && (old & ~clear) == 0ull) ? 1u : 0u;
        }
    }
    cleared = elev_wave_sum(cleared), emptied = elev_wave_sum(emptied);
    if (lane == 0u) {
        unsigned int *shard = elev_shard(stats);
        if (cleared) atomicAdd(&shard[5], cleared);
        if (emptied) atomicAdd(&shard[6], emptied);
    }
}

// The class of this lane's cell, (r.x0 + tile_x kElevTile + tx, r.y0 + tile_y kElevTile + ty) with tx = threadIdx.x % kElevTile: every
// lane of the workgroup calls it (it holds the barrier).  grounds: kElevHalo^2 bytes of LDS.  -> inside: the cell lies in the
// rectangle; value, ground and which (elev_value) are its results.  Halo cells outside the rectangle but inside the grid are read
// like any other, so a rectangle's result is the full grid's restricted to it; cells outside the grid read as unknown.
static __device__ __forceinline__ bool elev_classify_cell(const unsigned long long *__restrict__ columns, uint32_t width, uint32_t height, const ElevParams &p,
                                                          const ElevRect &r, uint32_t tiles_x, uint8_t *grounds, int8_t &value, uint8_t &ground, uint32_t &which) {
    const uint32_t tx = threadIdx.x % kElevTile, ty = threadIdx.x / kElevTile;
    const uint32_t bx = r.x0 + (blockIdx.x % tiles_x) * kElevTile, by = r.y0 + (blockIdx.x / tiles_x) * kElevTile;  // the tile's corner: inside the rectangle
    const uint32_t x = bx + tx, y = by + ty;
    const bool in_grid = x < width && y < height;
    const bool inside = x - r.x0 < r.w && y - r.y0 < r.h;  // (inside the rectangle implies inside the grid)
    const unsigned long long c = in_grid ? columns[static_cast<size_t>(y) * width + x] : 0ull;
    ground = elev_ground(c);
    grounds[(ty + 1u) * kElevHalo + (tx + 1u)] = ground;
    if (threadIdx.x < 4u * kElevTile + 4u) {  // the halo's 68 cells: two rows of kElevHalo, two columns of kElevTile
        const uint32_t k = threadIdx.x;
        const uint32_t hx = k < kElevHalo ? k : k < 2u * kElevHalo ? k - kElevHalo : k < 2u * kElevHalo + kElevTile ? 0u : kElevHalo - 1u;
        const uint32_t hy = k < kElevHalo ? 0u : k < 2u * kElevHalo ? kElevHalo - 1u : k < 2u * kElevHalo + kElevTile ? k - 2u * kElevHalo + 1u : k - 2u * kElevHalo - kElevTile + 1u;
        const int64_t gx = static_cast<int64_t>(bx) + hx - 1, gy = static_cast<int64_t>(by) + hy - 1;
        const bool ok = gx >= 0 && gy >= 0 && gx < static_cast<int64_t>(width) && gy < static_cast<int64_t>(height);
        grounds[hy * kElevHalo + hx] = ok ? elev_ground(columns[static_cast<size_t>(gy) * width + static_cast<size_t>(gx)]) : kElevNoGround;
    }
    __syncthreads();
    bool body = false, step = false;
    if (c) {
        body = elev_body(c, ground, p);
#pragma unroll
        for (uint32_t dy = 0; dy < 3u; ++dy)
#pragma unroll
            for (uint32_t dx = 0; dx < 3u; ++dx)
                if (dx != 1u || dy != 1u) step = step || elev_step(ground, grounds[(ty + dy) * kElevHalo + (tx + dx)], p);
    }
    value = elev_value(which, c != 0ull, body, step);
    return inside;
}

// out / out_ground (nullable): r.h * r.w values; counts (nullable): kElevCountShards x kElevCountStride words, a wave adds unknown,
// traversable, BODY, STEP only to words 0 .. 3 of its shard
static __global__ __launch_bounds__(kElevBlock) void k_elev_classify(const unsigned long long *__restrict__ columns, uint32_t width, uint32_t height, ElevParams p, ElevRect r,
                                                                     uint32_t tiles_x, int8_t *__restrict__ out, uint8_t *__restrict__ out_ground,
                                                                     unsigned int *__restrict__ counts) {
    __shared__ uint8_t grounds[kElevHalo * kElevHalo];
    int8_t value;
    uint8_t ground;
    uint32_t which;
    const bool inside = elev_classify_cell(columns, width, height, p, r, tiles_x, grounds, value, ground, which);
    if (inside) {
        uint32_t rx, ry;
        elev_lane_cell(tiles_x, rx, ry);
        const size_t o = static_cast<size_t>(ry) * r.w + rx;
        out[o] = value;
        if (out_ground) out_ground[o] = ground;
    }
    if (counts) {
        unsigned int *shard = elev_shard(counts);
        for (uint32_t k = 0; k < 4u; ++k) elev_wave_add(&shard[k], inside && which == k);
    }
}

// grid_counts: the (hits, misses) pairs of a kicp_grid of width x height cells, written whole: obstacle (1, 0), traversable (0, 1),
// unknown (0, 0).  The rectangle is the full grid.
static __global__ __launch_bounds__(kElevBlock) void k_elev_to_grid(const unsigned long long *__restrict__ columns, uint32_t width, uint32_t height, ElevParams p, ElevRect r,
                                                                    uint32_t tiles_x, uint16_t *__restrict__ grid_counts) {
    __shared__ uint8_t grounds[kElevHalo * kElevHalo];
    int8_t value;
    uint8_t ground;
    uint32_t which;
    if (!elev_classify_cell(columns, width, height, p, r, tiles_x, grounds, value, ground, which)) return;  // (behind the barrier)
    uint32_t x, y;
    elev_lane_cell(tiles_x, x, y);
    reinterpret_cast<uint32_t *>(grid_counts)[static_cast<size_t>(y) * width + x] = elev_grid_word(value);
}

// ---- the plane fit: the slope limit and ROUGH (kicp_elev_traversability_slope / _rough, kicp_elev_to_grid_slope / _rough) --------------
// The window of a known cell out of LDS into the nine sums, with Rough the tenth.  L IS A TEMPLATE ARGUMENT: both loops unroll, dx, dy,
// their products and the byte offsets become constants, and the walk of a fully known 1 600 x 1 600 layer at L = 8 takes 0.29 ms where
// the same loops bounded by a kernel argument took 0.70.
template <int L, bool Rough>
static __device__ __forceinline__ void elev_fit_walk(const uint8_t *centre, uint32_t ground, uint32_t gate, ElevFitSums &s) {
    constexpr int32_t side = static_cast<int32_t>(kElevTile) + 2 * L;
#pragma unroll
    for (int32_t dy = -L; dy <= L; ++dy)
#pragma unroll
        for (int32_t dx = -L; dx <= L; ++dx) elev_fit_add<Rough>(s, ground, centre[dy * side + dx], dx, dy, gate);
}
// The class of this lane's cell with the slope limit and, with Rough, the class ROUGH; the lane's cell as in elev_classify_cell: every
// lane of the workgroup calls it (it holds the barrier).  L = sp.radius (the host picks the instantiation).  grounds: side^2 bytes of
// LDS, side = kElevTile + 2 L: the tile's grounds and a halo of L cells, loaded by all lanes in a strided loop along rows, EVERY LOAD
// BEHIND THE INSIDE-THE-GRID TEST; a cell outside the grid reads 255 like an unknown one.  After the barrier a lane whose cell is known
// walks its (2 L + 1)^2 window out of LDS into the sums; a lane whose cell is unknown skips the walk - most of a real layer is unknown,
// and a wave with no known cell branches over it.  STEP comes from the same bytes, BODY from the lane's own column.  Every loop is
// bounded by L <= 8.  With Rough a cell with a fit also gets the residual Q (64-bit, by elev_rough_residual's bounds) and the 128-bit
// comparison; rp is read with Rough only.
// -> inside: the cell lies in the rectangle; value, ground, which (elev_value) and fit = D, Da, Db, with Rough also Q, n (zeros without
// a fit) are its results.
template <int L, bool Rough>
static __device__ __forceinline__ bool elev_fit_cell(const unsigned long long *__restrict__ columns, uint32_t width, uint32_t height, const ElevParams &p,
                                                     const ElevSlopeParams &sp, const ElevRoughParams &rp, const ElevRect &r, uint32_t tiles_x, uint8_t *grounds,
                                                     int8_t &value, uint8_t &ground, uint32_t &which, int64_t (&fit)[kElevFitValues<Rough>]) {
    static_assert(L >= 1 && L <= static_cast<int>(kElevSlopeMaxRadius), "the halo is 1 .. 8 cells");
    constexpr uint32_t side = kElevTile + 2u * L;
    const uint32_t tx = threadIdx.x % kElevTile, ty = threadIdx.x / kElevTile;
    const uint32_t bx = r.x0 + (blockIdx.x % tiles_x) * kElevTile, by = r.y0 + (blockIdx.x / tiles_x) * kElevTile;  // the tile's corner: inside the rectangle
    const uint32_t x = bx + tx, y = by + ty;
    const bool inside = x - r.x0 < r.w && y - r.y0 < r.h;  // (inside the rectangle implies inside the grid)
#pragma unroll
    for (uint32_t k = threadIdx.x; k < side * side; k += kElevBlock) {  // at most four trips
        const uint32_t hx = k % side, hy = k / side;
        const int64_t gx = static_cast<int64_t>(bx) + hx - L, gy = static_cast<int64_t>(by) + hy - L;
        const bool ok = gx >= 0 && gy >= 0 && gx < static_cast<int64_t>(width) && gy < static_cast<int64_t>(height);
        grounds[k] = ok ? elev_ground(columns[static_cast<size_t>(gy) * width + static_cast<size_t>(gx)]) : kElevNoGround;
    }
    __syncthreads();
    const uint8_t *centre = grounds + (ty + L) * side + (tx + L);
    ground = *centre;
    const bool known = ground != kElevNoGround;
    bool body = false, step = false, slope = false, rough = false;
#pragma unroll
    for (uint32_t k = 0; k < kElevFitValues<Rough>; ++k) fit[k] = 0;
    if (known) {  // (a known cell lies inside the grid: the load is behind that test)
        body = elev_body(columns[static_cast<size_t>(y) * width + x], ground, p);
#pragma unroll
        for (int32_t dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int32_t dx = -1; dx <= 1; ++dx)
                if (dx || dy) step = step || elev_step(ground, centre[dy * static_cast<int32_t>(side) + dx], p);
        ElevFitSums s{};
        elev_fit_walk<L, Rough>(centre, ground, sp.gate, s);
        int64_t d, da, db;
        elev_slope_determinants(s, d, da, db);
        if (elev_slope_has_fit(s, d, sp)) {  // THE ORDER COUNTS: residual, SLOPE, ROUGH, then the triple - stored first it costs 7 .. 10 VGPRs
            if constexpr (Rough) {
                int64_t dc;
                fit[3] = elev_rough_residual(s, d, da, db, dc), fit[4] = s.n;
            }
            slope = elev_slope_exceeds(d, da, db, sp);
            if constexpr (Rough) rough = elev_rough_exceeds(fit[3], d, s.n, rp);
            fit[0] = d, fit[1] = da, fit[2] = db;
        }
    }
    value = elev_value(which, known, body, step, slope, rough);
    return inside;
}

// out / out_ground (nullable) / out_fit (nullable: kElevFitValues<Rough> values per cell): r.h * r.w entries; counts (nullable):
// kElevCountShards x kElevCountStride words, a wave adds unknown, traversable, BODY, STEP only, SLOPE only and with Rough ROUGH only to
// words 0 .. 4 or 5 of its shard
template <int L, bool Rough>
static __global__ __launch_bounds__(kElevBlock) void k_elev_fit(const unsigned long long *__restrict__ columns, uint32_t width, uint32_t height, ElevParams p,
                                                                ElevSlopeParams sp, ElevRoughParams rp, ElevRect r, uint32_t tiles_x, int8_t *__restrict__ out,
                                                                uint8_t *__restrict__ out_ground, long long *__restrict__ out_fit, unsigned int *__restrict__ counts) {
    constexpr uint32_t values = kElevFitValues<Rough>;
    __shared__ uint8_t grounds[(kElevTile + 2u * L) * (kElevTile + 2u * L)];
    int8_t value;
    uint8_t ground;
    uint32_t which;
    int64_t fit[values];
    const bool inside = elev_fit_cell<L, Rough>(columns, width, height, p, sp, rp, r, tiles_x, grounds, value, ground, which, fit);
    if (inside) {
        uint32_t rx, ry;
        elev_lane_cell(tiles_x, rx, ry);
        const size_t o = static_cast<size_t>(ry) * r.w + rx;
        out[o] = value;
        if (out_ground) out_ground[o] = ground;
        if (out_fit) {
#pragma unroll
            for (uint32_t k = 0; k < values; ++k) out_fit[values * o + k] = fit[k];
        }
    }
    if (counts) {
        unsigned int *shard = elev_shard(counts);
        for (uint32_t k = 0; k < kElevFitCounts<Rough>; ++k) elev_wave_add(&shard[k], inside && which == k);
    }
}

// k_elev_to_grid with the slope limit and, with Rough, the class ROUGH: the rectangle is the full grid
template <int L, bool Rough>
static __global__ __launch_bounds__(kElevBlock) void k_elev_fit_to_grid(const unsigned long long *__restrict__ columns, uint32_t width, uint32_t height, ElevParams p,
                                                                        ElevSlopeParams sp, ElevRoughParams rp, ElevRect r, uint32_t tiles_x,
                                                                        uint16_t *__restrict__ grid_counts) {
    __shared__ uint8_t grounds[(kElevTile + 2u * L) * (kElevTile + 2u * L)];
    int8_t value;
    uint8_t ground;
    uint32_t which;
    int64_t fit[kElevFitValues<Rough>];
    if (!elev_fit_cell<L, Rough>(columns, width, height, p, sp, rp, r, tiles_x, grounds, value, ground, which, fit)) return;  // (behind the barrier)
    uint32_t x, y;
    elev_lane_cell(tiles_x, x, y);
    reinterpret_cast<uint32_t *>(grid_counts)[static_cast<size_t>(y) * width + x] = elev_grid_word(value);
}

}  // namespace kicp
