// kicp_pass_visit.hpp -- the pass kernels' search over the 16-bit mirror ("variant 3"): a lane's start at its own voxel, the cull of the
// 27 neighbours, the bucket trips in packed fp32 with their integer-key tournament, and the visits built from them.  It PRE-SELECTS; the
// exact phase that follows (resolve_and_accumulate) and the loop that drives the visits (gather32_pass) are in kicp_kernels.hpp.
// voxel_coord, voxel_coord_offset and axis_from are __host__ __device__: tests/cpp runs them on the host.
#pragma once
#include "kicp_common.hpp"
#include "kicp_nn_exact.hpp"
#include "kicp_pass_params.hpp"
#include "kicp_se3.hpp"

namespace kicp {

// ------------------------------------------------------------------------------------------------------------
// variant 3: thread-per-query gather over the 16-bit mirror, per-lane work lists
//   * candidates are read from the compact mirror (kicp_common.hpp::MirrorPoint: 8 bytes per point, offsets from the voxel
//     corner in units of voxel_size / 65536; two points per 16-byte load) and compared in fp32 IN THOSE UNITS with packed
//     fp32 arithmetic (two points per instruction); the three smallest squared distances are tracked with the
//     indices / visiting order of the two smallest.  The mirror only PRE-SELECTS: the winner (and the runner-up when it
//     lies within the error margin) is re-evaluated in fp64 from the fp64 pool, ties resolved by the reference's visiting
//     order; if even the third smallest is within the margin the lane falls back to the exact fp64 search.  The chosen
//     neighbour and its distance are therefore exactly the fp64 reference's.
//   * each lane walks ITS OWN list of neighbour voxels (bit mask over the 27 shifts, in the reference's order): culled
//     voxels cost ALU only, so a wave iterates max-over-lanes(#voxels actually visited) times instead of over the union
//     of the lanes' shifts; a bucket is scanned 20 points per trip (ten 16-byte loads in flight).
// ------------------------------------------------------------------------------------------------------------
constexpr int kTrip = kMirrorTrip;  // bucket points in flight per lane and trip (even: two points per load)
typedef float v2f __attribute__((ext_vector_type(2)));
struct Best3 {
    float b1, b2, b3;
    uint32_t i1, i2, o1, o2;  // pool index and visiting order (shift * kOrdStride + k) of the two smallest
};
__device__ __forceinline__ void best3_update(Best3 &t, float d, uint32_t idx, uint32_t ord) {
    const bool lt1 = d < t.b1, lt2 = d < t.b2, lt3 = d < t.b3;
    t.b3 = lt2 ? t.b2 : (lt3 ? d : t.b3);
    t.b2 = lt1 ? t.b1 : (lt2 ? d : t.b2);
    t.i2 = lt1 ? t.i1 : (lt2 ? idx : t.i2);
    t.o2 = lt1 ? t.o1 : (lt2 ? ord : t.o2);
    t.b1 = lt1 ? d : t.b1;
    t.i1 = lt1 ? idx : t.i1;
    t.o1 = lt1 ? ord : t.o1;
}

// minimum of N register-resident unsigned keys (v_min3_u32 friendly reduction)
constexpr uint32_t kFarKey = 0x7F000000u;  // 1.7e38 as a float: beyond every real squared distance
template <int N>
__device__ __forceinline__ uint32_t tree_min_u32(const uint32_t (&v)[N]) {
    uint32_t a[N];
#pragma unroll
    for (int u = 0; u < N; ++u) a[u] = v[u];
#pragma unroll
    for (int width = N; width > 1; width = (width + 2) / 3) {
#pragma unroll
        for (int u = 0; u < (width + 2) / 3; ++u) {
            const int i0 = 3 * u, i1 = min(3 * u + 1, width - 1), i2 = min(3 * u + 2, width - 1);
            a[u] = min(a[i0], min(a[i1], a[i2]));
        }
    }
    return a[0];
}

// minimum AND runner-up of N register-resident unsigned keys in one tournament: every node carries (min, second).  For three
// nodes a, b, c:  min = min3(a.m, b.m, c.m);  second = min(med3(a.m, b.m, c.m), min3(a.s, b.s, c.s)) - the seconds of the two
// losing nodes are never smaller than the median of the minima, so they may take part unharmed (no selects).  20 keys: 26
// instructions, against 11 + 20 + 11 for a minimum, a re-keying subtraction and a second minimum.
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) { return max(min(a, b), min(max(a, b), c)); }  // -> v_med3_u32
template <int N>
__device__ __forceinline__ void tree_min2_u32(const uint32_t (&v)[N], uint32_t &first, uint32_t &second) {
    constexpr int L1 = (N + 2) / 3;
    uint32_t m[L1], s[L1];
#pragma unroll
    for (int u = 0; u < L1; ++u) {  // leaves: triples (the last node may hold one or two keys)
        const int i0 = 3 * u, i1 = 3 * u + 1, i2 = 3 * u + 2;
        if (i2 < N) m[u] = min(v[i0], min(v[i1], v[i2])), s[u] = umed3(v[i0], v[i1], v[i2]);
        else if (i1 < N) m[u] = min(v[i0], v[i1]), s[u] = max(v[i0], v[i1]);
        else m[u] = v[i0], s[u] = 0xFFFFFFFFu;
    }
#pragma unroll
    for (int width = L1; width > 1; width = (width + 2) / 3) {
#pragma unroll
        for (int u = 0; u < (width + 2) / 3; ++u) {
            const int i0 = 3 * u, i1 = 3 * u + 1, i2 = 3 * u + 2;
            if (i2 < width) {
                const uint32_t mm = min(m[i0], min(m[i1], m[i2])), md = umed3(m[i0], m[i1], m[i2]), ss = min(s[i0], min(s[i1], s[i2]));
                m[u] = mm, s[u] = min(md, ss);
            } else if (i1 < width) {
                const uint32_t mm = min(m[i0], m[i1]), mx = max(m[i0], m[i1]), ss = min(s[i0], s[i1]);
                m[u] = mm, s[u] = min(mx, ss);
            } else {
                m[u] = m[i0], s[u] = s[i0];
            }
        }
    }
    first = m[0], second = s[0];
}

// merge the three-smallest record of another lane into `t`
__device__ __forceinline__ void best3_merge(Best3 &t, const Best3 &o) {
    best3_update(t, o.b1, o.i1, o.o1);
    best3_update(t, o.b2, o.i2, o.o2);
    t.b3 = fminf(t.b3, o.b3);  // o.b3 can never undercut the runner-up of a set that already holds o.b1 <= o.b2
}

// best3_merge(t, o) for a `t` that holds nothing yet, t = {B, B, B, none, none, 0, 0}, and o.b1 <= o.b2 <= o.b3 as a trip's
// tournament leaves them - compare for compare: the first update takes o's winner iff o.b1 < B and leaves the rest at B; the second
// finds o.b2 >= the new t.b1 (o.b1, or B <= o.b1) and takes the runner-up's place iff o.b2 < B; t.b3 stays B but for o.b3.
// Three compares and six selects where the merge into an unknown record takes ~40 instructions.
__device__ __forceinline__ void best3_assign_fresh(Best3 &t, const Best3 &o) {
    const float B = t.b1;
    const bool lt1 = o.b1 < B, lt2 = o.b2 < B;
    t.b1 = lt1 ? o.b1 : B, t.i1 = lt1 ? o.i1 : kNoIndex32, t.o1 = lt1 ? o.o1 : 0u;
    t.b2 = lt2 ? o.b2 : B, t.i2 = lt2 ? o.i2 : kNoIndex32, t.o2 = lt2 ? o.o2 : 0u;
    t.b3 = fminf(B, o.b3);
}

// PointToVoxel component: static_cast<int>(floor(c / vs)) as the reference evaluates it (kiss-icp v1.2.0 core/VoxelUtils.hpp),
// without paying an fp64 division for every coordinate: t = c * (1 / vs) agrees with fl(c / vs) to a few ulps, so the two
// floors can only differ when t lies within that distance of an integer - and only then is the division carried out.
// "A few ulps" of t is below 4e-16 |t|, which is below 8.6e-7 for every |t| < 2^31 (beyond that the conversion to int32 is out of
// range on either path), so ONE constant guard serves all of them: the fast path is trusted while frac = t - floor(t) lies in
// [G, 1 - G], G = 1e-6 - an addition and a compare with |.| where a guard relative to |t| took five fp64 instructions per axis.  The
// division runs for 2e-6 of the coordinates instead of 1e-10 and yields the same integer wherever both paths are valid.
// voxel_coord_offset also hands back the query's offset inside that voxel in mirror units (Probe::lx ..), in [0, 65536).  On the fast
// path frac IS the offset in voxel sizes: one conversion and one fp32 product (frac <= 1 - 1e-6 keeps it below 65536) where
// (c - v vs) upm took five fp64 instructions.  Where the division decided, the offset is formed from the division's voxel, as before,
// and held to the range: that voxel is the reference's, and a coordinate within an ulp of a face can lie 1e-10 units outside it.
constexpr double kVoxelGuard = 1.0e-6;
constexpr float kCell = 65536.f;  // one voxel in mirror units
KICP_HD bool voxel_frac_is_safe(double frac) { return !(fabs(frac - 0.5) > 0.5 - kVoxelGuard); }
KICP_HD int32_t voxel_coord(double c, double vs, double inv_vs) {
    const double t = c * inv_vs;
    const double f = floor(t);
    if (__builtin_expect(!voxel_frac_is_safe(t - f), 0)) return static_cast<int32_t>(floor(c / vs));
    return static_cast<int32_t>(f);
}
struct VoxelCoord {
    int32_t v;
    float off;
};
KICP_HD VoxelCoord voxel_coord_offset(double c, double vs, double inv_vs, double upm) {
    const double t = c * inv_vs;
    const double f = floor(t);
    const double frac = t - f;
    if (__builtin_expect(!voxel_frac_is_safe(frac), 0)) {
        const int32_t v = static_cast<int32_t>(floor(c / vs));
        return VoxelCoord{v, fminf(fmaxf(static_cast<float>((c - v * vs) * upm), 0.f), 65535.99609375f)};
    }
    return VoxelCoord{static_cast<int32_t>(f), static_cast<float>(frac) * kCell};
}

// What a bucket visit needs to know about the query it serves (a lane may visit on behalf of another lane's query).
struct Probe {
    float lx, ly, lz;  // the query's offset inside its own voxel, mirror units
    uint32_t slot0;    // table slot of the own voxel's entry (its record lists the 27 neighbours' buckets)
};
// One query's search state.
struct Lane {
    uint32_t i;  // query index, kNoIndex32 = none
    Probe q;
    uint32_t todo;  // neighbour voxels still to visit (bit s = shift s of the reference's order)
    Best3 t;
};

// the transformed point T * source[i] and its voxel (PointToVoxel); recomputed where needed rather than kept in registers
// (`kept`: the latency-oriented build has the registers to keep the query and the two source coordinates the Jacobian needs
// through the search, and so starts its exact phase without re-reading the source point: -0.5 us per cfg2 scan)
struct KeptQuery {
    Query q;
    double sx, sy;
    bool voxel;  // q.vx .. q.vz are valid (a query parked in LDS comes back without them: only the rare exact search needs them)
};
// (`src`: the scan's points - p.src, or the scan a resident kernel was told to take up next, kicp_small.hpp)
// (`probe`: a search starts here - the offsets inside the voxel come with the voxel, voxel_coord_offset)
__device__ __forceinline__ void make_query_of(Query &q, const PassParams &p, const double *__restrict__ src, const Pose &T, uint32_t i, KeptQuery *kept = nullptr,
                                              Probe *probe = nullptr) {
    const double sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
    if (kept) kept->sx = sx, kept->sy = sy;
    double rx, ry, rz;
    quat_rotate(T, sx, sy, sz, rx, ry, rz);
    q.x = rx + T.tx, q.y = ry + T.ty, q.z = rz + T.tz;
    const double vs = p.map.voxel_size;
    if (probe) {
        const VoxelCoord x = voxel_coord_offset(q.x, vs, p.search.inv_vs, p.search.upm), y = voxel_coord_offset(q.y, vs, p.search.inv_vs, p.search.upm),
                         z = voxel_coord_offset(q.z, vs, p.search.inv_vs, p.search.upm);
        q.vx = x.v, q.vy = y.v, q.vz = z.v;
        probe->lx = x.off, probe->ly = y.off, probe->lz = z.off;
    } else {
        q.vx = voxel_coord(q.x, vs, p.search.inv_vs), q.vy = voxel_coord(q.y, vs, p.search.inv_vs), q.vz = voxel_coord(q.z, vs, p.search.inv_vs);
    }
}
// Everything the search does is in MIRROR UNITS (voxel_size / 65536) until the exact phase.  Error model (units): a mirror
// coordinate is within 1.0 of the true offset (rounding 0.5; 1.0 where the top of the range is clamped), the query offset and
// the difference add < 0.05 (fp32 roundings of numbers < 2^18), so a squared distance D is off by <= 2 sqrt(3 D) 1.05 + 3.3,
// plus 4.2e-6 D for the fp32 squares / sums and the 5 mantissa bits dropped for the integer tournament.  sp.margin_u covers
// the errors of BOTH candidates of a decision with 10 % to spare, for D up to the acceptance bound (and never farther than
// the 27-voxel neighbourhood reaches, D <= 12 voxel sizes^2): computed on the host (search_params()).
// The query offset is frac = t - floor(t) of t = c (1 / vs), times 65536 (voxel_coord_offset): t carries two roundings, 2.2e-16 |t|,
// which is <= 1.5e-5 units for |t| <= 2^20 (the subtraction is exact), and the conversion to fp32 with its product <= 0.004 (half
// an ulp of a number < 2^16; so is the clamp of the division's branch) - together well inside the 0.05 above.
template <bool OWN_VAL>
__device__ __forceinline__ void start_lane(Lane &L, const PassParams &p, const double *__restrict__ src, const Pose &T, uint32_t i, bool valid, uint32_t &own_val,
                                           KeptQuery *kept = nullptr) {  // OWN_VAL: the caller wants the probe's `own_val`
    const SearchParams &sp = p.search;
    L.i = valid ? i : kNoIndex32;
    L.q.slot0 = 0u, L.todo = 0u;
    L.t = Best3{sp.bound_u, sp.bound_u, sp.bound_u, kNoIndex32, kNoIndex32, 0u, 0u};
    Query q;
    make_query_of(q, p, src, T, valid ? i : 0u, kept, &L.q);
    if (kept) kept->q = q, kept->voxel = true;
    // ONE probe at the own voxel: the occupancy mask of the 27 neighbours (bit s = shift s of the reference's order) and
    // the record of their buckets.  Only voxels that hold points are ever visited; empty space costs nothing.
    // (`own_val`: the entry's own bucket value, for a first round that visits the own voxel straight from the probe - visit_first)
    own_val = 0u;
    if (valid && dbg_not(p, 2)) table_lookup_entry<OWN_VAL>(p.map, q.vx, q.vy, q.vz, L.q.slot0, L.todo, own_val);
    if (dbg_is(p, 3)) L.todo &= 1u;     // experiments: own voxel only
    if (dbg_is(p, 5)) L.todo &= 0x7Fu;  // own + faces
    if (dbg_is(p, 4)) L.todo = 0u;      // probe only, no bucket visit
}
__device__ __forceinline__ void start_lane(Lane &L, const PassParams &p, const double *__restrict__ src, const Pose &T, uint32_t i, bool valid, KeptQuery *kept = nullptr) {
    uint32_t own_val;  // (not wanted)
    start_lane<false>(L, p, src, T, i, valid, own_val, kept);
}
// drop the neighbour voxels that cannot hold anything within the margin of `best` (units^2).  A voxel's lower bound is the sum of
// the squared distances to the faces crossed on the way to it (one term for the six face neighbours, two for the twelve edge
// neighbours, three for the eight corners); it is alive while  sum <= (best + 4 margin) 1.00001  - the slack covers the fp32
// roundings of the sum and, per face crossed, the margin by which a mirror distance may undercut the truth (round 4 subtracted the
// margin per face: this bound is the same for corners and a hair more generous for faces and edges).
// Branch-free, and without a compare-and-select per voxel: the 26 differences `limit - sum` are formed two per instruction (packed
// fp32), and their SIGN BITS are shifted into the mask one v_alignbit_b32 each, last shift first.  ~50 instructions per round
// where the compare / select / or form took 125.
__device__ __forceinline__ uint32_t push_sign(uint32_t mask, float d) { return __builtin_amdgcn_alignbit(mask, __float_as_uint(d), 31u); }  // (mask << 1) | (d < 0)
__device__ __forceinline__ uint32_t cull_todo(const Lane &L, float best, float margin) {
    const Probe &P = L.q;
    const v2f x = {kCell - P.lx, P.lx}, y = {kCell - P.ly, P.ly}, z = {kCell - P.lz, P.lz};  // distances to the {+, -} faces of the own voxel
    const v2f fx = x * x, fy = y * y, fz = z * z;
    const float lim = (best + 4.0f * margin) * 1.00001f;
    const v2f A = {lim, lim};
    // reference order (kShiftTable): 0 own | 1 +x 2 -x 3 +y 4 -y 5 +z 6 -z | 7 ++0 8 +-0 9 -+0 10 --0 | 11 +0+ 12 +0- 13 -0+ 14 -0-
    // | 15 0++ 16 0+- 17 0-+ 18 0-- | 19 +++ 20 ++- 21 +-+ 22 +-- 23 -++ 24 -+- 25 --+ 26 ---
    const v2f dx = A - fx, dy = A - fy, dz = A - fz;                    // faces {1, 2} {3, 4} {5, 6}
    const v2f dxp = {dx.x, dx.x}, dxm = {dx.y, dx.y}, dyp = {dy.x, dy.x}, dym = {dy.y, dy.y};
    const v2f exy_p = dxp - fy, exy_m = dxm - fy;                        // xy edges {7, 8} {9, 10}
    const v2f exz_p = dxp - fz, exz_m = dxm - fz;                        // xz edges {11, 12} {13, 14}
    const v2f eyz_p = dyp - fz, eyz_m = dym - fz;                        // yz edges {15, 16} {17, 18}
    const v2f c_pp = v2f{exy_p.x, exy_p.x} - fz, c_pm = v2f{exy_p.y, exy_p.y} - fz;  // corners {19, 20} {21, 22}
    const v2f c_mp = v2f{exy_m.x, exy_m.x} - fz, c_mm = v2f{exy_m.y, exy_m.y} - fz;  //         {23, 24} {25, 26}
    uint32_t dead = 0u;
    dead = push_sign(push_sign(dead, c_mm.y), c_mm.x), dead = push_sign(push_sign(dead, c_mp.y), c_mp.x);
    dead = push_sign(push_sign(dead, c_pm.y), c_pm.x), dead = push_sign(push_sign(dead, c_pp.y), c_pp.x);
    dead = push_sign(push_sign(dead, eyz_m.y), eyz_m.x), dead = push_sign(push_sign(dead, eyz_p.y), eyz_p.x);
    dead = push_sign(push_sign(dead, exz_m.y), exz_m.x), dead = push_sign(push_sign(dead, exz_p.y), exz_p.x);
    dead = push_sign(push_sign(dead, exy_m.y), exy_m.x), dead = push_sign(push_sign(dead, exy_p.y), exy_p.x);
    dead = push_sign(push_sign(dead, dz.y), dz.x), dead = push_sign(push_sign(dead, dy.y), dy.x), dead = push_sign(push_sign(dead, dx.y), dx.x);
    return L.todo & ~(dead << 1);  // (bit 0, the own voxel, is always alive)
}
// One trip over N consecutive points of a mirror bucket, in two halves so that a caller can keep several trips in flight:
// load_trip issues the N / 2 16-byte loads at immediate offsets; process_trip turns the loaded words into distances in mirror
// units, finds the two smallest by an integer-key tournament and merges them into t.  `pos0` = position of the trip's first
// point inside the bucket.  process_trip returns whether the bucket goes on behind this trip (its last slot holds a point).
// PARTS = 2: two neighbouring lanes share the trip (the odd lane holds its last slot).
template <int N>
__device__ __forceinline__ void load_trip(const uint4 *bt, uint4 (&c)[N / 2]) {
#pragma unroll
    for (int u = 0; u < N / 2; ++u) c[u] = bt[u];
}
// FRESH: `t` is known to be the record a search starts from, {B, B, B, none, none, 0, 0} with B = the acceptance bound (start_lane),
// and this is a bucket's first trip: what the trip found is ASSIGNED (best3_assign_fresh), not merged.
template <int N, int PARTS, bool FRESH = false>
__device__ __forceinline__ bool process_trip(const uint4 (&c)[N / 2], uint32_t pos0, uint32_t base, int s, const v2f qx, const v2f qy, const v2f qz, Best3 &t,
                                             float margin) {
    // All distances first (independent), then the minimum as a tournament over integer keys: a non-negative
    // float orders like its bit pattern, so (bits & ~31) | position is one v_min3_u32 per three candidates
    // and yields value and position at once (unique keys: the lower position wins a tie, like the
    // reference's first minimum).  The 5 dropped mantissa bits are part of the margin's error model.
    // Empty slots need no test: their second word reads 4.3e9 units (kicp_common.hpp).  x and y are converted from their 16-bit
    // halves; z is stored as the float itself: no conversion, only a register copy per pair of points to bring the two z words of a
    // load into one register pair (profiles/mirror_z_ab.txt; a device layout that pairs the z words was built, measured and lost its
    // A/B: profiles/visit_trim_ab.txt).
    uint32_t key[N];
#pragma unroll
    for (int u = 0; u < N / 2; ++u) {
        const v2f px = {static_cast<float>(c[u].x & 0xffffu), static_cast<float>(c[u].z & 0xffffu)};
        const v2f py = {static_cast<float>(c[u].x >> 16), static_cast<float>(c[u].z >> 16)};
        const v2f pz = {mirror_word_z(c[u].y), mirror_word_z(c[u].w)};  // (the word IS the float: z, or far away for an empty slot)
        const v2f ddx = px - qx, ddy = py - qy, ddz = pz - qz;
        const v2f d = __builtin_elementwise_fma(ddz, ddz, __builtin_elementwise_fma(ddy, ddy, ddx * ddx));
        key[2 * u] = (__float_as_uint(d.x) & ~31u) | static_cast<uint32_t>(2 * u);
        key[2 * u + 1] = (__float_as_uint(d.y) & ~31u) | static_cast<uint32_t>(2 * u + 1);
    }
    // the bucket ends where a trip's last slot is empty (the pair of lanes of a shared bucket must agree: the odd lane
    // holds that slot - quad_perm [1, 1, 3, 3])
    uint32_t last_word = c[N / 2 - 1].w;
    if (PARTS == 2) last_word = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(last_word), 0xF5, 0xf, 0xf, false));
    const bool more = mirror_word_is_point(last_word);
    // winner and runner-up in one tournament (the keys are unique, so the runner-up is a different candidate)
    uint32_t key1, key2;
    tree_min2_u32<N>(key, key1, key2);
    const float m1 = __uint_as_float(key1 & ~31u);
    if (m1 <= t.b1 + margin) {  // something here can come within the margin of the running minimum
        // The third place is only worth a tournament when the runner-up lies within the margin of the winner; otherwise the
        // runner-up's value stands in for it (a lower bound that can never look like a near tie).  key - (key2 + 1) wraps to
        // the top of the range for the winner and the runner-up alone and keeps the order of all the others.
        uint32_t key3 = key2;
        if (__uint_as_float(min(key2, kFarKey) & ~31u) - m1 <= margin) {
            const uint32_t after2 = key2 + 1u;
#pragma unroll
            for (int u = 0; u < N; ++u) key[u] -= after2;
            key3 = after2 + tree_min_u32<N>(key);
        }
        const uint32_t k1 = pos0 + (key1 & 31u), k2 = pos0 + (key2 & 31u);  // positions within the bucket
        // with fewer than three points the far key stands in (finite, beyond every real distance)
        Best3 o{m1, __uint_as_float(min(key2, kFarKey) & ~31u), __uint_as_float(min(key3, kFarKey) & ~31u), base + k1,
                base + k2, static_cast<uint32_t>(s) * kOrdStride + k1, static_cast<uint32_t>(s) * kOrdStride + k2};
        if (FRESH) best3_assign_fresh(t, o);
        else best3_merge(t, o);
    }
    return more;
}
// the query as seen from the corner of neighbour voxel `s`, both lanes of the packed arithmetic
// (Reading the 27 triples shift x 65536 from a table in device memory - one 16-byte load per lane beside the load of nb[s] - takes 31
// VALU instructions per wave and block out of this and was SLOWER by the clock, cfg5 + 2.3 %: profiles/lane_start_ab.txt.  Not kept.)
// Per axis the value is l - d 65536 with d = the shift's component, -1, 0 or 1.  The order's components are packed once more for this
// (kFromX / Y / Z), two bits per shift that ARE the top two bits of the float -2 d: 00 -> 0, 01 -> 2.0 (d = -1), 11 -> -2.0 (d = 1).  A
// shift right by 2 s, a shift left by 30 (which drops the other shifts' bits: no mask) and one fma, l + (-2 d) 32768: the product is
// exact, so the sum is rounded once - the same float as l - d 65536 formed from the integer d (tests/cpp/query_from_test.cpp).  Three
// instructions per axis where extracting d, converting and multiplying it took six.
// (The equality holds for every finite l, negative ones included - one exact product, one rounding - with one exception that cannot
// matter: l = -0 with d = 0 gives +0 where the subtraction gave -0, and the value is only ever subtracted from and squared.)
constexpr uint64_t pack_axis_from(int axis) {
    uint64_t v = 0;
    for (int s = 0; s < 27; ++s) v |= static_cast<uint64_t>(kShiftTable[s][axis] > 0 ? 3 : (kShiftTable[s][axis] < 0 ? 1 : 0)) << (2 * s);
    return v;
}
constexpr uint64_t kFromX = pack_axis_from(0), kFromY = pack_axis_from(1), kFromZ = pack_axis_from(2);
KICP_HD float axis_from(float l, uint64_t packed, int s) {
    const float minus_two_d = __builtin_bit_cast(float, static_cast<uint32_t>(packed >> (2 * s)) << 30);
    return fmaf(minus_two_d, 0.5f * kCell, l);
}
struct QueryFrom {
    v2f x, y, z;
};
// COMPONENTS: the form before, from the integer components - the same floats.  visit_bucket of the pose-scoring kernels asks for it -
// the only visit those kernels compile (they have no written-out first round and are not the latency build, so visit_first and
// visit_two are dead code there): k_score_poses sits at 128 VGPRs and spilled two of them with the shorter form's schedule.  A second
// form of the same floats is kept for that reason alone; it can go as soon as k_score_poses has a register to spare.
template <bool COMPONENTS = false>
__device__ __forceinline__ QueryFrom query_from(const Probe &P, int s) {
    if constexpr (COMPONENTS) {
        const int dx = shift_component(kShiftX, s), dy = shift_component(kShiftY, s), dz = shift_component(kShiftZ, s);
        return QueryFrom{{P.lx - dx * kCell, P.lx - dx * kCell}, {P.ly - dy * kCell, P.ly - dy * kCell}, {P.lz - dz * kCell, P.lz - dz * kCell}};
    } else {
        const float x = axis_from(P.lx, kFromX, s), y = axis_from(P.ly, kFromY, s), z = axis_from(P.lz, kFromZ, s);
        return QueryFrom{{x, x}, {y, y}, {z, z}};
    }
}
// scan the bucket of neighbour voxel `s` of query P and merge what it finds into t.  PARTS = 2: two neighbouring lanes serve the
// same query and share every bucket - this lane takes points [10 part, 10 part + 10) of each 20-point trip (five 16-byte loads),
// the records are merged by the caller.
template <int PARTS, bool COMPONENTS = false>
__device__ __forceinline__ void visit_bucket(const Probe &P, Best3 &t, const MapView &m, int s, float margin, int part = 0) {
    static_assert(PARTS == 1 || PARTS == 2, "a trip is dealt to one lane or to two");
    constexpr int kMine = kTrip / PARTS;  // points of a trip this lane looks at
    // the neighbour's bucket comes out of the own voxel's record (same cache line as the probe): no second probe
    const uint32_t bucket = m.table[P.slot0].nb[s];
    const uint32_t base = bucket * m.cap;  // index into the fp64 pool
    const uint32_t stride16 = m.cap16;
    const uint4 *b = reinterpret_cast<const uint4 *>(m.pool16 + static_cast<size_t>(bucket) * stride16);
    const QueryFrom q = query_from<COMPONENTS>(P, s);
    const uint32_t first = static_cast<uint32_t>(part) * kMine;  // this lane's first point within a trip
    for (uint32_t k0 = 0; k0 < stride16; k0 += kTrip) {  // (the mirror's bucket stride is a multiple of kTrip: a trip never leaves the bucket)
        uint4 c[kMine / 2];
        load_trip<kMine>(b + (k0 + first) / 2, c);
        if (!process_trip<kMine, PARTS>(c, k0 + first, base, s, q.x, q.y, q.z, t, margin)) break;
    }
}
// The FIRST visit of a query, with the record start_lane left.  Where it goes to the own voxel (s == 0: two queries of three on a
// 64-beam scan) the bucket is the one the probe's entry names (`val`: no load of nb[0] behind the probe); a query whose own voxel
// holds no points reads its first neighbour's bucket from the entry's record as every later visit does.  The first trip's findings
// are assigned to the fresh record (process_trip FRESH); a bucket deeper than one trip (max_points_per_voxel > kTrip) goes on with
// the generic trip.
__device__ __forceinline__ void visit_first(const Probe &P, Best3 &t, const MapView &m, int s, uint32_t val, float margin) {
    uint32_t bucket = val_bucket(val, m.cbits);
    if (s != 0) bucket = m.table[P.slot0].nb[s];
    const uint32_t base = bucket * m.cap;
    const uint32_t stride16 = m.cap16;
    const uint4 *b = reinterpret_cast<const uint4 *>(m.pool16 + static_cast<size_t>(bucket) * stride16);
    const QueryFrom q = query_from(P, s);
    uint4 c[kTrip / 2];
    load_trip<kTrip>(b, c);
    bool more = process_trip<kTrip, 1, true>(c, 0u, base, s, q.x, q.y, q.z, t, margin);
    for (uint32_t k0 = kTrip; more && k0 < stride16; k0 += kTrip) {
        load_trip<kTrip>(b + k0 / 2, c);
        more = process_trip<kTrip, 1>(c, k0, base, s, q.x, q.y, q.z, t, margin);
    }
}
// Latency-oriented round (scans that leave the machine two waves per SIMD: every dependent memory access is ~0.9 us of a wave's
// ~12): TWO neighbour voxels per round.  Both bucket records and both buckets' first trips are in flight together; the first is
// decided, and the second is only looked at if its voxel can still hold something within the margin of the new minimum (its
// lower bound `lb2`, the same test cull_todo applies) - so the arithmetic saved by culling stays saved, only the wait is shared.
__device__ __forceinline__ void visit_two(const Probe &P, Best3 &t, const MapView &m, int s1, int s2, bool has2, float lb2, float margin) {
    const uint32_t bucket1 = m.table[P.slot0].nb[s1], bucket2 = has2 ? m.table[P.slot0].nb[s2] : 0u;
    const uint32_t stride16 = m.cap16;
    const uint4 *b1 = reinterpret_cast<const uint4 *>(m.pool16 + static_cast<size_t>(bucket1) * stride16);
    const uint4 *b2 = reinterpret_cast<const uint4 *>(m.pool16 + static_cast<size_t>(bucket2) * stride16);
    uint4 c1[kTrip / 2], c2[kTrip / 2];
    load_trip<kTrip>(b1, c1);
    if (has2) load_trip<kTrip>(b2, c2);
    const QueryFrom q1 = query_from(P, s1);
    bool more = process_trip<kTrip, 1>(c1, 0u, bucket1 * m.cap, s1, q1.x, q1.y, q1.z, t, margin);
    for (uint32_t k0 = kTrip; more && k0 < stride16; k0 += kTrip) {  // (deeper buckets than one trip: max_points_per_voxel > 20)
        load_trip<kTrip>(b1 + k0 / 2, c1);
        more = process_trip<kTrip, 1>(c1, k0, bucket1 * m.cap, s1, q1.x, q1.y, q1.z, t, margin);
    }
    if (has2 && lb2 <= t.b1 + margin) {
        const QueryFrom q2 = query_from(P, s2);
        more = process_trip<kTrip, 1>(c2, 0u, bucket2 * m.cap, s2, q2.x, q2.y, q2.z, t, margin);
        for (uint32_t k0 = kTrip; more && k0 < stride16; k0 += kTrip) {
            load_trip<kTrip>(b2 + k0 / 2, c2);
            more = process_trip<kTrip, 1>(c2, k0, bucket2 * m.cap, s2, q2.x, q2.y, q2.z, t, margin);
        }
    }
}
// lower bound (units^2, with cull_todo's slack) of the squared distance from query P to anything in neighbour voxel s
__device__ __forceinline__ float voxel_lower_bound(const Probe &P, int s, float margin) {
    const int dx = shift_component(kShiftX, s), dy = shift_component(kShiftY, s), dz = shift_component(kShiftZ, s);
    const float lx = dx > 0 ? kCell - P.lx : P.lx, ly = dy > 0 ? kCell - P.ly : P.ly, lz = dz > 0 ? kCell - P.lz : P.lz;
    float lb = 0.f;
    if (dx != 0) lb += lx * lx * 0.99999f - margin;
    if (dy != 0) lb += ly * ly * 0.99999f - margin;
    if (dz != 0) lb += lz * lz * 0.99999f - margin;
    return lb;
}

}  // namespace kicp
