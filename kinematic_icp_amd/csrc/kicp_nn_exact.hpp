// kicp_nn_exact.hpp -- the plain fp64 nearest-neighbour search over the voxel table: kiss_icp::VoxelHashMap::GetClosestNeighbor (kiss-icp
// v1.2.0 core/VoxelHashMap.cpp) as the reference runs it - one probe per neighbour voxel, every bucket scanned in insertion order, the
// reference's rule on the rounded norms.  k_closest (kicp_map_kernels.hpp) runs it as it is; the pass kernels' mirror search
// (kicp_pass_visit.hpp) takes its probe and falls back on it where three candidates are too close to call (kicp_kernels.hpp).
#pragma once
#include "kicp_common.hpp"
#include "kicp_pass_params.hpp"

namespace kicp {

// ------------------------------------------------------------------------------------------------------------
// nearest-neighbour search helpers
// ------------------------------------------------------------------------------------------------------------
struct Query {
    double x, y, z;      // transformed point T*p
    int32_t vx, vy, vz;  // PointToVoxel(T*p)
};
// squared distances to the -/+ faces of the own voxel per axis, and the culling slack
struct Faces {
    double fm[3], fp[3];
    double slack;
};

__device__ __forceinline__ void make_query(Query &q, double x, double y, double z, double vs) {
    q.x = x, q.y = y, q.z = z;
    q.vx = static_cast<int32_t>(floor(x / vs)), q.vy = static_cast<int32_t>(floor(y / vs)), q.vz = static_cast<int32_t>(floor(z / vs));
}
__device__ __forceinline__ void make_faces(Faces &f, const Query &q, double vs) {
    const double lx = q.x - q.vx * vs, ly = q.y - q.vy * vs, lz = q.z - q.vz * vs;
    f.fm[0] = lx * lx, f.fm[1] = ly * ly, f.fm[2] = lz * lz;
    f.fp[0] = (vs - lx) * (vs - lx), f.fp[1] = (vs - ly) * (vs - ly), f.fp[2] = (vs - lz) * (vs - lz);
    // culling slack: far above fp64 rounding of the face distances, far below anything that matters
    f.slack = 4.0 * vs * 9.1e-13 * (fabs(q.x) + fabs(q.y) + fabs(q.z) + vs);
}

// lower bound of the squared distance from the query to any point of neighbour voxel (dx,dy,dz)
__device__ __forceinline__ double box_d2(const Faces &f, int dx, int dy, int dz) {
    double d = 0.0;
    d += dx > 0 ? f.fp[0] : (dx < 0 ? f.fm[0] : 0.0);
    d += dy > 0 ? f.fp[1] : (dy < 0 ? f.fm[1] : 0.0);
    d += dz > 0 ? f.fp[2] : (dz < 0 ? f.fm[2] : 0.0);
    return d;
}

// bucket value of voxel (x,y,z), or kEmptyVal when it holds no points (absent or halo entry)
__device__ __forceinline__ uint32_t table_lookup(const MapView &m, int32_t x, int32_t y, int32_t z) {
    uint32_t h = voxel_hash(x, y, z) & m.mask;
    for (;;) {
        const int4 e = *reinterpret_cast<const int4 *>(m.table + h);
        if (static_cast<uint32_t>(e.w) == kEmptyVal) return kEmptyVal;
        if (e.x == x && e.y == y && e.z == z) return val_count(static_cast<uint32_t>(e.w), m.cbits) ? static_cast<uint32_t>(e.w) : kEmptyVal;
        h = (h + 1) & m.mask;
    }
}
// the whole entry: bucket value and the 27-bit neighbour-occupancy mask (0 when the voxel has no entry at all,
// i.e. none of its 27 neighbours holds a point)
// slot index of the entry (for its nb[] record) and the 27-bit neighbour-occupancy mask; nbr == 0 when the voxel has
// no entry at all, i.e. none of its 27 neighbours holds a point.  `val`: the entry's own bucket value (a halo entry's where the voxel
// itself holds no points: bit 0 of nbr is clear then), for the caller that visits the own voxel without reading nb[0]
template <bool WITH_VAL>
__device__ __forceinline__ void table_lookup_entry(const MapView &m, int32_t x, int32_t y, int32_t z, uint32_t &slot, uint32_t &nbr, uint32_t &val) {
    uint32_t h = voxel_hash(x, y, z) & m.mask;
    for (;;) {
        int4 e = *reinterpret_cast<const int4 *>(m.table + h);
        uint32_t n = m.table[h].nbr;  // same cache line: issued together with the key
        // (all five words are wanted HERE: left to itself the compiler loads val, tests it, then loads the key, then nbr - three
        // round trips to one cache line in every wave's chain.  Only the build that asks for val is made to: the five registers
        // this holds at once are not free in every kernel that probes.)
        if (WITH_VAL) asm volatile("; the entry's key, val and nbr" : "+v"(e.x), "+v"(e.y), "+v"(e.z), "+v"(e.w), "+v"(n));
        if (static_cast<uint32_t>(e.w) == kEmptyVal) {
            slot = 0u, nbr = 0u;
            return;
        }
        if (e.x == x && e.y == y && e.z == z) {
            slot = h, nbr = n;
            if (WITH_VAL) val = static_cast<uint32_t>(e.w);
            return;
        }
        h = (h + 1) & m.mask;
    }
}

// `a` beats the running minimum `best` (both exact squared distances) under the reference's rule: kiss-icp compares
// (p - query).norm(), i.e. the ROUNDED SQUARE ROOTS, with strict '<' (std::min_element inside a voxel, `distance <
// closest_distance` across voxels - kiss-icp v1.2.0 core/VoxelHashMap.cpp GetClosestNeighbor), so a later candidate whose
// squared distance is smaller by an ulp or two but whose square root rounds to the same double does NOT replace the earlier
// one.  The square roots are only taken when the squared distances are that close (sqrt halves a relative difference: beyond
// 2^-50 the roots differ by more than their rounding).
__device__ __forceinline__ bool closer_by_norm(double a, double best) {
    if (!(a < best)) return false;
    if (a < best * (1.0 - 8.8817841970012523e-16)) return true;  // 1 - 2^-50
    return sqrt(a) < sqrt(best);
}
// `distance < max_correspondance_distance` (Registration.cpp:75) as the reference evaluates it - on the ROUNDED square root - without
// paying for the root where the squared distance is not within 2^-49 of tau^2: d2 < tau^2 (1 - 2^-49) makes the rounded root smaller
// than tau whatever the roundings of tau * tau and of the root (each 2^-53), d2 >= tau^2 (1 + 2^-49) makes it larger.
__device__ __forceinline__ bool accepted_by_norm(double d2, double tau, const SearchParams &sp) {
    if (d2 < sp.tau2_lo) return true;
    if (!(d2 < sp.tau2_hi)) return false;
    return sqrt(d2) < tau;
}
// scan one bucket in insertion order; strict '<' on the norms keeps the first minimum (std::min_element + `distance < closest`)
__device__ __forceinline__ void scan_points(const double *__restrict__ p, uint32_t count, uint32_t base_index, const Query &q,
                                            double &best, uint32_t &best_idx) {
    uint32_t k = 0;
    // ten, then four points per trip: all of a trip's loads in flight together, then the comparisons in insertion order (a bucket of
    // the default 20 points is two round trips to memory instead of ten)
    for (; k + 10 <= count; k += 10) {
        double c[30];
#pragma unroll
        for (int j = 0; j < 30; ++j) c[j] = p[3 * k + j];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const double dx = c[3 * j] - q.x, dy = c[3 * j + 1] - q.y, dz = c[3 * j + 2] - q.z;
            const double d2 = dx * dx + dy * dy + dz * dz;
            if (closer_by_norm(d2, best)) best = d2, best_idx = base_index + k + j;
        }
    }
    for (; k + 4 <= count; k += 4) {
        double c[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) c[j] = p[3 * k + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double dx = c[3 * j] - q.x, dy = c[3 * j + 1] - q.y, dz = c[3 * j + 2] - q.z;
            const double d2 = dx * dx + dy * dy + dz * dz;
            if (closer_by_norm(d2, best)) best = d2, best_idx = base_index + k + j;
        }
    }
    for (; k + 2 <= count; k += 2) {
        const double ax = p[3 * k], ay = p[3 * k + 1], az = p[3 * k + 2];
        const double bx = p[3 * k + 3], by = p[3 * k + 4], bz = p[3 * k + 5];
        const double adx = ax - q.x, ady = ay - q.y, adz = az - q.z;
        const double bdx = bx - q.x, bdy = by - q.y, bdz = bz - q.z;
        const double a2 = adx * adx + ady * ady + adz * adz;
        const double b2 = bdx * bdx + bdy * bdy + bdz * bdz;
        if (closer_by_norm(a2, best)) best = a2, best_idx = base_index + k;
        if (closer_by_norm(b2, best)) best = b2, best_idx = base_index + k + 1;
    }
    if (k < count) {
        const double dx = p[3 * k] - q.x, dy = p[3 * k + 1] - q.y, dz = p[3 * k + 2] - q.z;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (closer_by_norm(d2, best)) best = d2, best_idx = base_index + k;
    }
}

// 27-voxel 1-NN straight from HBM/L2.  `best` enters as the acceptance bound (or DBL_MAX).  `cull`: a squared distance some
// point of the map is KNOWN to have (the pre-selected winner's, exact) - voxels that cannot hold anything that close are skipped
// from the start; the winner is still chosen among everything that is visited, in visiting order, by the reference's rule.
__device__ __forceinline__ void search_global(const MapView &m, const Query &q, double &best, uint32_t &best_idx, double cull = 1.7976931348623157e308) {
    Faces f;
    make_faces(f, q, m.voxel_size);
#pragma unroll 1
    for (int s = 0; s < 27; ++s) {
        const int dx = shift_component(kShiftX, s), dy = shift_component(kShiftY, s), dz = shift_component(kShiftZ, s);
        if (box_d2(f, dx, dy, dz) > fmin(best, cull) + f.slack) continue;  // no point in there can beat `best` (or match `cull`)
        const uint32_t val = table_lookup(m, q.vx + dx, q.vy + dy, q.vz + dz);
        if (val == kEmptyVal) continue;
        const uint32_t bucket = val_bucket(val, m.cbits);
        scan_points(m.pool + static_cast<size_t>(bucket) * m.cap * 3, val_count(val, m.cbits), bucket * m.cap, q, best, best_idx);
    }
}

constexpr uint32_t kNoIndex32 = 0xFFFFFFFFu;
// exact fp64 evaluation of one candidate from the HBM pool
__device__ __forceinline__ double exact_d2_of(double tx, double ty, double tz, const Query &q) {
    const double dx = tx - q.x, dy = ty - q.y, dz = tz - q.z;
    return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ double exact_d2(const MapView &m, uint32_t gidx, const Query &q) {
    const double *t = m.pool + static_cast<size_t>(gidx) * 3;
    return exact_d2_of(t[0], t[1], t[2], q);
}

}  // namespace kicp
