// kicp_elev.hip -- the height columns a mapping run keeps beside its occupancy grid (kicp_elev_*; include/kicp.h states the semantics):
// per cell one 64-bit column of the world heights that ever returned, and the traversability read off it - unknown, traversable,
// obstacle by height over the local ground; kicp_elev_update* also clear what a frame's rays pass through.  Kernels: kicp_elev.hpp; the arithmetic they share with the host entries:
// kicp_elev_host.hpp.  kicp_elev_to_grid writes the classes into a kicp_grid's counters, so this file sees that handle too.
#include <cstring>
#include <memory>
#include <utility>

#include "kicp_elev.hpp"
#include "kicp_grid_internal.hpp"
#include "kicp_scroll.hpp"

// The handle keeps the grid's rules (kicp_grid_internal.hpp): const entries write only the `mutable` group, and every entry returns
// with the stream drained.
struct kicp_elev {
    int device = 0;
    kicp_elev_config cfg{};
    ElevGeom geom{};
    size_t cells = 0;
    DevBuf<unsigned long long> d_columns;  // the layer: one column per cell
    DevBuf<unsigned long long> d_columns_spare;  // kicp_elev_scroll: what a shift writes into, swapped with d_columns afterwards; as kicp_grid's
    hipStream_t stream = nullptr;
    unsigned long long frames = 0;
    bool has_window = false;  // as kicp_grid's
    int32_t win_x0 = 0, win_y0 = 0;
    // kicp_elev_integrate*: skipped, outside_grid, outside_column, new_bits, new_cells of the frame in flight, in their shards
    struct {
        DevBuf<unsigned int> d_stats;
        PinnedBuf<unsigned int> h_stats;
        FrameUpload upload;  // kicp_elev_integrate's points
        DevBuf<unsigned long long> d_rays;  // kicp_elev_update*: the carve list, room for one record per point
    } frame;
    // kicp_elev_traversability*: the classes, the ground bytes and the four, five or six counts in their shards
    mutable struct {
        DevBuf<int8_t> d_classes;
        DevBuf<uint8_t> d_ground;
        DevBuf<unsigned int> d_counts;
        PinnedBuf<unsigned int> h_counts;
        DevBuf<long long> d_fit;  // kicp_elev_traversability_slope: D, Da, Db per cell; kicp_elev_traversability_rough: D, Da, Db, Q, n
    } readout;
    ~kicp_elev() {
        if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
    }
};

namespace {
constexpr int kElevStats = 5;  // words of a shard the mark kernel adds to
constexpr size_t kElevCountWords = static_cast<size_t>(kElevCountShards) * kElevCountStride;  // a sharded counter block (kicp_elev.hpp)
// word k of such a block as it came back, summed over the shards
unsigned long long shard_sum(const unsigned int *h, int k) {
    unsigned long long sum = 0;
    for (uint32_t shard = 0; shard < kElevCountShards; ++shard) sum += h[shard * kElevCountStride + k];
    return sum;
}

int check_elev_params(const kicp_elev_traversability_config *cfg, ElevParams &p) {
    p = ElevParams{cfg->step_slabs, cfg->robot_slabs};
    if (cfg->step_slabs > kElevMaxStep) return fail(KICP_ERR_ARG, "step_slabs must lie in 0 .. 62");
    if (!(cfg->step_slabs < cfg->robot_slabs && cfg->robot_slabs <= kElevSlabs)) return fail(KICP_ERR_ARG, "robot_slabs must satisfy step_slabs < robot_slabs <= 64");
    return KICP_OK;
}
int check_slope_config(const kicp_elev_slope_config *cfg, ElevSlopeParams &p) {
    p = ElevSlopeParams{cfg->radius_cells, cfg->gate_slabs, cfg->min_cells, cfg->rise_slabs, cfg->run_cells};
    if (cfg->radius_cells < 1u || cfg->radius_cells > kElevSlopeMaxRadius) return fail(KICP_ERR_ARG, "radius_cells must lie in 1 .. 8");
    if (cfg->gate_slabs > kElevSlopeMaxGate) return fail(KICP_ERR_ARG, "gate_slabs must lie in 0 .. 63");
    if (cfg->min_cells < kElevSlopeMinCells || cfg->min_cells > 289u) return fail(KICP_ERR_ARG, "min_cells must lie in 3 .. 289");
    if (cfg->rise_slabs > kElevSlopeMaxRatio) return fail(KICP_ERR_ARG, "rise_slabs must lie in 0 .. 65535");
    if (cfg->run_cells < 1u || cfg->run_cells > kElevSlopeMaxRatio) return fail(KICP_ERR_ARG, "run_cells must lie in 1 .. 65535");
    return KICP_OK;
}
int check_elev_rect(unsigned int width, unsigned int height, const ElevRect &r, size_t cap) {
    if (r.w < 1u || r.h < 1u || r.x0 >= width || r.y0 >= height || r.w > width - r.x0 || r.h > height - r.y0)
        return fail(KICP_ERR_ARG, "the rectangle must lie inside the layer of " + std::to_string(width) + " x " + std::to_string(height) + " cells, w and h at least 1");
    if (cap != static_cast<size_t>(r.w) * r.h) return fail(KICP_ERR_ARG, "cap must be w * h = " + std::to_string(static_cast<size_t>(r.w) * r.h));
    return KICP_OK;
}
// the layer's configuration as kicp_elev_create and the pure-host update take it -> the geometry and the number of cells
int check_elev_config(const kicp_elev_config *cfg, ElevGeom &geom, unsigned long long &cells) {
    if (!(cfg->cell > 0.0) || !std::isfinite(cfg->cell)) return fail(KICP_ERR_ARG, "cell must be positive and finite");
    if (!(cfg->max_ray > 0.0) || !std::isfinite(cfg->max_ray)) return fail(KICP_ERR_ARG, "max_ray must be positive and finite");
    if (!(cfg->slab > 0.0) || !std::isfinite(cfg->slab)) return fail(KICP_ERR_ARG, "slab must be positive and finite");
    if (!std::isfinite(cfg->origin_x) || !std::isfinite(cfg->origin_y) || !std::isfinite(cfg->z_origin)) return fail(KICP_ERR_ARG, "the origin and z_origin must be finite");
    if (cfg->width == 0 || cfg->height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    cells = static_cast<unsigned long long>(cfg->width) * cfg->height;
    if (cells > kGridMaxCells)
        return fail(KICP_ERR_CAPACITY, "the layer would have " + std::to_string(cfg->width) + " x " + std::to_string(cfg->height) + " = " + std::to_string(cells) +
                                           " cells (limit 2^28 = " + std::to_string(kGridMaxCells) + ")");
    const double reach = std::ceil(cfg->max_ray / cfg->cell);
    if (!(reach <= static_cast<double>(kGridMaxReach)))
        return fail(KICP_ERR_CAPACITY, "max_ray / cell gives a reach of " + std::to_string(reach) + " cells (limit " + std::to_string(kGridMaxReach) + ")");
    const double inf = std::numeric_limits<double>::infinity();
    geom = ElevGeom{GridGeom{cfg->cell, cfg->origin_x, cfg->origin_y, -inf, inf, cfg->width, cfg->height, static_cast<int32_t>(reach)}, cfg->z_origin, cfg->slab};
    return KICP_OK;
}
int check_carve_config(const kicp_elev_carve_config *cfg, ElevCarveParams &p) {
    p = ElevCarveParams{cfg->margin_steps, cfg->widen_slabs, cfg->keep_ground};
    if (cfg->widen_slabs > kElevMaxWiden) return fail(KICP_ERR_ARG, "widen_slabs must lie in 0 .. 64");
    if (cfg->keep_ground > 1u) return fail(KICP_ERR_ARG, "keep_ground must be 0 or 1");
    return KICP_OK;
}
// The frame at d_xyz (n points; arguments checked): the launches, the statistics back, the stream drained.  carve (nullable): an UPDATE -
// the list and the carve are launched in front of the mark, and out_stats has nine words, else six.
int integrate_on_device(kicp_elev *elev, const double *d_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], unsigned long long *out_stats,
                        const ElevCarveParams *carve = nullptr) {
    unsigned long long stats[KICP_ELEV_UPDATE_STATS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const ElevFrame f = elev_frame(elev->geom, pose_qt, sensor_xyz);
    elev->has_window = true, elev->win_x0 = f.plane.gx0, elev->win_y0 = f.plane.gy0;
    if (n) {
        hipStream_t st = elev->stream;
        auto &fr = elev->frame;
        const ElevCarveFrame cf = carve ? elev_carve_frame(elev->geom, f, sensor_xyz) : ElevCarveFrame{0, false};
        if (cf.carves && n > fr.d_rays.capacity()) {
            HIP_TRY(hipStreamSynchronize(st));
            if (int rc = fr.d_rays.reserve(n + n / 2)) return rc;
        }
        HIP_TRY(hipMemsetAsync(fr.d_stats.get(), 0, kElevCountWords * sizeof(unsigned int), st));
        if (cf.carves) {
            const uint32_t list_blocks = static_cast<uint32_t>((n + kElevBlock * kElevListPoints - 1) / (kElevBlock * kElevListPoints));
            hipLaunchKernelGGL(k_elev_list, dim3(list_blocks), dim3(kElevBlock), 0, st, d_xyz, static_cast<uint32_t>(n), elev->geom, f, fr.d_rays.get(), fr.d_stats.get());
            // One wave per ray, at most one ray per point: a wave for each of n rays, in up to 2048 workgroups whose waves stride over the
            // list - its length is on the device.  (Sized by points per workgroup, as k_grid_rays is, a 1 080-beam scan got 5 workgroups
            // for 1 080 rays of up to 500 steps: DESIGN 5i.)
            const uint32_t ray_blocks = static_cast<uint32_t>((n + kElevBlock / 64u - 1) / (kElevBlock / 64u));
            hipLaunchKernelGGL(k_elev_carve, dim3(std::min(ray_blocks, 2048u)), dim3(kElevBlock), 0, st, fr.d_rays.get(), fr.d_stats.get() + kElevListWord, elev->geom, f, cf.ss,
                               *carve, elev->d_columns.get(), fr.d_stats.get());
        }
        hipLaunchKernelGGL(k_elev_mark, dim3(static_cast<uint32_t>((n + kElevBlock - 1) / kElevBlock)), dim3(kElevBlock), 0, st, d_xyz, static_cast<uint32_t>(n), elev->geom,
                           f, elev->d_columns.get(), fr.d_stats.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(fr.h_stats.get(), fr.d_stats.get(), kElevCountWords * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int k = 0; k < kElevStats; ++k) stats[1 + k] = shard_sum(fr.h_stats.get(), k);
        stats[0] = n - (stats[1] + stats[2] + stats[3]);
        if (cf.carves) stats[6] = fr.h_stats.get()[kElevListWord], stats[7] = shard_sum(fr.h_stats.get(), 5), stats[8] = shard_sum(fr.h_stats.get(), 6);
    }
    ++elev->frames;
    if (out_stats)
        for (int k = 0; k < (carve ? KICP_ELEV_UPDATE_STATS : KICP_ELEV_STATS); ++k) out_stats[k] = stats[k];
    return KICP_OK;
}
int check_frame_args(const kicp_elev *elev, const double *xyz, size_t n, const double *pose_qt, const double *sensor_xyz) {
    return FrameUpload::check(elev && pose_qt && sensor_xyz && (xyz || !n), n, "frame too large");
}
// The shift by (dx, dy), not both 0 (the handle checked): as the grid's scroll_on_device (kicp_grid.hip), for the columns.
int scroll_on_device(kicp_elev *elev, int dx, int dy) {
    kicp_elev_config &cfg = elev->cfg;
    const double origin_x = scroll_host::scroll_origin(cfg.origin_x, dx, cfg.cell), origin_y = scroll_host::scroll_origin(cfg.origin_y, dy, cfg.cell);
    if (!std::isfinite(origin_x) || !std::isfinite(origin_y)) return fail(KICP_ERR_ARG, "the origin after the shift is not finite");
    if (int rc = set_device(elev->device)) return rc;
    const bool empties = scroll_empties(cfg.width, cfg.height, dx, dy);
    if (empties) {
        HIP_TRY(hipMemsetAsync(elev->d_columns.get(), 0, elev->cells * sizeof(unsigned long long), elev->stream));
    } else {
        if (int rc = elev->d_columns_spare.reserve(elev->cells)) return rc;
        hipLaunchKernelGGL(k_scroll_plane<unsigned long long>, dim3(scroll_blocks<unsigned long long>(elev->cells)), dim3(kScrollBlock), 0, elev->stream,
                           elev->d_columns.get(), elev->d_columns_spare.get(), cfg.width, cfg.height, dx, dy);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(elev->stream));
    if (!empties) std::swap(elev->d_columns, elev->d_columns_spare);
    cfg.origin_x = elev->geom.plane.origin_x = origin_x, cfg.origin_y = elev->geom.plane.origin_y = origin_y;
    if (elev->has_window) elev->has_window = scroll_host::scroll_window(elev->win_x0, elev->win_y0, dx, dy);
    return KICP_OK;
}
uint32_t elev_tiles(uint32_t cells_side) { return (cells_side + kElevTile - 1u) / kElevTile; }
int check_rough_config(const kicp_elev_rough_config *cfg, ElevRoughParams &p) {
    p = ElevRoughParams{cfg->num, cfg->den};
    if (cfg->num > kElevRoughMaxRatio) return fail(KICP_ERR_ARG, "num must lie in 0 .. 65535");
    if (cfg->den < 1u || cfg->den > kElevRoughMaxRatio) return fail(KICP_ERR_ARG, "den must lie in 1 .. 65535");
    return KICP_OK;
}
// The classes an entry reads out: the plain ones, with the slope limit (fit), with ROUGH too (fit and rough).
struct ElevClasses {
    ElevParams p{};
    ElevSlopeParams sp{};
    ElevRoughParams rp{};
    bool fit = false, rough = false;
    size_t fit_values() const { return !fit ? 0u : rough ? kElevFitValues<true> : kElevFitValues<false>; }  // per cell
    int counts() const { return !fit ? 4 : static_cast<int>(rough ? kElevFitCounts<true> : kElevFitCounts<false>); }
};
// cfg and, where the entry takes them (else null), slope and rough; an entry with rough has slope
int check_classes(const kicp_elev_traversability_config *cfg, const kicp_elev_slope_config *slope, const kicp_elev_rough_config *rough, ElevClasses &c) {
    c.fit = slope != nullptr, c.rough = rough != nullptr;
    if (int rc = check_elev_params(cfg, c.p)) return rc;
    if (slope)
        if (int rc = check_slope_config(slope, c.sp)) return rc;
    if (rough)
        if (int rc = check_rough_config(rough, c.rp)) return rc;
    return KICP_OK;
}
// The fit kernels' instantiations for L = radius (1 .. 8: check_slope_config), with and without ROUGH.
struct FitKernels {
    void (*readout)(const unsigned long long *, uint32_t, uint32_t, ElevParams, ElevSlopeParams, ElevRoughParams, ElevRect, uint32_t, int8_t *, uint8_t *, long long *, unsigned int *);
    void (*to_grid)(const unsigned long long *, uint32_t, uint32_t, ElevParams, ElevSlopeParams, ElevRoughParams, ElevRect, uint32_t, uint16_t *);
};
template <bool Rough, size_t... I>
FitKernels fit_kernels(uint32_t radius, std::index_sequence<I...>) {
    static const FitKernels k[] = {{k_elev_fit<static_cast<int>(I) + 1, Rough>, k_elev_fit_to_grid<static_cast<int>(I) + 1, Rough>}...};
    return k[radius - 1u];
}
FitKernels fit_kernels(const ElevClasses &c) {
    constexpr std::make_index_sequence<kElevSlopeMaxRadius> radii{};
    return c.rough ? fit_kernels<true>(c.sp.radius, radii) : fit_kernels<false>(c.sp.radius, radii);
}
// what kicp_elev_to_grid, kicp_elev_to_grid_slope and kicp_elev_to_grid_rough ask of the grid: the layer's plane, on the layer's device
int check_to_grid(const kicp_elev *elev, const kicp_grid *grid) {
    const kicp_grid_config &gc = grid->cfg;
    const kicp_elev_config &ec = elev->cfg;
    auto same_bits = [](double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; };
    if (!(same_bits(gc.cell, ec.cell) && same_bits(gc.origin_x, ec.origin_x) && same_bits(gc.origin_y, ec.origin_y) && gc.width == ec.width && gc.height == ec.height))
        return fail(KICP_ERR_ARG, "the grid's cell, origin, width and height must equal the layer's");
    if (grid->device != elev->device)
        return fail(KICP_ERR_ARG, "the grid lives on device " + std::to_string(grid->device) + ", the layer on device " + std::to_string(elev->device));
    return KICP_OK;
}
// The classes c of the rectangle r (arguments checked up to here) on the device: the launch, the results back, the stream drained.
// out_ground, out_fit (c.fit_values() per cell; null without a fit) and out_counts (c.counts() words) are nullable.
int readout_on_device(const kicp_elev *elev, const ElevClasses &c, const ElevRect &r, signed char *out, unsigned char *out_ground, long long *out_fit,
                      unsigned long long *out_counts, size_t cap) {
    if (int rc = check_elev_rect(elev->cfg.width, elev->cfg.height, r, cap)) return rc;
    if (int rc = set_device(elev->device)) return rc;
    auto &ro = elev->readout;
    const size_t fit_values = c.fit_values() * cap;
    if (int rc = ro.d_classes.reserve(cap)) return rc;
    if (out_ground)
        if (int rc = ro.d_ground.reserve(cap)) return rc;
    if (out_fit)
        if (int rc = ro.d_fit.reserve(fit_values)) return rc;
    if (out_counts) {
        if (int rc = ro.d_counts.reserve(kElevCountWords)) return rc;
        if (int rc = ro.h_counts.reserve(kElevCountWords, hipHostMallocDefault, false)) return rc;
    }
    hipStream_t st = elev->stream;
    if (out_counts) HIP_TRY(hipMemsetAsync(ro.d_counts.get(), 0, kElevCountWords * sizeof(unsigned int), st));
    const uint32_t tiles_x = elev_tiles(r.w), tiles_y = elev_tiles(r.h);  // (their product stays below 2^25: cells <= 2^28)
    uint8_t *d_ground = out_ground ? ro.d_ground.get() : nullptr;
    long long *d_fit = out_fit ? ro.d_fit.get() : nullptr;
    unsigned int *d_counts = out_counts ? ro.d_counts.get() : nullptr;
    if (c.fit)
        hipLaunchKernelGGL(fit_kernels(c).readout, dim3(tiles_x * tiles_y), dim3(kElevBlock), 0, st, elev->d_columns.get(), elev->cfg.width, elev->cfg.height, c.p, c.sp, c.rp, r,
                           tiles_x, ro.d_classes.get(), d_ground, d_fit, d_counts);
    else
        hipLaunchKernelGGL(k_elev_classify, dim3(tiles_x * tiles_y), dim3(kElevBlock), 0, st, elev->d_columns.get(), elev->cfg.width, elev->cfg.height, c.p, r, tiles_x,
                           ro.d_classes.get(), d_ground, d_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ro.d_classes.get(), cap, hipMemcpyDeviceToHost, st));
    if (out_ground) HIP_TRY(hipMemcpyAsync(out_ground, ro.d_ground.get(), cap, hipMemcpyDeviceToHost, st));
    if (out_fit) HIP_TRY(hipMemcpyAsync(out_fit, ro.d_fit.get(), fit_values * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (out_counts) HIP_TRY(hipMemcpyAsync(ro.h_counts.get(), ro.d_counts.get(), kElevCountWords * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (out_counts)
        for (int k = 0; k < c.counts(); ++k) out_counts[k] = shard_sum(ro.h_counts.get(), k);
    return KICP_OK;
}
// The classes c of every cell into the grid's counters.  Both handles' streams are idle (the stream rule); the launch runs on the
// layer's and is waited for, so the grid's next entry finds its counters written.
int to_grid_on_device(const kicp_elev *elev, const ElevClasses &c, kicp_grid *grid) {
    if (int rc = check_to_grid(elev, grid)) return rc;
    if (int rc = set_device(elev->device)) return rc;
    const kicp_elev_config &ec = elev->cfg;
    const ElevRect r{0u, 0u, ec.width, ec.height};
    const uint32_t tiles_x = elev_tiles(ec.width), tiles_y = elev_tiles(ec.height);
    if (c.fit)
        hipLaunchKernelGGL(fit_kernels(c).to_grid, dim3(tiles_x * tiles_y), dim3(kElevBlock), 0, elev->stream, elev->d_columns.get(), ec.width, ec.height, c.p, c.sp, c.rp, r,
                           tiles_x, grid->d_counts.get());
    else
        hipLaunchKernelGGL(k_elev_to_grid, dim3(tiles_x * tiles_y), dim3(kElevBlock), 0, elev->stream, elev->d_columns.get(), ec.width, ec.height, c.p, r, tiles_x,
                           grid->d_counts.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(elev->stream));
    return KICP_OK;
}
// The classes c of the rectangle r of columns given on the host (the *_from_columns entries; c checked): the outputs as readout_on_device's.
int classify_columns(const unsigned long long *columns, unsigned int width, unsigned int height, const ElevClasses &c, const ElevRect &r, signed char *out,
                     unsigned char *out_ground, long long *out_fit, unsigned long long *out_counts, size_t cap) {
    if (int rc = check_grid_dims(width, height)) return rc;
    if (int rc = check_elev_rect(width, height, r, cap)) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "a column is 64 bits");
    const uint64_t *col = reinterpret_cast<const uint64_t *>(columns);
    int8_t *classes = reinterpret_cast<int8_t *>(out);
    if (!c.fit) elev_host::classify(col, width, height, c.p, r, classes, out_ground, out_counts);
    else if (!c.rough) elev_host::classify_fit<false>(col, width, height, c.p, c.sp, c.rp, r, classes, out_ground, out_fit, out_counts);
    else elev_host::classify_fit<true>(col, width, height, c.p, c.sp, c.rp, r, classes, out_ground, out_fit, out_counts);
    return KICP_OK;
}
}  // namespace

extern "C" {

int kicp_elev_create(const kicp_elev_config *cfg, int device, kicp_elev **out) {
    KICP_TRACE_CALL();
    if (!cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    *out = nullptr;
    ElevGeom geom;
    unsigned long long cells;
    if (int rc = check_elev_config(cfg, geom, cells)) return rc;
    if (int rc = set_device(device)) return rc;
    std::unique_ptr<kicp_elev> elev(new kicp_elev);
    elev->device = device, elev->cfg = *cfg, elev->cells = static_cast<size_t>(cells), elev->geom = geom;
    HIP_TRY(hipStreamCreateWithFlags(&elev->stream, hipStreamNonBlocking));
    if (int rc = elev->d_columns.reserve(elev->cells)) return rc;
    if (int rc = elev->frame.d_stats.reserve(kElevCountWords)) return rc;
    if (int rc = elev->frame.h_stats.reserve(kElevCountWords, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemsetAsync(elev->d_columns.get(), 0, elev->cells * sizeof(unsigned long long), elev->stream));
    HIP_TRY(hipStreamSynchronize(elev->stream));
    *out = elev.release();
    return KICP_OK;
}
void kicp_elev_destroy(kicp_elev *elev) {
    if (!elev) return;
    (void)hipSetDevice(elev->device);
    delete elev;
}
int kicp_elev_info(const kicp_elev *elev, kicp_elev_config *out_config, int *out_reach, unsigned long long *out_frames) {
    if (!elev) return fail(KICP_ERR_ARG, "null argument");
    if (out_config) *out_config = elev->cfg;
    if (out_reach) *out_reach = elev->geom.plane.reach;
    if (out_frames) *out_frames = elev->frames;
    return KICP_OK;
}
int kicp_elev_clear(kicp_elev *elev) {
    KICP_TRACE_CALL();
    if (!elev) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = set_device(elev->device)) return rc;
    HIP_TRY(hipMemsetAsync(elev->d_columns.get(), 0, elev->cells * sizeof(unsigned long long), elev->stream));
    HIP_TRY(hipStreamSynchronize(elev->stream));
    elev->frames = 0, elev->has_window = false;
    return KICP_OK;
}
int kicp_elev_integrate(kicp_elev *elev, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], unsigned long long out_stats[6]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(elev, frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (int rc = set_device(elev->device)) return rc;
    if (int rc = elev->frame.upload.put(frame_xyz, n, elev->stream)) return rc;
    return integrate_on_device(elev, elev->frame.upload.d_xyz.get(), n, pose_qt, sensor_xyz, out_stats);
}
int kicp_elev_integrate_device(kicp_elev *elev, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                               unsigned long long out_stats[6]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(elev, d_frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (int rc = set_device(elev->device)) return rc;
    return integrate_on_device(elev, d_frame_xyz, n, pose_qt, sensor_xyz, out_stats);
}
int kicp_elev_update(kicp_elev *elev, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], const kicp_elev_carve_config *carve_config,
                     unsigned long long out_stats[9]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(elev, frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (!carve_config) return fail(KICP_ERR_ARG, "null argument");
    ElevCarveParams p;
    if (int rc = check_carve_config(carve_config, p)) return rc;
    if (int rc = set_device(elev->device)) return rc;
    if (int rc = elev->frame.upload.put(frame_xyz, n, elev->stream)) return rc;
    return integrate_on_device(elev, elev->frame.upload.d_xyz.get(), n, pose_qt, sensor_xyz, out_stats, &p);
}
int kicp_elev_update_device(kicp_elev *elev, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                            const kicp_elev_carve_config *carve_config, unsigned long long out_stats[9]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(elev, d_frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (!carve_config) return fail(KICP_ERR_ARG, "null argument");
    ElevCarveParams p;
    if (int rc = check_carve_config(carve_config, p)) return rc;
    if (int rc = set_device(elev->device)) return rc;
    return integrate_on_device(elev, d_frame_xyz, n, pose_qt, sensor_xyz, out_stats, &p);
}
int kicp_elev_update_columns(const kicp_elev_config *config, unsigned long long *columns, size_t cells, const double *frame_xyz, size_t n, const double pose_qt[7],
                             const double sensor_xyz[3], const kicp_elev_carve_config *carve_config, unsigned long long out_stats[9]) {
    if (int rc = FrameUpload::check(config && columns && carve_config && pose_qt && sensor_xyz && (frame_xyz || !n), n, "frame too large")) return rc;
    ElevGeom geom;
    unsigned long long layer_cells;
    ElevCarveParams p;
    if (int rc = check_elev_config(config, geom, layer_cells)) return rc;
    if (int rc = check_carve_config(carve_config, p)) return rc;
    if (cells != layer_cells) return fail(KICP_ERR_ARG, "cells must be the layer's " + std::to_string(layer_cells) + " cells");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "a column is 64 bits");
    unsigned long long stats[KICP_ELEV_UPDATE_STATS];
    elev_host::update(geom, reinterpret_cast<uint64_t *>(columns), frame_xyz, n, pose_qt, sensor_xyz, p, stats);
    if (out_stats)
        for (int k = 0; k < KICP_ELEV_UPDATE_STATS; ++k) out_stats[k] = stats[k];
    return KICP_OK;
}
int kicp_elev_columns(const kicp_elev *elev, unsigned long long *out, size_t cap_cells) {
    KICP_TRACE_CALL();
    if (!elev || !out) return fail(KICP_ERR_ARG, "null argument");
    if (cap_cells != elev->cells) return fail(KICP_ERR_ARG, "cap_cells must be the layer's " + std::to_string(elev->cells) + " cells");
    if (int rc = set_device(elev->device)) return rc;
    HIP_TRY(hipMemcpyAsync(out, elev->d_columns.get(), elev->cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, elev->stream));
    HIP_TRY(hipStreamSynchronize(elev->stream));
    return KICP_OK;
}
int kicp_elev_set_columns(kicp_elev *elev, const unsigned long long *in, size_t cells) {
    KICP_TRACE_CALL();
    if (!elev || !in) return fail(KICP_ERR_ARG, "null argument");
    if (cells != elev->cells) return fail(KICP_ERR_ARG, "cells must be the layer's " + std::to_string(elev->cells) + " cells");
    if (int rc = set_device(elev->device)) return rc;
    HIP_TRY(hipMemcpyAsync(elev->d_columns.get(), in, elev->cells * sizeof(unsigned long long), hipMemcpyHostToDevice, elev->stream));
    HIP_TRY(hipStreamSynchronize(elev->stream));
    return KICP_OK;
}
int kicp_elev_scroll(kicp_elev *elev, int dx, int dy) {
    KICP_TRACE_CALL();
    if (!elev) return fail(KICP_ERR_ARG, "null argument");
    if (dx == 0 && dy == 0) return KICP_OK;
    return scroll_on_device(elev, dx, dy);
}
int kicp_elev_follow(kicp_elev *elev, double x, double y, unsigned int margin, unsigned int step, int *out_dx, int *out_dy) {
    KICP_TRACE_CALL();
    if (!elev) return fail(KICP_ERR_ARG, "null argument");
    const kicp_elev_config &cfg = elev->cfg;
    int32_t dx = 0, dy = 0;
    const int bad = scroll_host::follow_shifts(x, y, cfg.origin_x, cfg.origin_y, cfg.cell, cfg.width, cfg.height, margin, step, &dx, &dy);
    if (bad == 1) return fail(KICP_ERR_ARG, "the position must be finite and its cell within 2^30 cells of the layer's first");
    if (bad) return fail(KICP_ERR_ARG, "following needs margin >= 1, step >= 1 and 2 * margin + step <= width and height");
    if (dx != 0 || dy != 0)
        if (int rc = scroll_on_device(elev, dx, dy)) return rc;
    if (out_dx) *out_dx = dx;
    if (out_dy) *out_dy = dy;
    return KICP_OK;
}
int kicp_elev_last_window(const kicp_elev *elev, unsigned int *x0, unsigned int *y0, unsigned int *w, unsigned int *h) {
    if (!elev || !x0 || !y0 || !w || !h) return fail(KICP_ERR_ARG, "null argument");
    *x0 = *y0 = *w = *h = 0u;
    if (!elev->has_window) return KICP_OK;
    const int64_t side = 2 * static_cast<int64_t>(elev->geom.plane.reach) + 1;
    const int64_t ax = std::max<int64_t>(elev->win_x0, 0), bx = std::min<int64_t>(elev->win_x0 + side, elev->cfg.width);
    const int64_t ay = std::max<int64_t>(elev->win_y0, 0), by = std::min<int64_t>(elev->win_y0 + side, elev->cfg.height);
    if (ax >= bx || ay >= by) return KICP_OK;
    *x0 = static_cast<unsigned int>(ax), *y0 = static_cast<unsigned int>(ay), *w = static_cast<unsigned int>(bx - ax), *h = static_cast<unsigned int>(by - ay);
    return KICP_OK;
}
int kicp_elev_traversability(const kicp_elev *elev, const kicp_elev_traversability_config *cfg, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h,
                             signed char *out, unsigned char *out_ground, unsigned long long out_counts[4], size_t cap) {
    KICP_TRACE_CALL();
    if (!elev || !cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, nullptr, nullptr, c)) return rc;
    return readout_on_device(elev, c, ElevRect{x0, y0, w, h}, out, out_ground, nullptr, out_counts, cap);
}
int kicp_elev_traversability_from_columns(const unsigned long long *columns, unsigned int width, unsigned int height, const kicp_elev_traversability_config *cfg,
                                          unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, signed char *out, unsigned char *out_ground,
                                          unsigned long long out_counts[4], size_t cap) {
    if (!columns || !cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, nullptr, nullptr, c)) return rc;
    return classify_columns(columns, width, height, c, ElevRect{x0, y0, w, h}, out, out_ground, nullptr, out_counts, cap);
}
int kicp_elev_to_grid(const kicp_elev *elev, const kicp_elev_traversability_config *cfg, kicp_grid *grid) {
    KICP_TRACE_CALL();
    if (!elev || !cfg || !grid) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, nullptr, nullptr, c)) return rc;
    return to_grid_on_device(elev, c, grid);
}
int kicp_elev_traversability_slope(const kicp_elev *elev, const kicp_elev_traversability_config *cfg, const kicp_elev_slope_config *slope, unsigned int x0,
                                   unsigned int y0, unsigned int w, unsigned int h, signed char *out, unsigned char *out_ground, long long *out_fit,
                                   unsigned long long out_counts[5], size_t cap) {
    KICP_TRACE_CALL();
    if (!elev || !cfg || !slope || !out) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, slope, nullptr, c)) return rc;
    return readout_on_device(elev, c, ElevRect{x0, y0, w, h}, out, out_ground, out_fit, out_counts, cap);
}
int kicp_elev_traversability_slope_from_columns(const unsigned long long *columns, unsigned int width, unsigned int height, const kicp_elev_traversability_config *cfg,
                                                const kicp_elev_slope_config *slope, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, signed char *out,
                                                unsigned char *out_ground, long long *out_fit, unsigned long long out_counts[5], size_t cap) {
    if (!columns || !cfg || !slope || !out) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, slope, nullptr, c)) return rc;
    return classify_columns(columns, width, height, c, ElevRect{x0, y0, w, h}, out, out_ground, out_fit, out_counts, cap);
}
int kicp_elev_to_grid_slope(const kicp_elev *elev, const kicp_elev_traversability_config *cfg, const kicp_elev_slope_config *slope, kicp_grid *grid) {
    KICP_TRACE_CALL();
    if (!elev || !cfg || !slope || !grid) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, slope, nullptr, c)) return rc;
    return to_grid_on_device(elev, c, grid);
}
int kicp_elev_traversability_rough(const kicp_elev *elev, const kicp_elev_traversability_config *cfg, const kicp_elev_slope_config *slope,
                                   const kicp_elev_rough_config *rough, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, signed char *out,
                                   unsigned char *out_ground, long long *out_fit, unsigned long long out_counts[6], size_t cap) {
    KICP_TRACE_CALL();
    if (!elev || !cfg || !slope || !rough || !out) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, slope, rough, c)) return rc;
    return readout_on_device(elev, c, ElevRect{x0, y0, w, h}, out, out_ground, out_fit, out_counts, cap);
}
int kicp_elev_traversability_rough_from_columns(const unsigned long long *columns, unsigned int width, unsigned int height, const kicp_elev_traversability_config *cfg,
                                                const kicp_elev_slope_config *slope, const kicp_elev_rough_config *rough, unsigned int x0, unsigned int y0,
                                                unsigned int w, unsigned int h, signed char *out, unsigned char *out_ground, long long *out_fit,
                                                unsigned long long out_counts[6], size_t cap) {
    if (!columns || !cfg || !slope || !rough || !out) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, slope, rough, c)) return rc;
    return classify_columns(columns, width, height, c, ElevRect{x0, y0, w, h}, out, out_ground, out_fit, out_counts, cap);
}
int kicp_elev_to_grid_rough(const kicp_elev *elev, const kicp_elev_traversability_config *cfg, const kicp_elev_slope_config *slope,
                            const kicp_elev_rough_config *rough, kicp_grid *grid) {
    KICP_TRACE_CALL();
    if (!elev || !cfg || !slope || !rough || !grid) return fail(KICP_ERR_ARG, "null argument");
    ElevClasses c;
    if (int rc = check_classes(cfg, slope, rough, c)) return rc;
    return to_grid_on_device(elev, c, grid);
}
int kicp_elev_rough_limit(const kicp_elev_config *config, double rms_metres, unsigned int *num, unsigned int *den) {
    if (!config || !num || !den) return fail(KICP_ERR_ARG, "null argument");
    if (!(config->slab > 0.0) || !std::isfinite(config->slab)) return fail(KICP_ERR_ARG, "slab must be positive and finite");
    const double limit = std::floor(((rms_metres / config->slab) * (rms_metres / config->slab)) * 1024.0);
    if (!(limit >= 0.0 && limit <= static_cast<double>(kElevRoughMaxRatio)))  // (a NaN fails both)
        return fail(KICP_ERR_ARG, "rms_metres gives a limit of " + std::to_string(limit) + " / 1024 slabs^2: it must be finite and lie in 0 .. 65535");
    *num = static_cast<unsigned int>(limit), *den = 1024u;
    return KICP_OK;
}
int kicp_elev_slope_limit(const kicp_elev_config *config, double max_tangent, unsigned int *rise_slabs, unsigned int *run_cells) {
    if (!config || !rise_slabs || !run_cells) return fail(KICP_ERR_ARG, "null argument");
    if (!(config->cell > 0.0) || !std::isfinite(config->cell) || !(config->slab > 0.0) || !std::isfinite(config->slab))
        return fail(KICP_ERR_ARG, "cell and slab must be positive and finite");
    const double rise = std::floor(((max_tangent * config->cell) / config->slab) * 1024.0);
    if (!(rise >= 0.0 && rise <= static_cast<double>(kElevSlopeMaxRatio)))  // (a NaN fails both)
        return fail(KICP_ERR_ARG, "max_tangent gives a rise of " + std::to_string(rise) + " slabs per 1024 cells: it must be finite and lie in 0 .. 65535");
    *rise_slabs = static_cast<unsigned int>(rise), *run_cells = 1024u;
    return KICP_OK;
}

}  // extern "C"
