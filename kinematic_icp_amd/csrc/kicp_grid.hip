// kicp_grid.hip -- the 2-D occupancy grid a mapping run draws beside its voxel map (kicp_grid_*; include/kicp.h states the semantics):
// per frame the used points' endpoint cells are HIT and the cells their rays cross are MISS, once per cell per frame.  Kernels:
// kicp_grid.hpp; the geometry they share with the host entries: kicp_grid_host.hpp.  The handle, and which file holds what a planner
// reads off the counters: kicp_grid_internal.hpp.  The grid scrolls (kicp_grid_scroll, kicp_grid_follow): kernel kicp_scroll.hpp,
// arithmetic kicp_scroll_host.hpp.
#include <cerrno>
#include <cstring>
#include <memory>

#include "kicp_grid.hpp"
#include "kicp_grid_internal.hpp"
#include "kicp_scroll.hpp"

namespace {
int check_thresholds(double occupied_thresh, double free_thresh) {
    if (!(0.0 <= free_thresh && free_thresh < occupied_thresh && occupied_thresh <= 1.0))
        return fail(KICP_ERR_ARG, "thresholds must satisfy 0 <= free_thresh < occupied_thresh <= 1");
    return KICP_OK;
}
constexpr size_t kFillCountWords = static_cast<size_t>(kGridFillShards) * kGridFillStride;  // the fill's sharded counts (kicp_grid.hpp)
int check_fill_config(const kicp_grid_fill_config *cfg, GridFillParams &p) {
    p = GridFillParams{cfg->min_observations, cfg->free_max, cfg->occupied_min};
    if (cfg->min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    if (!(cfg->free_max <= 100u && cfg->free_max < cfg->occupied_min && cfg->occupied_min <= 101u))
        return fail(KICP_ERR_ARG, "the fill needs free_max <= 100 and free_max < occupied_min <= 101");
    return KICP_OK;
}
// the frame at d_xyz (n points; arguments checked): three launches, the statistics back, the stream drained
int integrate_on_device(kicp_grid *grid, const double *d_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], unsigned long long out_stats[4]) {
    unsigned long long stats[4] = {0, n, 0, 0};
    const GridFrame f = grid_frame(grid->geom, pose_qt, sensor_xyz);
    grid->has_window = true, grid->win_x0 = f.gx0, grid->win_y0 = f.gy0;
    if (n) {
        hipStream_t st = grid->stream;
        auto &fr = grid->frame;
        if (n > fr.d_rays.capacity()) {
            HIP_TRY(hipStreamSynchronize(st));
            if (int rc = fr.d_rays.reserve(n + n / 2)) return rc;
        }
        HIP_TRY(hipMemsetAsync(fr.d_stats.get(), 0, 4 * sizeof(unsigned int), st));
        const uint32_t blocks = static_cast<uint32_t>((n + kGridBlock - 1) / kGridBlock);
        hipLaunchKernelGGL(k_grid_mark, dim3(blocks), dim3(kGridBlock), 0, st, d_xyz, static_cast<uint32_t>(n), grid->geom, f, fr.d_hit.get(), fr.d_rays.get(),
                           fr.d_stats.get());
        // one wave per ray, at most one ray per point; the waves of up to 2048 workgroups stride over the list, whose length is on the device
        hipLaunchKernelGGL(k_grid_rays, dim3(std::min(blocks, 2048u)), dim3(kGridBlock), 0, st, fr.d_rays.get(), fr.d_stats.get() + 3, grid->geom.reach,
                           reinterpret_cast<uint8_t *>(fr.d_miss.get()));
        hipLaunchKernelGGL(k_grid_apply, dim3((fr.plane_words + kGridBlock - 1) / kGridBlock), dim3(kGridBlock), 0, st, fr.d_hit.get(), fr.d_miss.get(), fr.plane_words,
                           grid->geom, f, grid->d_counts.get(), fr.d_stats.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(fr.h_stats.get(), fr.d_stats.get(), 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const unsigned int *h = fr.h_stats.get();
        stats[0] = h[0], stats[1] = n - h[0], stats[2] = h[1], stats[3] = h[2];
    }
    ++grid->frames;
    copy_stats(out_stats, stats);
    return KICP_OK;
}
int check_frame_args(const kicp_grid *grid, const double *xyz, size_t n, const double *pose_qt, const double *sensor_xyz) {
    return FrameUpload::check(grid && pose_qt && sensor_xyz && (xyz || !n), n, "frame too large");
}
int check_counts_rect(const kicp_grid *grid, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, size_t cap) {
    const unsigned int width = grid->cfg.width, height = grid->cfg.height;
    if (w < 1u || h < 1u || x0 >= width || y0 >= height || w > width - x0 || h > height - y0)
        return fail(KICP_ERR_ARG, "the rectangle must lie inside the grid of " + std::to_string(width) + " x " + std::to_string(height) + " cells, w and h at least 1");
    if (cap != static_cast<size_t>(w) * h) return fail(KICP_ERR_ARG, "the number of cells must be w * h = " + std::to_string(static_cast<size_t>(w) * h));
    return KICP_OK;
}
// The shift by (dx, dy), not both 0 (the handle checked): the counters and the transient plane, then the handle's bookkeeping; the
// stream drained.  Nothing of the map changes when it fails before the launches (with a plane, the counters' spare may by then be
// allocated while the plane's failed: it is kept for the next call); a failure behind them returns without the swap, so the handle keeps
// its counters and its origin.
int scroll_on_device(kicp_grid *grid, int dx, int dy) {
    kicp_grid_config &cfg = grid->cfg;
    const double origin_x = scroll_host::scroll_origin(cfg.origin_x, dx, cfg.cell), origin_y = scroll_host::scroll_origin(cfg.origin_y, dy, cfg.cell);
    if (!std::isfinite(origin_x) || !std::isfinite(origin_y)) return fail(KICP_ERR_ARG, "the origin after the shift is not finite");
    if (int rc = set_device(grid->device)) return rc;
    hipStream_t st = grid->stream;
    const bool plane = grid->d_transient_plane.get() != nullptr, empties = scroll_empties(cfg.width, cfg.height, dx, dy);
    if (empties) {  // nothing survives: no spare needed
        HIP_TRY(hipMemsetAsync(grid->d_counts.get(), 0, 2 * grid->cells * sizeof(uint16_t), st));
        if (plane) HIP_TRY(hipMemsetAsync(grid->d_transient_plane.get(), 0, grid->cells, st));
    } else {
        if (int rc = grid->d_counts_spare.reserve(2 * grid->cells)) return rc;
        if (plane)
            if (int rc = grid->d_transient_spare.reserve(grid->cells)) return rc;
        hipLaunchKernelGGL(k_scroll_plane<uint32_t>, dim3(scroll_blocks<uint32_t>(grid->cells)), dim3(kScrollBlock), 0, st,
                           reinterpret_cast<const uint32_t *>(grid->d_counts.get()), reinterpret_cast<uint32_t *>(grid->d_counts_spare.get()), cfg.width, cfg.height, dx, dy);
        if (plane)
            hipLaunchKernelGGL(k_scroll_plane<uint8_t>, dim3(scroll_blocks<uint8_t>(grid->cells)), dim3(kScrollBlock), 0, st, grid->d_transient_plane.get(),
                               grid->d_transient_spare.get(), cfg.width, cfg.height, dx, dy);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (!empties) {
        std::swap(grid->d_counts, grid->d_counts_spare);
        if (plane) std::swap(grid->d_transient_plane, grid->d_transient_spare);
    }
    cfg.origin_x = grid->geom.origin_x = origin_x, cfg.origin_y = grid->geom.origin_y = origin_y;
    if (grid->has_window) grid->has_window = scroll_host::scroll_window(grid->win_x0, grid->win_y0, dx, dy);
    grid->plan.valid = false;  // the plan's cells no longer mean what they meant
    return KICP_OK;
}
}  // namespace

extern "C" {

int kicp_grid_create(const kicp_grid_config *cfg, int device, kicp_grid **out) {
    KICP_TRACE_CALL();
    if (!cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    *out = nullptr;
    if (!(cfg->cell > 0.0) || !std::isfinite(cfg->cell)) return fail(KICP_ERR_ARG, "cell must be positive and finite");
    if (!(cfg->max_ray > 0.0) || !std::isfinite(cfg->max_ray)) return fail(KICP_ERR_ARG, "max_ray must be positive and finite");
    if (!std::isfinite(cfg->origin_x) || !std::isfinite(cfg->origin_y)) return fail(KICP_ERR_ARG, "the origin must be finite");
    if (!(cfg->z_min < cfg->z_max)) return fail(KICP_ERR_ARG, "the band needs z_min < z_max");
    if (cfg->width == 0 || cfg->height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    const unsigned long long cells = static_cast<unsigned long long>(cfg->width) * cfg->height;
    if (cells > kGridMaxCells)
        return fail(KICP_ERR_CAPACITY, "the grid would have " + std::to_string(cfg->width) + " x " + std::to_string(cfg->height) + " = " + std::to_string(cells) +
                                           " cells (limit 2^28 = " + std::to_string(kGridMaxCells) + ")");
    const double reach = std::ceil(cfg->max_ray / cfg->cell);
    if (!(reach <= static_cast<double>(kGridMaxReach)))
        return fail(KICP_ERR_CAPACITY, "max_ray / cell gives a reach of " + std::to_string(reach) + " cells (limit " + std::to_string(kGridMaxReach) + ")");
    if (int rc = set_device(device)) return rc;
    std::unique_ptr<kicp_grid> grid(new kicp_grid);
    grid->device = device, grid->cfg = *cfg, grid->cells = static_cast<size_t>(cells);
    grid->geom = GridGeom{cfg->cell, cfg->origin_x, cfg->origin_y, cfg->z_min, cfg->z_max, cfg->width, cfg->height, static_cast<int32_t>(reach)};
    auto &fr = grid->frame;
    const unsigned long long side = 2ull * static_cast<unsigned long long>(grid->geom.reach) + 1ull;
    fr.plane_words = static_cast<uint32_t>((side * side + 3ull) / 4ull);
    HIP_TRY(hipStreamCreateWithFlags(&grid->stream, hipStreamNonBlocking));
    if (int rc = grid->d_counts.reserve(2 * grid->cells)) return rc;
    if (int rc = fr.d_hit.reserve(fr.plane_words)) return rc;
    if (int rc = fr.d_miss.reserve(fr.plane_words)) return rc;
    if (int rc = fr.d_stats.reserve(4)) return rc;
    if (int rc = fr.h_stats.reserve(4, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemsetAsync(grid->d_counts.get(), 0, 2 * grid->cells * sizeof(uint16_t), grid->stream));
    HIP_TRY(hipMemsetAsync(fr.d_hit.get(), 0, fr.plane_words * sizeof(uint32_t), grid->stream));
    HIP_TRY(hipMemsetAsync(fr.d_miss.get(), 0, fr.plane_words * sizeof(uint32_t), grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    *out = grid.release();
    return KICP_OK;
}
void kicp_grid_destroy(kicp_grid *grid) {
    if (!grid) return;
    (void)hipSetDevice(grid->device);
    delete grid;
}
int kicp_grid_info(const kicp_grid *grid, kicp_grid_config *out_config, int *out_reach, unsigned long long *out_frames) {
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    if (out_config) *out_config = grid->cfg;
    if (out_reach) *out_reach = grid->geom.reach;
    if (out_frames) *out_frames = grid->frames;
    return KICP_OK;
}
int kicp_grid_clear(kicp_grid *grid) {
    KICP_TRACE_CALL();
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = set_device(grid->device)) return rc;
    HIP_TRY(hipMemsetAsync(grid->d_counts.get(), 0, 2 * grid->cells * sizeof(uint16_t), grid->stream));
    if (grid->d_transient_plane.get()) HIP_TRY(hipMemsetAsync(grid->d_transient_plane.get(), 0, grid->cells, grid->stream));  // (the switch stays as it is)
    HIP_TRY(hipStreamSynchronize(grid->stream));
    grid->frames = 0, grid->has_window = false;
    return KICP_OK;
}
int kicp_grid_integrate(kicp_grid *grid, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(grid, frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    if (int rc = grid->frame.upload.put(frame_xyz, n, grid->stream)) return rc;
    return integrate_on_device(grid, grid->frame.upload.d_xyz.get(), n, pose_qt, sensor_xyz, out_stats);
}
int kicp_grid_integrate_device(kicp_grid *grid, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                               unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(grid, d_frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    return integrate_on_device(grid, d_frame_xyz, n, pose_qt, sensor_xyz, out_stats);
}
int kicp_grid_counts(const kicp_grid *grid, unsigned short *out, size_t cap_cells) {
    KICP_TRACE_CALL();
    if (!grid || !out) return fail(KICP_ERR_ARG, "null argument");
    if (cap_cells != grid->cells) return fail(KICP_ERR_ARG, "cap_cells must be the grid's " + std::to_string(grid->cells) + " cells");
    if (int rc = set_device(grid->device)) return rc;
    HIP_TRY(hipMemcpyAsync(out, grid->d_counts.get(), 2 * grid->cells * sizeof(uint16_t), hipMemcpyDeviceToHost, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_set_counts(kicp_grid *grid, const unsigned short *in, size_t cells) {
    KICP_TRACE_CALL();
    if (!grid || !in) return fail(KICP_ERR_ARG, "null argument");
    if (cells != grid->cells) return fail(KICP_ERR_ARG, "cells must be the grid's " + std::to_string(grid->cells) + " cells");
    if (int rc = set_device(grid->device)) return rc;
    HIP_TRY(hipMemcpyAsync(grid->d_counts.get(), in, 2 * grid->cells * sizeof(uint16_t), hipMemcpyHostToDevice, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_counts_rect(const kicp_grid *grid, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, unsigned short *out, size_t cap_cells) {
    KICP_TRACE_CALL();
    if (!grid || !out) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_counts_rect(grid, x0, y0, w, h, cap_cells)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    constexpr size_t pair = 2 * sizeof(uint16_t);
    HIP_TRY(hipMemcpy2DAsync(out, w * pair, grid->d_counts.get() + 2 * (static_cast<size_t>(y0) * grid->cfg.width + x0), grid->cfg.width * pair, w * pair, h,
                             hipMemcpyDeviceToHost, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_set_counts_rect(kicp_grid *grid, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, const unsigned short *in, size_t cells) {
    KICP_TRACE_CALL();
    if (!grid || !in) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_counts_rect(grid, x0, y0, w, h, cells)) return rc;
    if (int rc = set_device(grid->device)) return rc;
    constexpr size_t pair = 2 * sizeof(uint16_t);
    HIP_TRY(hipMemcpy2DAsync(grid->d_counts.get() + 2 * (static_cast<size_t>(y0) * grid->cfg.width + x0), grid->cfg.width * pair, in, w * pair, w * pair, h,
                             hipMemcpyHostToDevice, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_scroll(kicp_grid *grid, int dx, int dy) {
    KICP_TRACE_CALL();
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    if (dx == 0 && dy == 0) return KICP_OK;
    return scroll_on_device(grid, dx, dy);
}
int kicp_grid_follow(kicp_grid *grid, double x, double y, unsigned int margin, unsigned int step, int *out_dx, int *out_dy) {
    KICP_TRACE_CALL();
    if (!grid) return fail(KICP_ERR_ARG, "null argument");
    const kicp_grid_config &cfg = grid->cfg;
    int32_t dx = 0, dy = 0;
    const int bad = scroll_host::follow_shifts(x, y, cfg.origin_x, cfg.origin_y, cfg.cell, cfg.width, cfg.height, margin, step, &dx, &dy);
    if (bad == 1) return fail(KICP_ERR_ARG, "the position must be finite and its cell within 2^30 cells of the grid's first");
    if (bad) return fail(KICP_ERR_ARG, "following needs margin >= 1, step >= 1 and 2 * margin + step <= width and height");
    if (dx != 0 || dy != 0)
        if (int rc = scroll_on_device(grid, dx, dy)) return rc;
    if (out_dx) *out_dx = dx;
    if (out_dy) *out_dy = dy;
    return KICP_OK;
}
int kicp_shift_plane(const void *in, void *out, unsigned int width, unsigned int height, unsigned int elem_bytes, int dx, int dy) {
    if (!in || !out) return fail(KICP_ERR_ARG, "null argument");
    if (elem_bytes != 1u && elem_bytes != 2u && elem_bytes != 4u && elem_bytes != 8u) return fail(KICP_ERR_ARG, "elem_bytes must be 1, 2, 4 or 8");
    if (int rc = check_grid_dims(width, height)) return rc;
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out), bytes = static_cast<uintptr_t>(width) * height * elem_bytes;
    if (a < b + bytes && b < a + bytes) return fail(KICP_ERR_ARG, "in and out must not overlap");
    scroll_host::shift_plane(in, out, width, height, elem_bytes, dx, dy);
    return KICP_OK;
}
int kicp_follow_shift(long long c, unsigned int size, unsigned int margin, unsigned int step, long long *d) {
    if (!d) return fail(KICP_ERR_ARG, "null argument");
    if (!scroll_host::follow_shift(c, size, margin, step, d))
        return fail(KICP_ERR_ARG, "following needs margin >= 1, step >= 1 and 2 * margin + step <= size (and a shift inside 64 bits)");
    return KICP_OK;
}
int kicp_grid_occupancy(const kicp_grid *grid, unsigned int min_observations, signed char *out, size_t cap_cells) {
    KICP_TRACE_CALL();
    if (!grid || !out) return fail(KICP_ERR_ARG, "null argument");
    if (min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    if (cap_cells != grid->cells) return fail(KICP_ERR_ARG, "cap_cells must be the grid's " + std::to_string(grid->cells) + " cells");
    if (int rc = set_device(grid->device)) return rc;
    DevBuf<int8_t> &d_occupancy = grid->readout.d_occupancy;
    if (int rc = d_occupancy.reserve(grid->cells)) return rc;
    hipLaunchKernelGGL(k_grid_readout, dim3(static_cast<uint32_t>((grid->cells + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, grid->stream,
                       grid->d_counts.get(), grid->cells, min_observations, d_occupancy.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_occupancy.get(), grid->cells, hipMemcpyDeviceToHost, grid->stream));
    HIP_TRY(hipStreamSynchronize(grid->stream));
    return KICP_OK;
}
int kicp_grid_occupancy_from_counts(const unsigned short *counts, size_t cells, unsigned int min_observations, signed char *out) {
    if ((!counts || !out) && cells) return fail(KICP_ERR_ARG, "null argument");
    if (min_observations < 1u) return fail(KICP_ERR_ARG, "min_observations must be at least 1");
    for (size_t i = 0; i < cells; ++i) out[i] = grid_readout(counts[2 * i], counts[2 * i + 1], min_observations);
    return KICP_OK;
}
int kicp_grid_fill_unknown(kicp_grid *dst, const kicp_grid *src, const kicp_grid_fill_config *cfg, unsigned long long out_counts[7]) {
    KICP_TRACE_CALL();
    if (!dst || !src || !cfg) return fail(KICP_ERR_ARG, "null argument");
    GridFillParams p;
    if (int rc = check_fill_config(cfg, p)) return rc;
    if (dst == src) return fail(KICP_ERR_ARG, "the destination and the source must be two grids");
    const kicp_grid_config &a = dst->cfg, &b = src->cfg;
    auto same_bits = [](double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; };
    if (!(same_bits(a.cell, b.cell) && same_bits(a.origin_x, b.origin_x) && same_bits(a.origin_y, b.origin_y) && a.width == b.width && a.height == b.height))
        return fail(KICP_ERR_ARG, "the two grids' cell, origin, width and height must be equal");
    if (dst->device != src->device)
        return fail(KICP_ERR_ARG, "the destination lives on device " + std::to_string(dst->device) + ", the source on device " + std::to_string(src->device));
    if (int rc = set_device(dst->device)) return rc;
    auto &fl = dst->fill;
    if (out_counts) {
        if (int rc = fl.d_counts.reserve(kFillCountWords)) return rc;
        if (int rc = fl.h_counts.reserve(kFillCountWords, hipHostMallocDefault, false)) return rc;
    }
    // Both handles' streams are idle (the stream rule); the launch runs on the destination's and is waited for.
    hipStream_t st = dst->stream;
    if (out_counts) HIP_TRY(hipMemsetAsync(fl.d_counts.get(), 0, kFillCountWords * sizeof(unsigned int), st));
    const uint32_t blocks = static_cast<uint32_t>(std::min<size_t>((dst->cells + kGridBlock - 1) / kGridBlock, kGridFillBlocks));
    hipLaunchKernelGGL(k_grid_fill_unknown, dim3(blocks), dim3(kGridBlock), 0, st, reinterpret_cast<uint32_t *>(dst->d_counts.get()),
                       reinterpret_cast<const uint32_t *>(src->d_counts.get()), static_cast<uint32_t>(dst->cells), p,
                       out_counts ? fl.d_counts.get() : static_cast<unsigned int *>(nullptr));
    HIP_TRY(hipGetLastError());
    if (out_counts) HIP_TRY(hipMemcpyAsync(fl.h_counts.get(), fl.d_counts.get(), kFillCountWords * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    dst->plan.valid = false;  // the plan was made on other counters: the fill is part of the chain that ends in a new one
    if (out_counts)
        for (uint32_t k = 0; k < kGridFillCounts; ++k) {
            out_counts[k] = 0;
            for (uint32_t shard = 0; shard < kGridFillShards; ++shard) out_counts[k] += fl.h_counts.get()[shard * kGridFillStride + k];
        }
    return KICP_OK;
}
int kicp_grid_fill_unknown_counts(unsigned short *dst_counts, const unsigned short *src_counts, size_t cells, const kicp_grid_fill_config *cfg,
                                  unsigned long long out_counts[7]) {
    if (!cfg || ((!dst_counts || !src_counts) && cells)) return fail(KICP_ERR_ARG, "null argument");
    GridFillParams p;
    if (int rc = check_fill_config(cfg, p)) return rc;
    if (dst_counts == src_counts && cells) return fail(KICP_ERR_ARG, "the destination and the source must be two grids");
    static_assert(sizeof(unsigned short) == sizeof(uint16_t), "a counter is 16 bits");
    grid_host::fill_unknown(dst_counts, src_counts, cells, p, out_counts);
    return KICP_OK;
}
int kicp_grid_last_window(const kicp_grid *grid, unsigned int *x0, unsigned int *y0, unsigned int *w, unsigned int *h) {
    if (!grid || !x0 || !y0 || !w || !h) return fail(KICP_ERR_ARG, "null argument");
    *x0 = *y0 = *w = *h = 0u;
    if (!grid->has_window) return KICP_OK;
    const int64_t side = 2 * static_cast<int64_t>(grid->geom.reach) + 1;
    const int64_t ax = std::max<int64_t>(grid->win_x0, 0), bx = std::min<int64_t>(grid->win_x0 + side, grid->cfg.width);
    const int64_t ay = std::max<int64_t>(grid->win_y0, 0), by = std::min<int64_t>(grid->win_y0 + side, grid->cfg.height);
    if (ax >= bx || ay >= by) return KICP_OK;
    *x0 = static_cast<unsigned int>(ax), *y0 = static_cast<unsigned int>(ay), *w = static_cast<unsigned int>(bx - ax), *h = static_cast<unsigned int>(by - ay);
    return KICP_OK;
}
int kicp_grid_write_map(const char *prefix, const signed char *occupancy, unsigned int width, unsigned int height, double cell, double origin_x, double origin_y,
                        double occupied_thresh, double free_thresh) {
    if (!prefix || !occupancy) return fail(KICP_ERR_ARG, "null argument");
    if (width == 0 || height == 0) return fail(KICP_ERR_ARG, "width and height must be at least 1");
    if (int rc = check_cell_origin(cell, origin_x, origin_y)) return rc;
    if (int rc = check_thresholds(occupied_thresh, free_thresh)) return rc;
    const std::string pgm = std::string(prefix) + ".pgm", yaml = std::string(prefix) + ".yaml";
    std::FILE *f = std::fopen(pgm.c_str(), "wb");
    if (!f) return fail(KICP_ERR_ARG, "cannot write " + pgm + ": " + std::strerror(errno));
    bool ok = std::fprintf(f, "P5\n%u %u\n255\n", width, height) > 0;
    std::vector<unsigned char> row(width);
    for (unsigned int iy = height; ok && iy-- > 0;) {  // the image's first row is the grid's highest iy
        for (unsigned int ix = 0; ix < width; ++ix) row[ix] = grid_pixel(occupancy[static_cast<size_t>(iy) * width + ix], occupied_thresh, free_thresh);
        ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
    }
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) return fail(KICP_ERR_ARG, "cannot write " + pgm + ": " + std::strerror(errno));
    f = std::fopen(yaml.c_str(), "wb");
    if (!f) return fail(KICP_ERR_ARG, "cannot write " + yaml + ": " + std::strerror(errno));
    const size_t slash = pgm.find_last_of('/');
    ok = std::fprintf(f, "image: %s\nmode: trinary\nresolution: %.17g\norigin: [%.17g, %.17g, 0]\nnegate: 0\noccupied_thresh: %.17g\nfree_thresh: %.17g\n",
                      pgm.c_str() + (slash == std::string::npos ? 0 : slash + 1), cell, origin_x, origin_y, occupied_thresh, free_thresh) > 0;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) return fail(KICP_ERR_ARG, "cannot write " + yaml + ": " + std::strerror(errno));
    return KICP_OK;
}
int kicp_grid_save_map(const kicp_grid *grid, const char *prefix, unsigned int min_observations, double occupied_thresh, double free_thresh) {
    KICP_TRACE_CALL();
    if (!grid || !prefix) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = check_thresholds(occupied_thresh, free_thresh)) return rc;
    std::vector<signed char> occupancy(grid->cells);
    if (int rc = kicp_grid_occupancy(grid, min_observations, occupancy.data(), grid->cells)) return rc;
    return kicp_grid_write_map(prefix, occupancy.data(), grid->cfg.width, grid->cfg.height, grid->cfg.cell, grid->cfg.origin_x, grid->cfg.origin_y, occupied_thresh,
                               free_thresh);
}

}  // extern "C"
