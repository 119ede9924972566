// kicp_view.hip -- the depth view of a frame and the map sweep that reads it (kicp_view_*, kicp_map_remove_seen_through; include/kicp.h
// states the semantics): a cube map of Chebyshev depths around the sensor, faces aligned to the world axes, rendered from the frame the
// pipeline has just registered; a map point that the frame looks past - it lies in front of what the frame returned around its pixel,
// by more than a margin - leaves the map.  Kernels: kicp_view.hpp; geometry and verdict, shared with the host: kicp_view_host.hpp.
// A handle owns its stream, its frame upload (kicp_internal.hpp) and its device memory: the image, the sweep's voxel list and the statistics.
#include <memory>

#include "kicp_map_internal.hpp"  // dev_map
#include "kicp_view.hpp"

using namespace kicp;
using namespace kicp::host;

struct kicp_view {
    int device = 0;
    kicp_view_config cfg{};
    ViewGeom geom{};
    ViewFrame frame = view_no_frame();  // of the last rendered frame
    size_t pixels = 0;                  // 6 res^2
    unsigned long long frames = 0;
    hipStream_t stream = nullptr;
    DevBuf<uint32_t> d_depth;      // the image as float bit patterns
    DevBuf<unsigned int> d_stats;  // [0] points used by the render; [3] the length of d_list, [4 ..) the sweep's statistics, kSweepShards sets of four
    PinnedBuf<unsigned int> h_stats;
    FrameUpload upload;            // kicp_view_render's and kicp_view_classify's points; its staging buffer also serves the verdicts' download
    DevBuf<uint8_t> d_verdicts;    // kicp_view_classify's result
    DevBuf<uint32_t> d_list;       // the sweep's voxel list (slots)
    ~kicp_view() {
        if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
    }
};

namespace {
constexpr size_t kStatWords = 4 + 4 * kSweepShards;  // kicp_view::d_stats

// the frame at d_xyz (n points; arguments checked): the image emptied, one launch, the statistics back, the stream drained
int render_on_device(kicp_view *view, const double *d_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], unsigned long long out_stats[2]) {
    hipStream_t st = view->stream;
    view->frame = view_frame(pose_qt, sensor_xyz);
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(view->d_depth.get()), static_cast<int>(kViewEmptyBits), view->pixels, st));
    unsigned long long used = 0;
    if (n) {
        HIP_TRY(hipMemsetAsync(view->d_stats.get(), 0, sizeof(unsigned int), st));
        hipLaunchKernelGGL(k_view_render, dim3(static_cast<uint32_t>((n + kViewBlock - 1) / kViewBlock)), dim3(kViewBlock), 0, st, d_xyz, static_cast<uint32_t>(n),
                           view->geom, view->frame, view->d_depth.get(), view->d_stats.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(view->h_stats.get(), view->d_stats.get(), sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (n) used = view->h_stats.get()[0];
    ++view->frames;
    if (out_stats) out_stats[0] = used, out_stats[1] = n - used;
    return KICP_OK;
}
int check_frame_args(const kicp_view *view, const double *xyz, size_t n, const double *pose_qt, const double *sensor_xyz) {
    return FrameUpload::check(view && pose_qt && sensor_xyz && (xyz || !n), n, "frame too large");
}
int download_depth(const kicp_view *view, uint32_t *out) {
    HIP_TRY(hipMemcpyAsync(out, view->d_depth.get(), view->pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, view->stream));
    HIP_TRY(hipStreamSynchronize(view->stream));
    return KICP_OK;
}
}  // namespace

extern "C" {

int kicp_view_create(const kicp_view_config *cfg, int device, kicp_view **out) {
    KICP_TRACE_CALL();
    if (!cfg || !out) return fail(KICP_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->res > kViewMaxRes) return fail(KICP_ERR_CAPACITY, "res " + std::to_string(cfg->res) + " is beyond the limit of " + std::to_string(kViewMaxRes));
    if (cfg->window > kViewMaxWindow) return fail(KICP_ERR_CAPACITY, "window " + std::to_string(cfg->window) + " is beyond the limit of " + std::to_string(kViewMaxWindow));
    if (const char *why = view_config_error(cfg->res, cfg->window, cfg->min_rays, cfg->max_ray, cfg->margin, cfg->margin_per_metre)) return fail(KICP_ERR_ARG, why);
    if (int rc = set_device(device)) return rc;
    std::unique_ptr<kicp_view> view(new kicp_view);
    view->device = device, view->cfg = *cfg;
    view->geom = ViewGeom{cfg->res, cfg->window, cfg->min_rays, cfg->max_ray, cfg->margin, cfg->margin_per_metre};
    view->pixels = 6 * static_cast<size_t>(cfg->res) * cfg->res;
    HIP_TRY(hipStreamCreateWithFlags(&view->stream, hipStreamNonBlocking));
    if (int rc = view->d_depth.reserve(view->pixels)) return rc;
    if (int rc = view->d_stats.reserve(kStatWords)) return rc;
    if (int rc = view->h_stats.reserve(kStatWords, hipHostMallocDefault, false)) return rc;
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(view->d_depth.get()), static_cast<int>(kViewEmptyBits), view->pixels, view->stream));
    HIP_TRY(hipStreamSynchronize(view->stream));
    *out = view.release();
    return KICP_OK;
}
void kicp_view_destroy(kicp_view *view) {
    if (!view) return;
    (void)hipSetDevice(view->device);
    delete view;
}
int kicp_view_info(const kicp_view *view, kicp_view_config *out_config, double out_sensor_world[3], unsigned long long *out_frames) {
    if (!view) return fail(KICP_ERR_ARG, "null argument");
    if (out_config) *out_config = view->cfg;
    if (out_sensor_world) out_sensor_world[0] = view->frame.cx, out_sensor_world[1] = view->frame.cy, out_sensor_world[2] = view->frame.cz;
    if (out_frames) *out_frames = view->frames;
    return KICP_OK;
}
int kicp_view_render(kicp_view *view, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3], unsigned long long out_stats[2]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(view, frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (int rc = set_device(view->device)) return rc;
    if (int rc = view->upload.put(frame_xyz, n, view->stream)) return rc;
    return render_on_device(view, view->upload.d_xyz.get(), n, pose_qt, sensor_xyz, out_stats);
}
int kicp_view_render_device(kicp_view *view, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                            unsigned long long out_stats[2]) {
    KICP_TRACE_CALL();
    if (int rc = check_frame_args(view, d_frame_xyz, n, pose_qt, sensor_xyz)) return rc;
    if (int rc = set_device(view->device)) return rc;
    return render_on_device(view, d_frame_xyz, n, pose_qt, sensor_xyz, out_stats);
}
int kicp_view_depth(const kicp_view *view, float *out, size_t cap) {
    KICP_TRACE_CALL();
    if (!view || !out) return fail(KICP_ERR_ARG, "null argument");
    if (cap != view->pixels) return fail(KICP_ERR_ARG, "cap must be the view's 6 res^2 = " + std::to_string(view->pixels) + " pixels");
    if (int rc = set_device(view->device)) return rc;
    return download_depth(view, reinterpret_cast<uint32_t *>(out));
}
int kicp_view_classify(kicp_view *view, const double *points_xyz, size_t n, unsigned char *out) {
    KICP_TRACE_CALL();
    if (int rc = FrameUpload::check(view && ((points_xyz && out) || !n), n, "too many points")) return rc;
    if (!n) return KICP_OK;
    if (int rc = set_device(view->device)) return rc;
    if (int rc = view->upload.put(points_xyz, n, view->stream)) return rc;
    if (n > view->d_verdicts.capacity()) {
        HIP_TRY(hipStreamSynchronize(view->stream));
        if (int rc = view->d_verdicts.reserve(n + n / 2)) return rc;
    }
    hipLaunchKernelGGL(k_view_classify, dim3(static_cast<uint32_t>((n + kViewBlock - 1) / kViewBlock)), dim3(kViewBlock), 0, view->stream, view->upload.d_xyz.get(),
                       static_cast<uint32_t>(n), view->geom, view->frame, view->d_depth.get(), view->d_verdicts.get());
    HIP_TRY(hipGetLastError());
    return staged_download(view->upload.stage, out, view->d_verdicts.get(), n, view->stream);
}

int kicp_map_remove_seen_through(kicp_map *map, kicp_view *view, unsigned long long out_stats[4]) {
    KICP_TRACE_CALL();
    if (!map || !view) return fail(KICP_ERR_ARG, "null argument");
    if (int rc = map_finish_pending(map)) return rc;
    unsigned long long stats[4] = {0, 0, 0, 0};
    auto done = [&]() {
        if (out_stats)
            for (int k = 0; k < 4; ++k) out_stats[k] = stats[k];
        return KICP_OK;
    };
    if (view->frames == 0 || kicp_map_empty(map)) return done();  // nothing was seen / nothing to remove
    if (int rc = set_device(view->device)) return rc;
    if (map->host_updates_only || map->host.has_far_voxel()) {
        // a map whose updates stay on the host (a voxel the packed keys cannot express): the same verdict over the downloaded image
        if (int rc = ensure_host_current(map)) return rc;
        std::vector<uint32_t> depth(view->pixels);
        if (int rc = download_depth(view, depth.data())) return rc;
        view_host::sweep(view->geom, view->frame, depth.data(), map->host, stats);
        return done();
    }
    if (int rc = map_sync(map, view->device, nullptr)) return rc;
    DeviceMirror &mr = map->mirror;
    const size_t n_voxels = map->dev.n_voxels;
    if (n_voxels == 0) return done();
    hipStream_t st = nullptr;  // the map's kernels run on the null stream; the image is complete (the render drained its stream)
    if (n_voxels > view->d_list.capacity())
        if (int rc = view->d_list.reserve(n_voxels + n_voxels / 2)) return rc;
    const DevMap m = dev_map(*map);
    unsigned int *d_sweep = view->d_stats.get() + 4, *d_n_list = view->d_stats.get() + 3;
    HIP_TRY(hipMemsetAsync(d_n_list, 0, (kStatWords - 3) * sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_view_list, dim3(static_cast<uint32_t>(std::min<size_t>((mr.live_slots / 4 + kViewBlock - 1) / kViewBlock, 8192))), dim3(kViewBlock), 0, st, m, view->geom,
                       view->frame, view->d_list.get(), d_n_list);
    // one wave per listed voxel; the list's length is on the device, the host's voxel count bounds it
    hipLaunchKernelGGL(k_view_sweep, dim3(static_cast<uint32_t>((n_voxels + kSweepWaves - 1) / kSweepWaves)), dim3(64 * kSweepWaves), 0, st, m, view->geom, view->frame,
                       view->d_depth.get(), view->d_list.get(), d_n_list, d_sweep);
    HIP_TRY(hipGetLastError());
    DevMapCounters c{};
    HIP_TRY(hipMemcpyAsync(view->h_stats.get() + 4, d_sweep, 4 * kSweepShards * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&c, mr.d_ctr.get(), sizeof c, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    map->device_ahead = true;
    map->dev.n_points = c.n_points, map->dev.n_voxels = c.n_voxels, map->dev.free_count = c.free_count;
    for (uint32_t shard = 0; shard < kSweepShards; ++shard)
        for (int k = 0; k < 4; ++k) stats[k] += view->h_stats.get()[4 + 4 * shard + k];
    return done();
}

}  // extern "C"
