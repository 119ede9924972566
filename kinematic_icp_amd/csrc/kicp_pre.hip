// kicp_pre.hip -- the pipeline's pre-steps behind include/kicp.h (kicp_pre_*): the handle, deskew + crop + transform, the voxel
// downsample, and the whole chain of one frame (kernels: kicp_pre.hpp).  The message's way in is kicp_pre_ingest.hip, the results'
// way back kicp_pre_egress.hip; kicp_pre_internal.hpp holds the handle and says which thread writes what.
#include <hip/hip_ext.h>  // hipExtLaunchKernelGGL: a launch with its own stop event

#include "kicp_pre_internal.hpp"
#include "kicp_pre.hpp"

namespace kicp {
namespace host {
int pre_ensure(kicp_pre *p, size_t n) {
    if (n <= p->cap_n) return KICP_OK;
    const size_t cap = n + n / 4 + 1024;
    if (int rc = ahead_join(p)) return rc;
    if (p->ahead.stream) HIP_TRY(hipStreamSynchronize(p->ahead.stream));
    p->ahead.state = 0;  // (a cloud waiting in the second slot goes with it: its kicp_pre_ingest call uploads it again)
    p->cap_n = 0;  // (until all twelve are in place: a failed growth is made up for by the next call)
    const size_t slots = reference_bucket_count(cap);  // >= the reference's bucket count for every frame of <= cap points
    if (int rc = p->d_in.reserve(cap * 3)) return rc;
    if (int rc = p->d_ts.reserve(cap)) return rc;
    if (int rc = p->ahead.d_in2.reserve(cap * 3)) return rc;
    if (int rc = p->ahead.d_ts2.reserve(cap)) return rc;
    if (int rc = p->d_staged.reserve(cap * 3)) return rc;
    if (int rc = p->d_flags.reserve(cap)) return rc;
    if (int rc = p->d_block_counts.reserve(std::max(cap, slots) / 256 + 2)) return rc;
    if (int rc = p->d_table.reserve(slots * 20)) return rc;
    if (int rc = p->d_table2.reserve(slots * 20)) return rc;
    if (int rc = p->d_counts1.reserve(slots / 256 + 2)) return rc;
    if (int rc = p->d_counts2.reserve(slots / 256 + 2)) return rc;
    if (int rc = p->d_block_minmax.reserve((cap / 256 + 2) * 2)) return rc;
    p->cap_n = cap, p->table_slots = slots, p->table_clean = false;
    return KICP_OK;
}
}  // namespace host
}  // namespace kicp
namespace {
int pre_ensure_buf(kicp_pre *p, int b, size_t n) {
    if (b == 2) p->egress.src_on_host = false;  // (every path that refills a buffer comes through here first)
    if (n <= p->buf[b].capacity() / 3) return KICP_OK;
    return p->buf[b].reserve((n + n / 4 + 1024) * 3);
}
// What a step or the chain brought back: the longest probe, the range flag, and the survivor counts `n[0 .. k)` of buffers dst0 ..
// dst0 + k - 1 (-> buf_n and, where given, out_n[0 .. k)).  `downsampled`: a table was filled and emptied again - it is clean behind
// a call without a range error, and a probe beyond the limit is worth a warning.
int pre_report(kicp_pre *p, uint32_t range_error, uint32_t max_probe, bool downsampled, int dst0, int k, const uint32_t *n, size_t *out_n) {
    p->last_max_probe = max_probe;
    if (range_error) {  // report once: the flag must not poison the calls that follow on this handle
        HIP_TRY(hipMemsetAsync(p->d_misc.get() + kMiscError, 0, 4, p->stream));
        return fail(KICP_ERR_CAPACITY, "a voxel coordinate left the +-2^20 range of the downsampling table");
    }
    for (int i = 0; i < k; ++i) {
        p->buf_n[dst0 + i] = n[i];
        if (out_n) out_n[i] = n[i];
    }
    if (!downsampled) return KICP_OK;
    p->table_clean = true;
    if (p->last_max_probe > p->probe_limit) {
        // The survivors are the reference's; their ORDER is only the reference's while its robin_map never grew mid-way, which it
        // does when a probe exceeds the container's limit - a re-hash the parallel replay does not model.  Say so instead of
        // handing out an order that may differ (the points are in place, the caller decides).
        last_error() = "VoxelDownsample: a robin-hood probe of " + std::to_string(p->last_max_probe) + " buckets exceeds the limit of " +
                       std::to_string(p->probe_limit) + " at which tsl::robin_map grows its table: the output ORDER may differ from the reference's";
        return KICP_WARN_TABLE_ORDER;
    }
    return KICP_OK;
}
// the survivor count (misc[0]) and the range flag (misc[1]) of the kernels queued so far -> buf_n[dst]
int pre_finish(kicp_pre *p, int dst, size_t *out_n, bool downsampled) {
    uint32_t misc[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(misc, p->d_misc.get(), sizeof misc, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return pre_report(p, misc[kMiscError], misc[kMiscProbe], downsampled, dst, 1, misc + kMiscTotal, out_n);
}
// exclusive scan of the first `nblocks` block counts in place, their sum to *total (grids beyond kFusedScanBlocks workgroups)
void scan_blocks(kicp_pre *p, uint32_t nblocks, uint32_t *total) {
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, p->stream, p->d_block_counts.get(), nblocks, total);
    ++p->scan_launches;
}
uint32_t tiles_of(size_t n) { return static_cast<uint32_t>((n + 255) / 256); }
// k_preprocess's arguments for what d_in / d_ts hold
PreprocessParams preprocess_params(const kicp_pre *p, size_t n, bool do_deskew, const double relative_motion_qt[7], const double lidar_to_base_qt[7],
                                   double max_range, double min_range) {
    PreprocessParams pp{};
    pp.in = p->d_in.get(), pp.timestamps = p->d_ts.get(), pp.n = static_cast<uint32_t>(n), pp.deskew = do_deskew ? 1 : 0;
    const Pose rel = pose_from(relative_motion_qt);
    pose_log(rel, pp.omega);
    pp.motion_inverse = pose_inverse(rel), pp.lidar_to_base = pose_from(lidar_to_base_qt);
    pp.max_range = max_range, pp.min_range = min_range;
    pp.ts_normalise = p->ingest.ts_raw ? 1 : 0, pp.ts_lo = p->ingest.ts_lo, pp.ts_hi = p->ingest.ts_hi;
    pp.flags = p->d_flags.get(), pp.staged = p->d_staged.get(), pp.block_counts = p->d_block_counts.get();
    return pp;
}
// k_preprocess, then the order-preserving compaction of what it staged into `out`, the survivor count to *total
void launch_preprocess(kicp_pre *p, const PreprocessParams &pp, uint32_t *total, double *out) {
    const uint32_t grid = tiles_of(pp.n);
    hipLaunchKernelGGL(k_preprocess, dim3(grid), dim3(256), 0, p->stream, pp);
    const int raw = grid <= kFusedScanBlocks ? 1 : 0;  // (frame-sized grids: every workgroup adds up the counts before it itself)
    if (!raw) scan_blocks(p, grid, total);
    hipLaunchKernelGGL(k_compact, dim3(grid), dim3(256), 0, p->stream, static_cast<const double *>(p->d_staged.get()), static_cast<const uint32_t *>(p->d_flags.get()),
                       static_cast<const uint32_t *>(p->d_block_counts.get()), raw, total, pp.n, out);
}
// k_preprocess over what d_in / d_ts hold, then compaction into buffer dst
int pre_run_preprocess(kicp_pre *p, size_t n, bool do_deskew, const double relative_motion_qt[7], const double lidar_to_base_qt[7],
                       double max_range, double min_range, int dst_buffer, size_t *out_n) {
    if (n == 0) {
        p->buf_n[dst_buffer] = 0;
        if (out_n) *out_n = 0;
        return KICP_OK;
    }
    if (int rc = pre_ensure_buf(p, dst_buffer, n)) return rc;
    launch_preprocess(p, preprocess_params(p, n, do_deskew, relative_motion_qt, lidar_to_base_qt, max_range, min_range), p->d_misc.get() + kMiscTotal, p->buf[dst_buffer].get());
    HIP_TRY(hipGetLastError());
    return pre_finish(p, dst_buffer, out_n, false);
}
// a caller's frame (and its stamps, where it is deskewed) into d_in / d_ts
int upload_frame(kicp_pre *p, const double *frame_xyz, size_t n, const double *timestamps, bool do_deskew) {
    if (int rc = pre_ensure(p, n)) return rc;
    p->ingest.valid = false, p->ingest.ts_raw = false;  // d_in / d_ts are overwritten (the caller's stamps are normalised already)
    if (int rc = stage_reserve(p->stage, n * 32, p->stream)) return rc;  // one buffer for both arrays
    if (int rc = staged_upload(p->stage, 0, p->d_in.get(), frame_xyz, n * 24, p->stream)) return rc;
    if (do_deskew)
        if (int rc = staged_upload(p->stage, n * 24, p->d_ts.get(), timestamps, n * 8, p->stream)) return rc;
    return KICP_OK;
}
// A downsampling table's four arrays inside its buffer, laid out for `slots` buckets: keys | min_index | order | home_at.  The layout
// depends on `slots`; "every byte 0xFF" is clean under every layout (keys free, no winner yet, buckets of the replay free).
DsTable table_at(unsigned char *base, size_t slots) {
    DsTable t{};
    t.keys = reinterpret_cast<unsigned long long *>(base);
    t.min_index = reinterpret_cast<uint32_t *>(base + slots * 8);
    t.order = t.min_index + slots, t.home_at = t.order + slots;
    return t;
}
// a frame of n points fits the tables the handle holds (`slots`: the reference's bucket count for n)
int table_fits(const kicp_pre *p, size_t n, size_t slots) {
    if (slots > p->table_slots || slots > 0x80000000ull || n > slots / 2)  // n > 2^24: float rounding in reserve() lets the reference re-hash mid-way
        return fail(KICP_ERR_CAPACITY, "frame too large for the downsampling table");
    return KICP_OK;
}
// all bytes of the table(s) 0xFF on the handle's stream
int wipe_tables(kicp_pre *p, bool both) {
    HIP_TRY(hipMemsetAsync(p->d_table.get(), 0xFF, p->table_slots * 20, p->stream));
    if (both) HIP_TRY(hipMemsetAsync(p->d_table2.get(), 0xFF, p->table_slots * 20, p->stream));
    return KICP_OK;
}
// the unfused downsample's arguments over table `t` (in, n / n_dev, voxel_size, mask: the caller's)
DownsampleParams downsample_params(const kicp_pre *p, const DsTable &t) {
    DownsampleParams dp{};
    dp.keys = t.keys, dp.min_index = t.min_index, dp.order = t.order, dp.home_at = t.home_at;
    dp.block_counts = p->d_block_counts.get(), dp.error = p->d_misc.get() + kMiscError, dp.probe_max = p->d_misc.get() + kMiscProbe;
    return dp;
}
// one downsample as three launches (and the scan, beyond kFusedScanBlocks tiles): claim over `grid` point tiles, replay and gather over
// `sgrid` bucket tiles; the survivors to `out`, their count to *total
void launch_downsample(kicp_pre *p, const DownsampleParams &dp, uint32_t grid, uint32_t sgrid, uint32_t *total, double *out) {
    hipLaunchKernelGGL(k_downsample_claim, dim3(grid), dim3(256), 0, p->stream, dp);
    hipLaunchKernelGGL(k_downsample_replay, dim3(sgrid), dim3(256), 0, p->stream, dp);
    const int raw = sgrid <= kFusedScanBlocks ? 1 : 0;
    if (!raw) scan_blocks(p, sgrid, total);
    hipLaunchKernelGGL(k_downsample_gather, dim3(sgrid), dim3(256), 0, p->stream, dp, static_cast<const uint32_t *>(p->d_block_counts.get()), raw, total, out);
}
}  // namespace
extern "C" {
int kicp_pre_create(int device, kicp_pre **out) {
    if (!out) return fail(KICP_ERR_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(KICP_ERR_HIP, "no HIP device visible: this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(KICP_ERR_ARG, "device index out of range");
    if (int rc = set_device(device)) return rc;
    kicp_pre *p = new kicp_pre;
    p->device = device;
    hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    int rc = KICP_OK;
    if (e == hipSuccess) rc = p->d_misc.reserve(kMiscWords);
    if (e == hipSuccess && !rc) rc = p->h_rec.reserve(kRecWords, hipHostMallocMapped | hipHostMallocCoherent, false);  // (the kernels take the host address)
    if (e == hipSuccess && !rc) rc = p->ingest.d_ticket.reserve(2);
    if (e == hipSuccess && !rc) rc = p->egress.d_push_tickets.reserve(kPushPieces);
    if (e == hipSuccess && !rc) {
        std::memset(p->h_rec.get(), 0, kRecWords * sizeof(unsigned long long));
        // The counters must read zero before the first kernel draws a ticket.  hipMemset of device memory may return before it has run,
        // and the handle's streams are non-blocking - nothing orders them behind the null stream: a first ingest that draws its ticket
        // ahead of the memset passes, the memset then wipes the count, and every later call of the handle waits for a last workgroup
        // that never comes ("finished without handing their result over").  So: on the handle's stream, and waited for here.
        e = hipMemsetAsync(p->d_misc.get(), 0, kMiscWords * 4, p->stream);
        if (e == hipSuccess) e = hipMemsetAsync(p->ingest.d_ticket.get(), 0, 16, p->stream);
        if (e == hipSuccess) e = hipMemsetAsync(p->egress.d_push_tickets.get(), 0, kPushPieces * 8, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&p->chain.ready, hipEventDisableTiming);
    }
    if (e != hipSuccess || rc) {
        kicp_pre_destroy(p);
        return fail(KICP_ERR_HIP, std::string("kicp_pre_create: ") + (rc ? last_error() : hipGetErrorString(e)));
    }
    *out = p;
    return KICP_OK;
}
void kicp_pre_destroy(kicp_pre *p) {
    if (!p) return;
    hipSetDevice(p->device);
    if (p->stream) hipStreamSynchronize(p->stream);
    (void)ahead_join(p);
    p->ahead.thread.stop();
    if (p->ahead.stream) hipStreamSynchronize(p->ahead.stream), hipStreamDestroy(p->ahead.stream);
    if (p->ingest.stream2) hipStreamSynchronize(p->ingest.stream2), hipStreamDestroy(p->ingest.stream2);
    egress_destroy(p);
    if (p->chain.ready) hipEventDestroy(p->chain.ready);
    if (p->stream) hipStreamDestroy(p->stream);
    delete p;  // (the buffers: every stream is synchronised, every helper thread joined)
}
int kicp_pre_preprocess(kicp_pre *p, const double *frame_xyz, size_t n, const double *timestamps, size_t n_timestamps,
                        const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range, double min_range,
                        int deskew, int dst_buffer, size_t *out_n) {
    KICP_TRACE_CALL();
    if (!p || (!frame_xyz && n) || !relative_motion_qt || !lidar_to_base_qt || dst_buffer < 0 || dst_buffer >= KICP_PRE_BUFFERS)
        return fail(KICP_ERR_ARG, "bad argument");
    const bool do_deskew = deskew && n_timestamps != 0;  // Preprocessing.cpp: `if (deskew_ && !timestamps.empty())`
    if (do_deskew && (!timestamps || n_timestamps < n)) return fail(KICP_ERR_ARG, "one timestamp per point is required for deskewing");
    if (int rc = set_device(p->device)) return rc;
    if (n > 0x7FFFFFF0ull / 3) return fail(KICP_ERR_CAPACITY, "frame too large");
    if (n)
        if (int rc = upload_frame(p, frame_xyz, n, timestamps, do_deskew)) return rc;
    return pre_run_preprocess(p, n, do_deskew, relative_motion_qt, lidar_to_base_qt, max_range, min_range, dst_buffer, out_n);
}
int kicp_pre_preprocess_ingested(kicp_pre *p, const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range,
                                 double min_range, int deskew, int dst_buffer, size_t *out_n) {
    KICP_TRACE_CALL();
    if (!p || !relative_motion_qt || !lidar_to_base_qt || dst_buffer < 0 || dst_buffer >= KICP_PRE_BUFFERS)
        return fail(KICP_ERR_ARG, "bad argument");
    if (!p->ingest.valid) return fail(KICP_ERR_ARG, "no ingested cloud: call kicp_pre_ingest first");
    if (int rc = set_device(p->device)) return rc;
    return pre_run_preprocess(p, p->ingest.n, deskew && p->ingest.stamps, relative_motion_qt, lidar_to_base_qt, max_range, min_range,
                              dst_buffer, out_n);
}
int kicp_pre_voxel_downsample(kicp_pre *p, int src, double voxel_size, int dst, size_t *out_n) {
    KICP_TRACE_CALL();
    if (!p || src < 0 || src >= KICP_PRE_BUFFERS || dst < 0 || dst >= KICP_PRE_BUFFERS || src == dst || !(voxel_size > 0.0))
        return fail(KICP_ERR_ARG, "bad argument");
    if (int rc = set_device(p->device)) return rc;
    const size_t n = p->buf_n[src];
    if (n == 0) {
        p->buf_n[dst] = 0;
        if (out_n) *out_n = 0;
        return KICP_OK;
    }
    if (int rc = pre_ensure(p, n)) return rc;
    if (int rc = pre_ensure_buf(p, dst, n)) return rc;
    // the reference's table: tsl::robin_map::reserve(frame.size()) buckets, ideal bucket = std::hash<Voxel> & mask (kicp_pre.hpp)
    const size_t slots = reference_bucket_count(n);
    if (int rc = table_fits(p, n, slots)) return rc;
    DownsampleParams dp = downsample_params(p, table_at(p->d_table.get(), slots));
    dp.in = p->buf[src].get(), dp.n = static_cast<uint32_t>(n), dp.voxel_size = voxel_size, dp.mask = static_cast<uint32_t>(slots - 1);
    // The gather step puts every bucket it has read back into the clean state, so only the first call after an allocation (or after
    // a failure) clears the table - one stream operation (~5 us) less per call.
    if (!p->table_clean)
        if (int rc = wipe_tables(p, false)) return rc;
    p->table_clean = false;  // (until this call is known to have run to its end)
    launch_downsample(p, dp, tiles_of(n), tiles_of(slots), p->d_misc.get() + kMiscTotal, p->buf[dst].get());
    HIP_TRY(hipGetLastError());
    return pre_finish(p, dst, out_n, true);
}
}  // extern "C"

// ---- the whole pre-step chain of one frame behind ONE host synchronisation (KinematicICP.cpp:54-62) ------------------------
// What d_in / d_ts hold (n_in points: an uploaded frame or an ingested cloud) is preprocessed into buffer 0, buffer 0 is
// downsampled into buffer 1 at `voxel_a`, buffer 1 into buffer 2 at `voxel_b`.  The survivor count of each step stays on the
// device and is the next step's input count (every launch is sized for n_in, every kernel derives the reference's bucket count
// from the real count itself); the three counts come back together at the end.  Buffer 0 - the preprocessed frame the pipeline
// returns - starts travelling to `out` (room for n_in points; may be nullptr) as soon as it is complete, on the download stream,
// while the downsamples run (f32: as x y z FLOAT32 records, k_push_frame_f32; buffer 2's host copy then holds records too).
namespace {
struct ChainCall {
    size_t n_in;
    uint32_t grid, sgrid;  // tiles of 256 points / of 256 buckets of the largest table the frame may need
    PreprocessParams pp;
    double voxel_a, voxel_b;
    void *out;  // the frame's landing area in caller memory (nullable), room for cap_points
    size_t cap_points;
    bool f32;
};
// Buffer 0 is complete behind the launch just queued: the event its way back waits for goes into the stream right here; everything
// else of that way - a dozen API calls, ~15 us of this thread (egress_start_frame) - waits until the chain's remaining launches are
// queued, so the device never idles on it.
int mark_frame_ready(kicp_pre *p, const ChainCall &c) {
    if (c.out) HIP_TRY(hipEventRecord(p->chain.ready, p->stream));
    return KICP_OK;
}
// table A's size is guessed from the last frame's survivor count, scaled with the frame (the first frame: from the input count - right
// whenever the crop leaves more than half of the points)
size_t chain_guess(const kicp_pre *p, size_t n_in) {
    size_t guess = n_in;
    if (p->chain.spec_n0 != 0 && p->chain.spec_n_in == 0) guess = std::min<size_t>(n_in, p->chain.spec_n0);
    if (p->chain.spec_n0 != 0 && p->chain.spec_n_in != 0)
        guess = std::min<size_t>(n_in, static_cast<size_t>(static_cast<double>(p->chain.spec_n0) * static_cast<double>(n_in) / static_cast<double>(p->chain.spec_n_in) + 0.5));
    return guess ? guess : n_in;
}
// FIVE launches (kicp_pre.hpp "the pre-steps of one frame in FIVE launches"), the frame's way back started beside them, and their
// record awaited: misc[1], [2], [4..6] as the unfused steps would return them; *unfused_tail: the guess was wrong, the downsamples have
// to run again from buffer 0 on
int chain_fused(kicp_pre *p, const ChainCall &c, uint32_t misc[8], bool *unfused_tail) {
    FrameParams f{};
    f.pre = c.pp;
    f.A = table_at(p->d_table.get(), p->table_slots), f.B = table_at(p->d_table2.get(), p->table_slots);
    f.voxel_a = c.voxel_a, f.voxel_b = c.voxel_b;
    f.spec_mask = static_cast<uint32_t>(reference_bucket_count(chain_guess(p, c.n_in)) - 1);
    f.tiles_pts = c.grid, f.tiles_spec = (f.spec_mask >> 8) + 1u;
    f.counts1 = p->d_counts1.get(), f.counts2 = p->d_counts2.get(), f.misc = p->d_misc.get();
    f.buf0 = p->buf[0].get(), f.buf1 = p->buf[1].get(), f.buf2 = p->buf[2].get();
    if (c.n_in * 24 > p->egress.h_src.capacity())
        if (int rc = p->egress.h_src.reserve(c.n_in * 24 + c.n_in * 6 + 4096, hipHostMallocDefault, false)) return rc;
    static const bool src_to_host = env_int("KICP_PRE_SRC_HOST", 1) != 0;
    f.host_buf2 = src_to_host ? reinterpret_cast<double *>(p->egress.h_src.dev()) : nullptr;
    f.host_buf2_f32 = c.f32 ? 1 : 0;
    f.host_rec = p->h_rec.get() + kRecChain, f.seq = ++p->chain.seq;
    if (f.seq == 0u) f.seq = ++p->chain.seq;  // (0 is what the device words hold before the first frame)
    // table B's size is known on the device only: its two launches walk the tiles there are with the workgroups they get - as
    // many as the previous frame's second table had tiles (twice that, for a frame that keeps more), sgrid at most
    const uint32_t grid_b = p->chain.spec_tiles_b ? std::min(c.sgrid, std::max(32u, 2u * p->chain.spec_tiles_b)) : std::min(c.sgrid, 1024u);
    hipLaunchKernelGGL(k_frame_pre, dim3(c.grid), dim3(256), 0, p->stream, f);
    // buffer 0 is complete behind the next launch: its way back starts beside the downsamples' remaining launches.  The event rides on
    // the launch's own completion signal (hipExtLaunchKernelGGL's stop event) where that is on - an event recorded behind the launch
    // is a packet of its own, and cost the device ~7 us between this launch and the next
    static const bool event_on_launch = env_flag("KICP_PRE_EVENT_ON_LAUNCH", true);
    if (event_on_launch && c.out) {
        hipExtLaunchKernelGGL(k_frame_l1_replay, dim3(std::max(c.grid, f.tiles_spec)), dim3(256), 0, p->stream, nullptr, p->chain.ready, 0, f);
    } else {
        hipLaunchKernelGGL(k_frame_l1_replay, dim3(std::max(c.grid, f.tiles_spec)), dim3(256), 0, p->stream, f);
        if (int rc = mark_frame_ready(p, c)) return rc;
    }
    hipLaunchKernelGGL(k_frame_l1_gather, dim3(f.tiles_spec), dim3(256), 0, p->stream, f);
    hipLaunchKernelGGL(k_frame_l2_replay, dim3(grid_b), dim3(256), 0, p->stream, f);
    hipLaunchKernelGGL(k_frame_l2_gather, dim3(grid_b), dim3(256), 0, p->stream, f);
    if (f.host_buf2) hipLaunchKernelGGL(k_frame_src_host, dim3(4), dim3(256), 0, p->stream, f);  // (nobody waits for it before kicp_pre_download(2))
    // (starting the frame's way back one, two or three launches later instead - the push's 3 MB of PCIe writes make the launches
    //  beside it 2-3 x as long, and the event costs the device 6 us between two launches - was measured: 1-4 % slower each)
    HIP_TRY(hipGetLastError());
    trace_lap("the frame's launches queued");
    if (int rc = egress_start_frame(p, c.n_in, c.out, c.cap_points, c.f32)) return rc;
    trace_lap("its way back queued");
    const unsigned long long tag = static_cast<unsigned long long>(f.seq) << 32, hi = 0xFFFFFFFF00000000ull;
    const volatile unsigned long long *rec = p->h_rec.get() + kRecChain;
    for (int w = 4; w >= 0; --w)
        if (int rc = wait_word(rec + w, tag, hi, p->stream, 2.0, kPreLost)) return rc;
    trace_lap("the chain's record at the host");
    ++p->chain.fused_frames;
    misc[4] = static_cast<uint32_t>(rec[0]), misc[5] = static_cast<uint32_t>(rec[1]), misc[6] = static_cast<uint32_t>(rec[2]);
    misc[kMiscProbe] = static_cast<uint32_t>(rec[3]), misc[kMiscError] = static_cast<uint32_t>(rec[4]) & 1u;
    *unfused_tail = (static_cast<uint32_t>(rec[4]) & 2u) != 0u;
    p->chain.spec_n0 = misc[4], p->chain.spec_n_in = static_cast<uint32_t>(c.n_in);
    p->egress.src_on_host = !*unfused_tail && f.host_buf2 != nullptr;
    p->egress.src_f32 = c.f32;
    p->egress.src_seq = f.seq;
    p->chain.spec_tiles_b = misc[5] ? static_cast<uint32_t>(reference_bucket_count(misc[5]) + 255) / 256u : 1u;
    p->chain.last_point_tiles = c.grid, p->chain.last_l1_tiles = f.tiles_spec, p->chain.last_l2_workgroups = grid_b;
    p->chain.last_l2_tiles = misc[5] ? ((reference_bucket_count_u32(misc[5]) - 1u) >> 8) + 1u : 0u;  // (the kernels' `tiles`, from the returned n1)
    if (*unfused_tail) {  // a guess was wrong: the tables hold claims made under the wrong size; buffer 0 and its count are in place
        ++p->chain.spec_misses;
        if (int rc = wipe_tables(p, true)) return rc;
    }
    return KICP_OK;
}
// the downsamples as three launches each, from buffer 0 on; every step's survivor count stays on the device as the next step's input
// count, and the words come back behind one synchronisation
int chain_unfused_tail(kicp_pre *p, const ChainCall &c, uint32_t misc[8]) {
    uint32_t *cnt = p->d_misc.get() + kMiscCounts;
    DownsampleParams dp = downsample_params(p, table_at(p->d_table.get(), p->table_slots));
    for (int stage = 0; stage < 2; ++stage) {
        dp.in = p->buf[stage].get(), dp.voxel_size = stage == 0 ? c.voxel_a : c.voxel_b, dp.n_dev = cnt + stage;
        dp.probe_max_sticky = stage == 0 ? nullptr : dp.probe_max;
        launch_downsample(p, dp, c.grid, c.sgrid, cnt + stage + 1, p->buf[stage + 1].get());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(misc, p->d_misc.get(), 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return KICP_OK;
}
int pre_frame_chain(kicp_pre *p, size_t n_in, bool do_deskew, const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range,
                    double min_range, double voxel_a, double voxel_b, void *out_frame_xyz, size_t cap_points, size_t counts[3], bool f32) {
    counts[0] = counts[1] = counts[2] = 0;
    p->buf_n[0] = p->buf_n[1] = p->buf_n[2] = 0;
    p->egress.src_on_host = false;
    if (n_in == 0) return KICP_OK;
    if (!(voxel_a > 0.0) || !(voxel_b > 0.0)) return fail(KICP_ERR_ARG, "bad voxel size");
    // Buffers 1 and 3 take turns: what the PREVIOUS frame left in buffer 1 - the points a map update that was begun with
    // kicp_map_update_pose_device_begin may still be reading - stays untouched, as buffer 3, until the frame after this one.
    std::swap(p->buf[1], p->buf[3]), std::swap(p->buf_n[1], p->buf_n[3]);
    p->buf_n[1] = 0;
    for (int b = 0; b < 3; ++b)
        if (int rc = pre_ensure_buf(p, b, n_in)) return rc;
    const size_t slots_up = reference_bucket_count(n_in);
    if (int rc = table_fits(p, n_in, slots_up)) return rc;
    const ChainCall c{n_in, tiles_of(n_in), tiles_of(slots_up), preprocess_params(p, n_in, do_deskew, relative_motion_qt, lidar_to_base_qt, max_range, min_range),
                      voxel_a, voxel_b, out_frame_xyz, cap_points, f32};
    // the next message, if one was announced, goes up NOW, from a thread of its own: its 2 MB copy into the staging buffer and its
    // launches run beside this thread's queueing of the frame's kernels, the GPU decodes it on a stream of its own
    bool ahead_out = false;
    if (int rc = ahead_post(p, &ahead_out)) return rc;
    // the tables' arrays are laid out for the LARGEST table this handle can hold
    if (!p->table_clean)
        if (int rc = wipe_tables(p, true)) return rc;
    p->table_clean = false;
    const auto t_start = std::chrono::steady_clock::now();
    const bool fused = p->chain.fused && c.grid <= kFusedScanBlocks;
    bool unfused_tail = true;  // the downsamples still have to run as launches of their own, from buffer 0 on
    uint32_t misc[8] = {};
    if (fused) {
        if (int rc = chain_fused(p, c, misc, &unfused_tail)) return rc;
    } else {
        launch_preprocess(p, c.pp, p->d_misc.get() + kMiscCounts, p->buf[0].get());
        if (int rc = mark_frame_ready(p, c)) return rc;
        if (int rc = egress_start_frame(p, n_in, out_frame_xyz, cap_points, f32)) return rc;
    }
    if (unfused_tail)
        if (int rc = chain_unfused_tail(p, c, misc)) return rc;
    if (g_trace) {
        std::fprintf(stderr, "[kicp]   chained pre-steps: %zu -> %u -> %u -> %u points; %s, results at the host %.3f ms after the first launch; look-ahead upload: %s\n", n_in, misc[4], misc[5], misc[6],
                     !fused ? "unfused" : (unfused_tail ? "fused, table size guessed wrong: unfused downsamples" : "five launches"),
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(),
                     ahead_out ? "on its own thread, collected by the message's kicp_pre_ingest" : "none");
    }
    const int rc = pre_report(p, misc[kMiscError], misc[kMiscProbe], true, 0, 3, misc + kMiscCounts, counts);
    // (what _finish reports; the copy worker moves the upper bound it was given and never reads this)
    if (out_frame_xyz && (rc == KICP_OK || rc == KICP_WARN_TABLE_ORDER)) p->egress.n = counts[0];
    return rc;
}
int frame_ingested_impl(kicp_pre *p, const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range, double min_range, int deskew,
                        double voxel_a, double voxel_b, void *out_frame_xyz, size_t cap_points, size_t out_counts[3], bool f32) {
    if (!p || !relative_motion_qt || !lidar_to_base_qt || !out_counts) return fail(KICP_ERR_ARG, "bad argument");
    if (!p->ingest.valid) return fail(KICP_ERR_ARG, "no ingested cloud: call kicp_pre_ingest first");
    if (out_frame_xyz && cap_points < p->ingest.n) return fail(KICP_ERR_ARG, "the frame's landing area must hold every ingested point");
    if (int rc = set_device(p->device)) return rc;
    return pre_frame_chain(p, p->ingest.n, deskew && p->ingest.stamps, relative_motion_qt, lidar_to_base_qt, max_range, min_range, voxel_a, voxel_b,
                           out_frame_xyz, cap_points, out_counts, f32);
}
int frame_impl(kicp_pre *p, const double *frame_xyz, size_t n, const double *timestamps, size_t n_timestamps, const double relative_motion_qt[7],
               const double lidar_to_base_qt[7], double max_range, double min_range, int deskew, double voxel_a, double voxel_b, void *out_frame_xyz,
               size_t cap_points, size_t out_counts[3], bool f32) {
    if (!p || (!frame_xyz && n) || !relative_motion_qt || !lidar_to_base_qt || !out_counts) return fail(KICP_ERR_ARG, "bad argument");
    const bool do_deskew = deskew && n_timestamps != 0;
    if (do_deskew && (!timestamps || n_timestamps < n)) return fail(KICP_ERR_ARG, "one timestamp per point is required for deskewing");
    if (out_frame_xyz && cap_points < n) return fail(KICP_ERR_ARG, "the frame's landing area must hold every input point");
    if (n > 0x7FFFFFF0ull / 3) return fail(KICP_ERR_CAPACITY, "frame too large");
    if (int rc = set_device(p->device)) return rc;
    if (n)
        if (int rc = upload_frame(p, frame_xyz, n, timestamps, do_deskew)) return rc;
    return pre_frame_chain(p, n, do_deskew, relative_motion_qt, lidar_to_base_qt, max_range, min_range, voxel_a, voxel_b, out_frame_xyz, cap_points, out_counts, f32);
}
}  // namespace
extern "C" {
int kicp_pre_frame_ingested(kicp_pre *p, const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range, double min_range, int deskew,
                            double voxel_a, double voxel_b, double *out_frame_xyz, size_t cap_points, size_t out_counts[3]) {
    KICP_TRACE_CALL();
    return frame_ingested_impl(p, relative_motion_qt, lidar_to_base_qt, max_range, min_range, deskew, voxel_a, voxel_b, out_frame_xyz, cap_points, out_counts, false);
}
int kicp_pre_frame_ingested_f32(kicp_pre *p, const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range, double min_range, int deskew,
                                double voxel_a, double voxel_b, float *out_frame_xyz, size_t cap_points, size_t out_counts[3]) {
    KICP_TRACE_CALL();
    return frame_ingested_impl(p, relative_motion_qt, lidar_to_base_qt, max_range, min_range, deskew, voxel_a, voxel_b, out_frame_xyz, cap_points, out_counts, true);
}
int kicp_pre_frame(kicp_pre *p, const double *frame_xyz, size_t n, const double *timestamps, size_t n_timestamps, const double relative_motion_qt[7],
                   const double lidar_to_base_qt[7], double max_range, double min_range, int deskew, double voxel_a, double voxel_b, double *out_frame_xyz,
                   size_t cap_points, size_t out_counts[3]) {
    KICP_TRACE_CALL();
    return frame_impl(p, frame_xyz, n, timestamps, n_timestamps, relative_motion_qt, lidar_to_base_qt, max_range, min_range, deskew, voxel_a, voxel_b, out_frame_xyz,
                      cap_points, out_counts, false);
}
int kicp_pre_frame_f32(kicp_pre *p, const double *frame_xyz, size_t n, const double *timestamps, size_t n_timestamps, const double relative_motion_qt[7],
                       const double lidar_to_base_qt[7], double max_range, double min_range, int deskew, double voxel_a, double voxel_b, float *out_frame_xyz,
                       size_t cap_points, size_t out_counts[3]) {
    KICP_TRACE_CALL();
    return frame_impl(p, frame_xyz, n, timestamps, n_timestamps, relative_motion_qt, lidar_to_base_qt, max_range, min_range, deskew, voxel_a, voxel_b, out_frame_xyz,
                      cap_points, out_counts, true);
}
int kicp_pre_set_option(kicp_pre *p, const char *name, double value) {
    if (!p || !name) return fail(KICP_ERR_ARG, "bad argument");
    const std::string n(name);
    if (n == "fused") p->chain.fused = value != 0.0;
    else if (n == "guess") p->chain.spec_n0 = value > 0.0 ? static_cast<uint32_t>(value) : 0u, p->chain.spec_n_in = 0u;  // (taken as it is for the next frame)
    else return fail(KICP_ERR_ARG, "unknown pre-step option: " + n);
    return KICP_OK;
}
double kicp_pre_get_option(const kicp_pre *p, const char *name) {
    if (!p || !name) return -1.0;
    const std::string n(name);
    if (n == "fused") return p->chain.fused ? 1.0 : 0.0;
    if (n == "guess") return static_cast<double>(p->chain.spec_n0);
    if (n == "fused_frames") return static_cast<double>(p->chain.fused_frames);
    if (n == "guess_misses") return static_cast<double>(p->chain.spec_misses);
    if (n == "point_tiles") return static_cast<double>(p->chain.last_point_tiles);
    if (n == "l1_tiles") return static_cast<double>(p->chain.last_l1_tiles);
    if (n == "l2_workgroups") return static_cast<double>(p->chain.last_l2_workgroups);
    if (n == "l2_tiles") return static_cast<double>(p->chain.last_l2_tiles);
    if (n == "scan_launches") return static_cast<double>(p->scan_launches);
    if (n == "push_launches") return static_cast<double>(p->egress.push_launches);
    if (n == "push_pieces") return static_cast<double>(p->egress.push_pieces);
    for (int slot = 0; slot < 2; ++slot) {  // "ingest_<counter>" / "ahead_<counter>": the last ingest_run of the slot
        const std::string prefix = slot ? "ahead_" : "ingest_";
        if (n.compare(0, prefix.size(), prefix) != 0) continue;
        const std::string c = n.substr(prefix.size());
        const kicp_pre::IngestCounts &ic = p->ingest.counts[slot];
        if (c == "launches") return static_cast<double>(ic.launches);
        if (c == "workgroups") return static_cast<double>(ic.workgroups);
        if (c == "aligned") return static_cast<double>(ic.aligned);
        if (c == "wide") return static_cast<double>(ic.wide);
        if (c == "piece_records") return static_cast<double>(ic.piece_records);
        if (c == "direct") return static_cast<double>(ic.direct);
    }
    return -1.0;
}
unsigned int kicp_pre_last_max_probe(const kicp_pre *p) { return p ? p->last_max_probe : 0u; }
int kicp_pre_set_probe_limit(kicp_pre *p, unsigned int limit) {
    if (!p || limit == 0u) return fail(KICP_ERR_ARG, "bad argument");
    p->probe_limit = limit;
    return KICP_OK;
}
int kicp_pre_upload(kicp_pre *p, int buffer, const double *xyz, size_t n) {
    KICP_TRACE_CALL();
    if (!p || buffer < 0 || buffer >= KICP_PRE_BUFFERS || (!xyz && n)) return fail(KICP_ERR_ARG, "bad argument");
    if (int rc = set_device(p->device)) return rc;
    if (int rc = pre_ensure_buf(p, buffer, n ? n : 1)) return rc;
    if (n)
        if (int rc = staged_upload(p->stage, 0, p->buf[buffer].get(), xyz, n * 24, p->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->buf_n[buffer] = n;
    return KICP_OK;
}
const double *kicp_pre_device_ptr(const kicp_pre *p, int buffer, size_t *out_n) {
    if (!p || buffer < 0 || buffer >= KICP_PRE_BUFFERS) return nullptr;
    if (out_n) *out_n = p->buf_n[buffer];
    return p->buf[buffer].get();
}
}  // extern "C"
