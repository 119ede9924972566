// kicp_pre_ingest.hip -- a sensor message's way into the pre-steps' ingest slot behind include/kicp.h: PointCloud2 records
// (kicp_pre_ingest), LaserScan ranges (kicp_pre_ingest_scan), the look-ahead that decodes the NEXT message beside the current frame
// (kicp_pre_ingest_ahead, ahead_post / ahead_join), and the slot's readout (kernels: kicp_pre_ingest.hpp).
#include "kicp_pre_internal.hpp"
#include "kicp_pre_ingest.hpp"

namespace {
int ingest_validate(const kicp_pre *p, const void *data, size_t n_points, const kicp_cloud_layout *layout) {
    if (!p || !layout || (!data && n_points)) return fail(KICP_ERR_ARG, "bad argument");
    const kicp_cloud_layout &L = *layout;
    const int st = L.stamp_datatype;
    if (st != 0 && st != KICP_FIELD_UINT32 && st != KICP_FIELD_FLOAT32 && st != KICP_FIELD_FLOAT64)
        return fail(KICP_ERR_ARG, "timestamp field type not supported");  // TimeStampHandler.cpp:103
    const uint32_t stamp_bytes = st == KICP_FIELD_FLOAT64 ? 8u : 4u;
    if (L.point_step == 0 || L.offset_x + 4ull > L.point_step || L.offset_y + 4ull > L.point_step || L.offset_z + 4ull > L.point_step ||
        (st != 0 && L.offset_stamp + static_cast<unsigned long long>(stamp_bytes) > L.point_step))
        return fail(KICP_ERR_ARG, "field offsets do not fit inside point_step");
    if (n_points > 0x7FFFFFF0ull / 3) return fail(KICP_ERR_CAPACITY, "cloud too large");
    return KICP_OK;
}
// Upload + decode of one message (n_points > 0, <= p->cap_n) on `stream` into (out_xyz, out_ts: stamps in SECONDS) and wait for it:
// the CPU copies the message into the pinned staging buffer piece by piece and launches k_ingest behind each piece, which decodes
// the records straight out of host memory (16 bytes per lane for the usual x y z t layout) while the CPU copies the next piece;
// the cloud's last workgroup folds the stamps' extrema and says so in the host record `slot` (0: this call's, 1: the look-ahead's).
// Round 5 pulled the bytes into HBM (k_pull_bytes per piece), decoded them with one more launch, normalised the stamps with another
// and copied the extrema back: four stream operations and 6 MB of traffic more per frame.
constexpr size_t kIngestPiece = 512u << 10;
// d_raw: the message bytes in HBM, where the device cannot read the staging buffer
int raw_reserve(kicp_pre *p, size_t bytes) {
    if (bytes <= p->ingest.d_raw.capacity()) return KICP_OK;
    HIP_TRY(hipDeviceSynchronize());  // (rare: the buffer grows; nothing may still be reading the old one)
    return p->ingest.d_raw.reserve(bytes + bytes / 4 + 4096);
}
int ingest_run(kicp_pre *p, const void *data, size_t n_points, const kicp_cloud_layout &L, const Pose *sensor_pose, hipStream_t stream, double *out_xyz,
               double *out_ts, HostStage &stage, int slot, double *out_lo, double *out_hi) {
    const int st = L.stamp_datatype;
    const uint32_t stamp_bytes = st == KICP_FIELD_FLOAT64 ? 8u : 4u;
    const size_t bytes = n_points * static_cast<size_t>(L.point_step);
    if (int rc = stage_begin(stage, bytes, stream)) return rc;
    if (slot == 0) trace_lap("staging buffer free");
    const bool direct = stage.buf.dev() != nullptr;  // the device reads the staging buffer itself
    if (!direct)
        if (int rc = raw_reserve(p, bytes)) return rc;
    IngestParams ip{};
    ip.point_step = L.point_step;
    ip.off_x = L.offset_x, ip.off_y = L.offset_y, ip.off_z = L.offset_z, ip.off_t = L.offset_stamp, ip.stamp_type = st;
    ip.transform = sensor_pose ? 1 : 0;
    // (the staging buffer and d_raw are 256-byte aligned; a piece starts at a multiple of 256 records)
    ip.aligned = (L.point_step % 4 == 0 && L.offset_x % 4 == 0 && L.offset_y % 4 == 0 && L.offset_z % 4 == 0 &&
                  (st == 0 || (L.offset_stamp % stamp_bytes == 0 && L.point_step % stamp_bytes == 0))) ? 1 : 0;
    if (sensor_pose) ip.T = *sensor_pose;
    ip.out_xyz = out_xyz, ip.out_stamps = out_ts, ip.block_minmax = p->d_block_minmax.get();
    ip.total_blocks = static_cast<uint32_t>((n_points + 255) / 256);
    ip.ticket = p->ingest.d_ticket.get() + slot;
    // a look-ahead message: few workgroups going round its tiles, so that at most ~200 KB of it are on request at any time (k_ingest;
    // 24 / 48 / 64 workgroups and 0.5 / 1 / 4 MB pieces measured within the boxes' noise of each other, 8 and 512 clearly worse)
    static const uint32_t ahead_wgs = static_cast<uint32_t>(std::max(1l, env_int("KICP_PRE_AHEAD_WGS", 48)));
    static const size_t ahead_piece = static_cast<size_t>(std::max(64l, env_int("KICP_PRE_AHEAD_PIECE_KB", 512))) << 10;
    const uint32_t wgs_cap = slot == 1 ? ahead_wgs : 0xFFFFFFFFu;
    unsigned long long *rec = p->h_rec.get() + kRecIngest + kRecIngestStride * slot;
    ip.host_rec = rec, ip.seq = ++p->ingest.seq;
    // pieces, so that the GPU decodes piece k while the CPU copies piece k + 1 (a look-ahead message too: as ONE launch behind the
    // whole 2 MB copy it was not there when the next frame asked for it)
    const size_t piece_records = std::max<size_t>(256, (slot == 1 ? ahead_piece : kIngestPiece) / L.point_step / 256 * 256);
    // What the call waits for is the link: a kernel's loads pull ~30 GB/s out of host memory (2 MB: ~65 us from the first launch to the
    // record), whoever copies and however the launches are arranged.  Measured and not kept: a helper thread sharing the copy into the
    // staging buffer (all four launches queued by 47 us instead of 66 - the record arrives at 87 us either way), the copy engine moving
    // the pieces into HBM first (106 us).
    // this call's message: consecutive pieces' decodes go to two streams in turn - on one stream each launch waits for the one before
    // it to drain; side by side they keep the link busy (2 % of the frame)
    static const bool two_streams = env_int("KICP_PRE_INGEST_STREAMS", 2) != 1;
    hipStream_t lanes[2] = {stream, stream};
    if (slot == 0 && two_streams) {
        if (!p->ingest.stream2) HIP_TRY(hipStreamCreateWithFlags(&p->ingest.stream2, hipStreamNonBlocking));
        lanes[1] = p->ingest.stream2;
    }
    unsigned piece_index = 0;
    uint32_t widest = 0;
    for (size_t first = 0; first < n_points; first += piece_records)  // (one ticket per workgroup of every launch)
        p->ingest.ticket_drawn[slot] += std::min<uint32_t>(wgs_cap, static_cast<uint32_t>((std::min(piece_records, n_points - first) + 255) / 256));
    ip.ticket_done = p->ingest.ticket_drawn[slot];
    for (size_t first = 0; first < n_points; first += piece_records) {
        const size_t count = std::min(piece_records, n_points - first), off = first * L.point_step, len = count * L.point_step;
        std::memcpy(stage.buf.get() + off, static_cast<const unsigned char *>(data) + off, len);
        if (direct) {
            ip.raw = stage.buf.dev() + off;
        } else {
            HIP_TRY(hipMemcpyAsync(p->ingest.d_raw.get() + off, stage.buf.get() + off, len, hipMemcpyHostToDevice, lanes[piece_index & 1u]));
            ip.raw = p->ingest.d_raw.get() + off;
        }
        ip.first = static_cast<uint32_t>(first), ip.n = static_cast<uint32_t>(count);
        const uint32_t wgs = std::min<uint32_t>(wgs_cap, static_cast<uint32_t>((count + 255) / 256));
        hipLaunchKernelGGL(k_ingest, dim3(wgs), dim3(256), 0, lanes[piece_index & 1u], ip);
        widest = std::max(widest, wgs);
        ++piece_index;
        if (slot == 0) trace_lap("piece copied, its decode launched");
    }
    HIP_TRY(hipGetLastError());
    kicp_pre::IngestCounts &ic = p->ingest.counts[slot];
    ic.launches = piece_index, ic.workgroups = widest, ic.aligned = ip.aligned, ic.wide = L.point_step > 128u ? 1 : 0, ic.direct = direct ? 1 : 0;
    ic.piece_records = piece_records;
    // (`data` and the staging buffer are free again behind this.)  The record is written by the workgroup that finishes last, on either
    // lane: once the limit has run out wait_word drains `stream` alone, so the other lane is drained too before the call gives up
    if (wait_word(rec + 2, ip.seq, ~0ull, stream, 2.0, kPreLost) != KICP_OK)
        if (int rc = wait_word(rec + 2, ip.seq, ~0ull, lanes[1], 0.0, kPreLost)) return rc;
    if (slot == 0) trace_lap("the decoded cloud's record at the host");
    *out_lo = *out_hi = 0.0;
    if (st != 0) *out_lo = ordered_value(rec[0]), *out_hi = ordered_value(rec[1]);
    return KICP_OK;
}
bool same_layout(const kicp_cloud_layout &a, const kicp_cloud_layout &b) {
    return a.point_step == b.point_step && a.offset_x == b.offset_x && a.offset_y == b.offset_y && a.offset_z == b.offset_z && a.stamp_datatype == b.stamp_datatype &&
           (a.stamp_datatype == 0 || a.offset_stamp == b.offset_stamp);
}
// the announced next message goes into the second slot now (the look-ahead thread's job)
int ahead_run(kicp_pre *p) {
    kicp_pre::Ahead &a = p->ahead;
    if (a.state != 1 || a.n == 0 || a.n > p->cap_n) return KICP_OK;  // (a cloud that does not fit the buffers is left to its kicp_pre_ingest call)
    if (!a.stream) {
        // lowest priority: background work - and the runtime keeps a pool of hardware queues per priority, so that this stream does
        // not share a queue with the frame's way back (same pool: the look-ahead's kernel waited for the push kernel's 60 us)
        int least = 0, greatest = 0;
        static const bool low = env_flag("KICP_PRE_AHEAD_PRIORITY", true);
        if (!(low && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest &&
              hipStreamCreateWithPriority(&a.stream, hipStreamNonBlocking, least) == hipSuccess)) {
            (void)hipGetLastError();  // (no priorities on this platform: an ordinary stream)
            a.stream = nullptr;
            HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
        }
    }
    if (int rc = ingest_run(p, a.data, a.n, a.layout, a.has_pose ? &a.pose : nullptr, a.stream, a.d_in2.get(), a.d_ts2.get(), a.stage, 1, &a.lo, &a.hi)) return rc;
    const size_t bytes = a.n * static_cast<size_t>(a.layout.point_step);
    a.edge_bytes = std::min<size_t>(64, bytes);
    std::memcpy(a.edge, a.data, a.edge_bytes);
    std::memcpy(a.edge + 64, static_cast<const unsigned char *>(a.data) + bytes - a.edge_bytes, a.edge_bytes);
    a.state = 2;
    return KICP_OK;
}
// what an ingest entry leaves behind: n points in d_in, with or without stamps (in seconds, between lo and hi, where `raw`)
void ingest_set(kicp_pre *p, size_t n, bool stamps, bool raw, double lo, double hi) {
    p->ingest.valid = true, p->ingest.n = n, p->ingest.stamps = stamps;
    p->ingest.ts_raw = raw, p->ingest.ts_lo = lo, p->ingest.ts_hi = hi;
}
// The projector's cosine table for this scan: rebuilt on the host (glibc cos / sin) and uploaded only when its key changes
// (laser_geometry's cache, kicp_pre_ingest.hpp laser_rules [RECALLED])
int scan_table(kicp_pre *p, size_t n, const kicp_laser_scan &s) {
    auto &t = p->scan;
    if (!laser_rules::table_stale(t.valid, n, s.angle_min, s.angle_max, t.n, t.angle_min, t.angle_max)) return KICP_OK;
    t.valid = false;  // (until the new one is in place)
    t.cs_host.resize(2 * n);
    for (size_t i = 0; i < n; ++i) laser_rules::table_entry(s.angle_min, s.angle_increment, static_cast<uint32_t>(i), t.cs_host[2 * i], t.cs_host[2 * i + 1]);
    if (n * 16 > t.d_cs.capacity())  // (nothing reads the old one: every scan ingest returns after its kernel)
        if (int rc = t.d_cs.reserve(n * 16 + n * 4 + 4096)) return rc;
    if (n)
        if (int rc = staged_upload(p->stage, 0, t.d_cs.get(), t.cs_host.data(), n * 16, p->stream)) return rc;
    t.valid = true, t.n = n, t.angle_min = s.angle_min, t.angle_max = s.angle_max;
    return KICP_OK;
}
}  // namespace
namespace kicp {
namespace host {
// the look-ahead upload, if one is out, must be over before its result is looked at or anything it uses changes hands
int ahead_join(kicp_pre *p) {
    if (!p->ahead.job_out) return KICP_OK;
    p->ahead.job_out = false;
    return p->ahead.thread.wait();
}
int ahead_post(kicp_pre *p, bool *posted) {
    *posted = false;
    if (int rc = ahead_join(p)) return rc;
    if (p->ahead.state == 1 && p->ahead.n != 0 && p->ahead.n <= p->cap_n) {
        p->ahead.thread.post(p->device, [p] { return ahead_run(p); });
        *posted = p->ahead.job_out = true;  // (collected by the kicp_pre_ingest call of that message - or whoever needs its buffers first: ahead_join)
    }
    return KICP_OK;
}
}  // namespace host
}  // namespace kicp
extern "C" {
int kicp_pre_ingest(kicp_pre *p, const void *data, size_t n_points, const kicp_cloud_layout *layout, const double sensor_pose_qt[7],
                    double *out_min_stamp, double *out_max_stamp) {
    KICP_TRACE_CALL();
    if (int rc = ingest_validate(p, data, n_points, layout)) return rc;
    const kicp_cloud_layout &L = *layout;
    const int st = L.stamp_datatype;
    if (int rc = set_device(p->device)) return rc;
    if (out_min_stamp) *out_min_stamp = 0.0;
    if (out_max_stamp) *out_max_stamp = 0.0;
    if (int rc = ahead_join(p)) return rc;  // (the announced message's upload has had the registration and the map update to finish behind)
    kicp_pre::Ahead &a = p->ahead;
    const bool pose_matches = sensor_pose_qt ? (a.has_pose && std::memcmp(&a.pose, sensor_pose_qt, 7 * sizeof(double)) == 0) : !a.has_pose;
    bool same_bytes = false;
    if (a.state == 2 && a.data == data && a.n == n_points && same_layout(a.layout, L) && pose_matches) {
        const size_t bytes = n_points * static_cast<size_t>(L.point_step);
        same_bytes = std::memcmp(a.edge, data, a.edge_bytes) == 0 &&
                     std::memcmp(a.edge + 64, static_cast<const unsigned char *>(data) + bytes - a.edge_bytes, a.edge_bytes) == 0;
    }
    const bool stamps = st != 0 && n_points != 0;
    if (same_bytes) {
        // the message was uploaded and decoded ahead (kicp_pre_ingest_ahead + the previous frame's chained pre-steps): take the slot
        std::swap(p->d_in, a.d_in2), std::swap(p->d_ts, a.d_ts2);
        a.state = 0, ++a.hits;
        ingest_set(p, n_points, stamps, stamps, a.lo, a.hi);
        if (out_min_stamp) *out_min_stamp = a.lo;
        if (out_max_stamp) *out_max_stamp = a.hi;
        return KICP_OK;
    }
    a.state = 0;  // (another message than the one announced: the announcement is void)
    ingest_set(p, n_points, stamps, false, 0.0, 0.0);
    if (n_points == 0) return KICP_OK;
    if (int rc = pre_ensure(p, n_points)) return rc;
    Pose T{};
    if (sensor_pose_qt) T = pose_from(sensor_pose_qt);
    double lo = 0.0, hi = 0.0;
    if (int rc = ingest_run(p, data, n_points, L, sensor_pose_qt ? &T : nullptr, p->stream, p->d_in.get(), p->d_ts.get(), p->stage, 0, &lo, &hi)) {
        p->ingest.valid = false;
        return rc;
    }
    p->ingest.ts_raw = st != 0, p->ingest.ts_lo = lo, p->ingest.ts_hi = hi;
    if (out_min_stamp) *out_min_stamp = lo;
    if (out_max_stamp) *out_max_stamp = hi;
    return KICP_OK;
}
int kicp_pre_ingest_scan(kicp_pre *p, const float *ranges, size_t n_ranges, const kicp_laser_scan *scan, double range_cutoff, double *out_min_stamp,
                         double *out_max_stamp) {
    KICP_TRACE_CALL();
    if (!p || !scan || (!ranges && n_ranges)) return fail(KICP_ERR_ARG, "bad argument");
    if (n_ranges > 0x7FFFFFF0ull / 3) return fail(KICP_ERR_CAPACITY, "scan too large");
    if (int rc = set_device(p->device)) return rc;
    if (out_min_stamp) *out_min_stamp = 0.0;
    if (out_max_stamp) *out_max_stamp = 0.0;
    if (int rc = ahead_join(p)) return rc;
    p->ahead.state = 0;  // (another message than the one announced: the announcement is void)
    p->ingest.valid = false, p->ingest.ts_raw = false, p->ingest.ts_lo = p->ingest.ts_hi = 0.0;
    const kicp_laser_scan &s = *scan;
    if (int rc = scan_table(p, n_ranges, s)) return rc;
    if (n_ranges == 0) {
        p->ingest.valid = true, p->ingest.n = 0, p->ingest.stamps = false;
        return KICP_OK;
    }
    if (int rc = pre_ensure(p, n_ranges)) return rc;
    // the ranges go up as a cloud's bytes do (ingest_run): into the pinned staging buffer, read from there by the kernel
    const size_t bytes = n_ranges * 4;
    if (int rc = stage_begin(p->stage, bytes, p->stream)) return rc;  // (waits for the table's upload, if there was one)
    std::memcpy(p->stage.buf.get(), ranges, bytes);
    ScanParams sp{};
    if (p->stage.buf.dev()) {
        sp.ranges = reinterpret_cast<const float *>(p->stage.buf.dev());
    } else {
        if (int rc = raw_reserve(p, bytes)) return rc;
        HIP_TRY(hipMemcpyAsync(p->ingest.d_raw.get(), p->stage.buf.get(), bytes, hipMemcpyHostToDevice, p->stream));
        sp.ranges = reinterpret_cast<const float *>(p->ingest.d_raw.get());
    }
    const uint32_t tiles = static_cast<uint32_t>((n_ranges + kScanTile - 1) / kScanTile);
    sp.tiles_per_wg = (tiles + kScanMaxWgs - 1) / kScanMaxWgs;
    const uint32_t grid = (tiles + sp.tiles_per_wg - 1) / sp.tiles_per_wg;  // (no workgroup without a tile)
    sp.cs = reinterpret_cast<const double *>(p->scan.d_cs.get()), sp.n = static_cast<uint32_t>(n_ranges);
    sp.range_min = s.range_min, sp.time_increment = s.time_increment, sp.cutoff = laser_rules::cutoff(range_cutoff, s.range_max);
    sp.out_xyz = p->d_in.get(), sp.out_stamps = p->d_ts.get(), sp.wg_counts = p->d_block_counts.get(), sp.block_minmax = p->d_block_minmax.get();
    p->ingest.ticket_drawn[0] += grid;
    sp.ticket = p->ingest.d_ticket.get(), sp.ticket_done = p->ingest.ticket_drawn[0];
    unsigned long long *rec = p->h_rec.get() + kRecIngest;
    sp.host_rec = rec, sp.seq = ++p->ingest.seq;
    hipLaunchKernelGGL(k_ingest_scan, dim3(grid), dim3(256), 0, p->stream, sp);
    HIP_TRY(hipGetLastError());
    if (int rc = wait_word(rec + 2, sp.seq, ~0ull, p->stream, 2.0, kPreLost)) return rc;  // (the staging buffer is free again behind this)
    const size_t kept = static_cast<size_t>(rec[3]);
    p->ingest.valid = true, p->ingest.n = kept, p->ingest.stamps = kept != 0;
    p->ingest.ts_raw = kept != 0;
    if (kept) p->ingest.ts_lo = ordered_value(rec[0]), p->ingest.ts_hi = ordered_value(rec[1]);
    if (out_min_stamp) *out_min_stamp = p->ingest.ts_lo;
    if (out_max_stamp) *out_max_stamp = p->ingest.ts_hi;
    return KICP_OK;
}
int kicp_pre_ingest_ahead(kicp_pre *p, const void *data, size_t n_points, const kicp_cloud_layout *layout, const double sensor_pose_qt[7]) {
    if (int rc = ingest_validate(p, data, n_points, layout)) return rc;
    if (int rc = ahead_join(p)) return rc;
    kicp_pre::Ahead &a = p->ahead;
    a.data = data, a.n = n_points, a.layout = *layout, a.has_pose = sensor_pose_qt != nullptr, a.state = n_points ? 1 : 0;
    if (sensor_pose_qt) a.pose = pose_from(sensor_pose_qt);
    return KICP_OK;
}
int kicp_pre_ingested(const kicp_pre *p, double *out_xyz, double *out_stamps, size_t cap_points, size_t *out_n, int *out_has_stamps) {
    if (!p) return fail(KICP_ERR_ARG, "bad argument");
    if (!p->ingest.valid) return fail(KICP_ERR_ARG, "no ingested cloud: call kicp_pre_ingest first");
    if (int rc = set_device(p->device)) return rc;
    const size_t k = std::min(p->ingest.n, cap_points);
    if (k && out_xyz)
        if (int rc = staged_download(p->stage, out_xyz, p->d_in.get(), k * 24, p->stream)) return rc;
    if (k && out_stamps && p->ingest.stamps) {
        if (int rc = staged_download(p->stage, out_stamps, p->d_ts.get(), k * 8, p->stream)) return rc;
        // TimeStampHandler.cpp:121-128 - the two fp64 operations the device applies where it consumes a stamp (kicp_pre.hpp: ts_normalise)
        if (p->ingest.ts_raw)
            for (size_t i = 0; i < k; ++i) out_stamps[i] = (out_stamps[i] - p->ingest.ts_lo) / (p->ingest.ts_hi - p->ingest.ts_lo);
    }
    if (out_n) *out_n = p->ingest.n;
    if (out_has_stamps) *out_has_stamps = p->ingest.stamps ? 1 : 0;
    return KICP_OK;
}
size_t kicp_pre_ingested_count(const kicp_pre *p) { return (p && p->ingest.valid) ? p->ingest.n : 0; }
unsigned long long kicp_pre_ahead_hits(const kicp_pre *p) { return p ? p->ahead.hits : 0ull; }
}  // extern "C"
