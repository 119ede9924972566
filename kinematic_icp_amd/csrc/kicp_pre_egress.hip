// kicp_pre_egress.hip -- the pre-steps' results on their way back to the caller behind include/kicp.h: kicp_pre_download*, the
// background download with its copy worker, and the push of the frame a chained call returns (kernels: kicp_pre_egress.hpp).
#include "kicp_pre_internal.hpp"
#include "kicp_pre_egress.hpp"

namespace {
// What the copy worker is handed at post, by value: it reads nothing of the handle that the caller writes while the job is out.
struct EgressJob {
    enum Mode {
        kOneEvent,  // the transfer is one piece: wait for egress.done, one copy
        kPieces,    // kCopyPieces transfers, an event behind each: copy piece i while piece i + 1 is on its way
        kPushed     // k_push_frame*'s pieces, announced in h_rec[kRecPush ..]: no HIP call to follow them
    } mode = kOneEvent;
    void *dst = nullptr;      // caller memory (nullptr: the bytes stay in the landing area, _finish hands them over)
    size_t dst_points = 0;    // ... and the points it holds
    size_t rec_bytes = 24;    // bytes per point
    size_t points = 0;        // points to move (an upper bound for a chained frame, whose count the host does not know yet)
    size_t piece_bytes = 0;   // kPieces, kPushed: bytes per piece
    uint32_t push_seq = 0;    // kPushed: the launch's sequence number, the upper half of its flags
    bool queues_transfer = false;  // the job begins with transfer_queue(buffer 0, points, behind chain.ready)
};
// a transfer of `bytes` goes in kCopyPieces pieces of this many bytes (0: in one - below 1 MiB the pieces' API calls cost more than
// the worker's copy behind the transfer)
size_t transfer_piece_bytes(size_t bytes) {
    return bytes >= (1u << 20) ? ((bytes + kicp_pre::kCopyPieces - 1) / kicp_pre::kCopyPieces + 4095) / 4096 * 4096 : 0;
}
int landing_reserve(kicp_pre *p, size_t bytes) {
    if (bytes <= p->egress.host.capacity()) return KICP_OK;
    return p->egress.host.reserve(bytes + bytes / 2 + (1u << 20), hipHostMallocDefault, false);
}
// the transfer itself, n points of 24 bytes of `buffer` into the landing area (calling thread, or the worker for the chained pre-steps)
int transfer_queue(kicp_pre *p, int buffer, size_t n, hipEvent_t after) {
    auto &g = p->egress;
    const size_t bytes = n * 24;
    if (int rc = landing_reserve(p, bytes)) return rc;
    // the buffer's contents are final (every call that fills a buffer returns only after its kernels have finished) - or will be
    // once `after` has happened on the pre-step stream
    if (after) HIP_TRY(hipStreamWaitEvent(g.stream, after, 0));
    if (const size_t piece = transfer_piece_bytes(bytes)) {  // frame-sized: in pieces, so that the worker's copy runs behind the transfer instead of after it
        for (int i = 0; i < kicp_pre::kCopyPieces; ++i) {
            if (!g.piece_done[i]) HIP_TRY(hipEventCreateWithFlags(&g.piece_done[i], hipEventDisableTiming));
            const size_t off = std::min(bytes, piece * i), len = std::min(piece, bytes - off);
            if (len) HIP_TRY(hipMemcpyAsync(g.host.get() + off, reinterpret_cast<const unsigned char *>(p->buf[buffer].get()) + off, len, hipMemcpyDeviceToHost, g.stream));
            HIP_TRY(hipEventRecord(g.piece_done[i], g.stream));
        }
    } else if (bytes) {
        HIP_TRY(hipMemcpyAsync(g.host.get(), p->buf[buffer].get(), bytes, hipMemcpyDeviceToHost, g.stream));
    }
    HIP_TRY(hipEventRecord(g.done, g.stream));
    return KICP_OK;
}
// wait for an event of the download WITHOUT going to sleep on it: a blocking wait wakes the thread by interrupt, tens of microseconds
// after the transfer has landed - more than the copy it is waiting to start takes; the wait is bounded (a frame's transfer takes
// ~100 us), after 5 ms the thread does block
int spin_on_event(hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return KICP_OK;
        if (q != hipErrorNotReady) HIP_TRY(q);
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > 5.0) {
            HIP_TRY(hipEventSynchronize(ev));
            return KICP_OK;
        }
    }
}
// k_push_frame's pieces: a flag per piece in host memory, (seq << 32) | bytes - a short piece is the last one
int follow_pushed_pieces(kicp_pre *p, const EgressJob &job, size_t want) {
    const volatile unsigned long long *flags = p->h_rec.get() + kRecPush;
    const unsigned long long tag = static_cast<unsigned long long>(job.push_seq) << 32;
    const auto t0 = std::chrono::steady_clock::now();
    double landed_us[kPushPieces] = {}, copied_us[kPushPieces] = {};
    int pieces_seen = 0, rc = KICP_OK;
    for (int i = 0; i < kPushPieces; ++i) {
        unsigned long long f = 0;  // (2 s for the whole frame: something is badly wrong then - surface it instead of spinning for ever)
        const double left_ms = 2000.0 - std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        rc = wait_word(flags + i, tag, 0xFFFFFFFF00000000ull, p->egress.stream, left_ms, "a piece of the frame was never announced", &f);
        if (rc) break;
        ++p->egress.push_pieces;
        const size_t len = static_cast<size_t>(f & 0xFFFFFFFFull), off = job.piece_bytes * i;
        if (g_trace) landed_us[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (len && job.dst && off < want) std::memcpy(static_cast<unsigned char *>(job.dst) + off, p->egress.host.get() + off, std::min(len, want - off));
        if (g_trace) copied_us[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), pieces_seen = i + 1;
        if (len < job.piece_bytes) break;
    }
    if (g_trace) {  // (since this thread took the job: when each piece's flag was seen, when its copy into the caller's memory was over)
        std::string line = "[kicp]     the frame's way back, us (landed/copied):";
        char buf[48];
        for (int i = 0; i < pieces_seen; ++i) std::snprintf(buf, sizeof buf, " %.0f/%.0f", landed_us[i], copied_us[i]), line += buf;
        std::fprintf(stderr, "%s\n", line.c_str());
    }
    return rc;
}
// the copy worker's job: the landed bytes into the caller's memory, piece by piece as they arrive
int egress_job(kicp_pre *p, const EgressJob &job) {
    if (job.queues_transfer)  // (chained pre-steps: the transfer is queued here, behind the event that says buffer 0 is complete)
        if (int rc = transfer_queue(p, 0, job.points, p->chain.ready)) return rc;
    const size_t want = std::min(job.points, job.dst_points) * job.rec_bytes;
    const unsigned char *landed = p->egress.host.get();
    switch (job.mode) {
    case EgressJob::kPushed: return follow_pushed_pieces(p, job, want);
    case EgressJob::kPieces:
        for (int i = 0; i < kicp_pre::kCopyPieces; ++i) {
            if (int rc = spin_on_event(p->egress.piece_done[i])) return rc;
            const size_t off = std::min(want, job.piece_bytes * i), len = std::min(job.piece_bytes, want - off);
            if (len) std::memcpy(static_cast<unsigned char *>(job.dst) + off, landed + off, len);
        }
        return KICP_OK;
    case EgressJob::kOneEvent:
        if (int rc = spin_on_event(p->egress.done)) return rc;
        if (want && job.dst) std::memcpy(job.dst, landed, want);
        return KICP_OK;
    }
    return KICP_OK;
}
// a job of n points of 24 bytes that the DMA engine moves: in pieces where the transfer is and there is somewhere to copy them to
EgressJob transfer_job(void *dst, size_t dst_points, size_t n) {
    EgressJob job;
    job.dst = dst, job.dst_points = dst_points, job.points = n;
    job.piece_bytes = transfer_piece_bytes(n * 24);
    job.mode = job.piece_bytes && dst ? EgressJob::kPieces : EgressJob::kOneEvent;
    return job;
}
void egress_post(kicp_pre *p, const EgressJob &job) {
    p->egress.dst = job.dst, p->egress.rec_bytes = job.rec_bytes;
    p->egress.worker.post(p->device, [p, job] { return egress_job(p, job); });
    p->egress.job_out = true;
}
// the copy worker's job, if one is out, is over behind this; its result
int egress_join(kicp_pre *p) {
    if (!p->egress.job_out) return KICP_OK;
    p->egress.job_out = false;
    return p->egress.worker.wait();
}
// the download's stream and event exist, and an earlier download nobody collected (and the worker's copy) has finished
int egress_settle(kicp_pre *p) {
    auto &g = p->egress;
    if (!g.stream) HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    if (!g.done) HIP_TRY(hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
    if (g.buffer >= 0) {
        (void)egress_join(p);  // (nobody asked for it: its result goes with it)
        HIP_TRY(hipStreamSynchronize(g.stream));
    }
    return KICP_OK;
}
// buffer 2's copy in host memory is complete (the fused chain's last launch writes it; nobody has waited for that launch yet)
int src_host_wait(const kicp_pre *p) {
    return wait_word(p->h_rec.get() + kRecSrcHost, static_cast<unsigned long long>(p->egress.src_seq) << 32, 0xFFFFFFFF00000000ull, p->stream, 2.0, kPreLost);
}
}  // namespace
namespace kicp {
namespace host {
int egress_start_frame(kicp_pre *p, size_t n_in, void *out, size_t cap_points, bool f32) {
    if (!out) return KICP_OK;
    auto &g = p->egress;
    if (int rc = egress_settle(p)) return rc;  // (an earlier download nobody collected)
    EgressJob job;
    job.dst = out, job.dst_points = cap_points, job.points = n_in, job.rec_bytes = f32 ? 12 : 24;
    if (int rc = landing_reserve(p, n_in * job.rec_bytes)) return rc;
    static const int push_wgs = static_cast<int>(env_int("KICP_PRE_PUSH_WGS", 16));
    if (f32 && !g.host.dev()) return fail(KICP_ERR_HIP, "the frame's FLOAT32 records need a host-mapped landing area");
    if (push_wgs <= 0 && !f32) {  // (A/B: the DMA engine moves the frame, in pieces, queued here instead of by the worker)
        if (int rc = transfer_queue(p, 0, n_in, p->chain.ready)) return rc;
        job = transfer_job(out, cap_points, n_in);
    } else if (g.host.dev()) {
        // k_push_frame on the download stream, behind the event: the frame crosses PCIe as a kernel's stores, piece by piece, each
        // piece announced in host memory; the worker needs no HIP call to follow it
        PushParams q{};
        q.src = reinterpret_cast<const unsigned char *>(p->buf[0].get()), q.dst = g.host.dev(), q.n_points = p->d_misc.get() + kMiscCounts;
        q.piece_bytes = static_cast<uint32_t>(((n_in * job.rec_bytes + kPushPieces - 1) / kPushPieces + 4095) / 4096 * 4096);
        const uint32_t push_grid = static_cast<uint32_t>(push_wgs > 0 ? push_wgs : 16);
        g.push_drawn += push_grid;
        q.tickets = g.d_push_tickets.get(), q.ticket_done = g.push_drawn, q.host_flags = p->h_rec.get() + kRecPush, q.seq = ++g.push_seq;
        if (q.seq == 0u) q.seq = ++g.push_seq;
        HIP_TRY(hipStreamWaitEvent(g.stream, p->chain.ready, 0));
        if (f32) hipLaunchKernelGGL(k_push_frame_f32, dim3(push_grid), dim3(256), 0, g.stream, q);
        else hipLaunchKernelGGL(k_push_frame, dim3(push_grid), dim3(256), 0, g.stream, q);
        HIP_TRY(hipGetLastError());
        ++g.push_launches;
        job.mode = EgressJob::kPushed, job.piece_bytes = q.piece_bytes, job.push_seq = q.seq;
    } else {  // no mapped landing area: the worker also queues the DMA transfer, in pieces (its dozen API calls cost the calling thread ~40 us)
        job = transfer_job(out, cap_points, n_in);
        job.queues_transfer = true;
    }
    g.buffer = 0, g.n = n_in;
    egress_post(p, job);  // the worker moves the pieces into the caller's memory as they land
    return KICP_OK;
}
void egress_destroy(kicp_pre *p) {
    auto &g = p->egress;
    (void)egress_join(p);
    g.worker.stop();
    if (g.stream) hipStreamSynchronize(g.stream), hipStreamDestroy(g.stream);
    if (g.done) hipEventDestroy(g.done);
    for (hipEvent_t e : g.piece_done)
        if (e) hipEventDestroy(e);
}
}  // namespace host
}  // namespace kicp
extern "C" {
int kicp_pre_download(const kicp_pre *p, int buffer, double *out_xyz, size_t cap_points, size_t *out_n) {
    KICP_TRACE_CALL();
    if (!p || buffer < 0 || buffer >= KICP_PRE_BUFFERS) return fail(KICP_ERR_ARG, "bad argument");
    if (int rc = set_device(p->device)) return rc;
    const size_t n = p->buf_n[buffer], k = std::min(n, cap_points);
    if (k && out_xyz) {
        if (buffer == 2 && p->egress.src_on_host && !p->egress.src_f32) {  // (the fused chain leaves a copy in host memory)
            if (int rc = src_host_wait(p)) return rc;
            std::memcpy(out_xyz, p->egress.h_src.get(), k * 24);
        } else if (int rc = staged_download(p->stage, out_xyz, p->buf[buffer].get(), k * 24, p->stream)) return rc;
    }
    if (out_n) *out_n = n;
    return KICP_OK;
}
int kicp_pre_download_f32(const kicp_pre *cp, int buffer, float *out_xyz, size_t cap_points, size_t *out_n) {
    KICP_TRACE_CALL();
    kicp_pre *p = const_cast<kicp_pre *>(cp);  // logically const: only the narrowing scratch is touched
    if (!p || buffer < 0 || buffer >= KICP_PRE_BUFFERS) return fail(KICP_ERR_ARG, "bad argument");
    if (int rc = set_device(p->device)) return rc;
    const size_t n = p->buf_n[buffer], k = std::min(n, cap_points);
    if (k && out_xyz) {
        if (buffer == 2 && p->egress.src_on_host && p->egress.src_f32) {  // (the fused chain of a kicp_pre_frame*_f32 call left the records in host memory)
            if (int rc = src_host_wait(p)) return rc;
            std::memcpy(out_xyz, p->egress.h_src.get(), k * 12);
        } else {
            DevBuf<float> &d_narrow = p->egress.d_narrow;
            if (k * 3 > d_narrow.capacity())
                if (int rc = d_narrow.reserve(k * 3 + k / 4 * 3 + 3072)) return rc;
            const size_t words = k * 3;
            hipLaunchKernelGGL(k_narrow_f32, dim3(static_cast<uint32_t>(std::min<size_t>((words + 255) / 256, 1024))), dim3(256), 0, p->stream, p->buf[buffer].get(), words, d_narrow.get());
            HIP_TRY(hipGetLastError());
            if (int rc = staged_download(p->stage, out_xyz, d_narrow.get(), words * 4, p->stream)) return rc;
        }
    }
    if (out_n) *out_n = n;
    return KICP_OK;
}
// Background download: the copy runs on its own stream while the caller goes on with the next steps (downsampling,
// registration, map update), and lands in pinned memory; _finish waits for it and hands the points over.
int kicp_pre_download_begin(kicp_pre *p, int buffer) {
    KICP_TRACE_CALL();
    if (!p || buffer < 0 || buffer >= KICP_PRE_BUFFERS) return fail(KICP_ERR_ARG, "bad argument");
    if (int rc = set_device(p->device)) return rc;
    if (int rc = egress_settle(p)) return rc;
    const size_t n = p->buf_n[buffer];
    if (int rc = transfer_queue(p, buffer, n, nullptr)) return rc;  // (the buffer is final already: nothing to wait for)
    p->egress.buffer = buffer, p->egress.n = n, p->egress.rec_bytes = 24;
    return KICP_OK;
}
// ... and the worker moves the landed bytes into the caller's memory while the calling thread goes on with the pipeline (it waits for
// the transfer's events, piece by piece); _finish only joins it
int kicp_pre_download_begin_into(kicp_pre *p, int buffer, double *out_xyz, size_t cap_points) {
    if (int rc = kicp_pre_download_begin(p, buffer)) return rc;
    egress_post(p, transfer_job(out_xyz, cap_points, p->egress.n));
    return KICP_OK;
}
int kicp_pre_download_finish(kicp_pre *p, int buffer, double *out_xyz, size_t cap_points, size_t *out_n) {
    KICP_TRACE_CALL();
    if (!p || buffer < 0 || buffer >= KICP_PRE_BUFFERS) return fail(KICP_ERR_ARG, "bad argument");
    auto &g = p->egress;
    if (g.buffer != buffer) return fail(KICP_ERR_ARG, "no download of this buffer in flight: kicp_pre_download_begin first");
    if (int rc = set_device(p->device)) return rc;
    bool delivered = false;
    if (g.job_out) {  // the worker owns this download: wait for it
        if (int rc = egress_join(p)) return rc;
        delivered = g.dst == out_xyz || out_xyz == nullptr;
    }
    if (!delivered) {
        HIP_TRY(hipEventSynchronize(g.done));
        const size_t k = std::min(g.n, cap_points);
        if (k && out_xyz && g.rec_bytes != 24) {  // (a frame's FLOAT32 records land in the caller's own buffer only)
            g.buffer = -1;
            return fail(KICP_ERR_ARG, "the frame's FLOAT32 records went to the kicp_pre_frame*_f32 call's out_frame_xyz: collect with NULL");
        }
        if (k && out_xyz) std::memcpy(out_xyz, g.host.get(), k * 24);
    }
    if (out_n) *out_n = g.n;
    g.buffer = -1;
    return KICP_OK;
}
}  // extern "C"
