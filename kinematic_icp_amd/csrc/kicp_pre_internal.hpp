// kicp_pre_internal.hpp -- what the translation units of the pipeline's pre-steps (kicp_pre*.hip) share: the handle behind kicp_pre,
// the rules its entries keep, and what more than one of them calls.  include/kicp.h states the semantics.  The pieces, each the only
// translation unit that includes its kernel header:
//   kicp_pre.hip         the steps and the fused chain (kicp_pre.hpp; the block scan, kicp_scan_blocks.hpp, it shares with kicp_map_cloud.hip):
//                        create / destroy, the options and the probe limit, kicp_pre_upload, kicp_pre_device_ptr, kicp_pre_preprocess*,
//                        kicp_pre_voxel_downsample, kicp_pre_frame*
//   kicp_pre_ingest.hip  a sensor message into the ingest slot (kicp_pre_ingest.hpp): kicp_pre_ingest, _ingest_scan, _ingest_ahead and
//                        the look-ahead's job, kicp_pre_ingested, _ingested_count, kicp_pre_ahead_hits
//   kicp_pre_egress.hip  the way back (kicp_pre_egress.hpp): kicp_pre_download, _download_f32, _download_begin, _begin_into, _finish, the
//                        copy worker, and the push of a chained frame (egress_start_frame)
#pragma once
#include "kicp_internal.hpp"
#include "kicp_pre_shared.hpp"  // kPushPieces, the words of d_misc and h_rec

// (an internal header of three translation units that all begin this way)
using namespace kicp;
using namespace kicp::host;

// THREE THREADS touch a handle: the CALLER's (one at a time: include/kicp.h), the LOOK-AHEAD thread (ahead.thread, runs ahead_run)
// and the COPY WORKER (egress.worker, runs egress_job).  Either helper runs one job at a time, and `job_out` of its group says that one
// is out.  Each group below states who may write it; what it does not mention, only the caller writes, and only while no job that
// reads it is out.
//
// CONST ENTRIES (kicp_pre_download*, kicp_pre_ingested) move data through `stage`, which is mutable; kicp_pre_download_f32 also grows
// its narrowing scratch and says so where it casts.
struct kicp_pre {
    int device = 0;
    hipStream_t stream = nullptr;
    // ---- BUFFERS AND TABLES.  The caller alone writes them.  The look-ahead thread reads cap_n, d_block_minmax's address and
    // h_rec's; the copy worker reads buf[0]'s address and polls h_rec[kRecPush ..].  pre_ensure joins the look-ahead before anything
    // here grows.  Every device and pinned buffer is an owner (kicp_internal.hpp): kicp_pre_destroy tears streams, events and threads
    // down explicitly, the memory goes with `delete`.
    DevBuf<double> buf[KICP_PRE_BUFFERS];  // 3 doubles per point
    size_t buf_n[KICP_PRE_BUFFERS] = {};
    DevBuf<double> d_in, d_ts, d_staged;  // (these, the second slot, the flags, counts and tables: sized together by pre_ensure, for cap_n points)
    DevBuf<uint32_t> d_flags, d_block_counts;
    DevBuf<uint32_t> d_misc;                 // kMiscWords words: kicp_pre_shared.hpp lays them out
    PinnedBuf<unsigned long long> h_rec;     // kRecWords words, host-coherent: kicp_pre_shared.hpp lays them out
    DevBuf<unsigned long long> d_block_minmax;
    DevBuf<unsigned char> d_table;  // downsampling table: keys | min_index | order | home_at, 20 B per bucket (table_at)
    DevBuf<unsigned char> d_table2;  // the fused chain's table of the second level (the first level's is still being emptied when it fills)
    DevBuf<uint32_t> d_counts1, d_counts2;  // the fused chain's occupied-bucket counts per tile of either table
    size_t cap_n = 0, table_slots = 0;
    bool table_clean = false;  // every byte of d_table / d_table2 is 0xFF (what a downsample needs to find; its gather step leaves it so)
    uint32_t last_max_probe = 0;
    // longest probe the reference's tsl::robin_map tolerates before it grows its table instead (kicp_pre_set_probe_limit)
    uint32_t probe_limit = static_cast<uint32_t>(env_int("KICP_ROBIN_PROBE_LIMIT", 128));
    unsigned long long scan_launches = 0;  // k_scan_blocks launches of this handle (kicp_pre_get_option "scan_launches")
    mutable HostStage stage;  // pinned staging for transfers from / to caller memory

    // ---- THE FUSED CHAIN (k_frame_*).  Caller only.  The survivor count its table size is guessed from (0: none yet), its sequence
    // number, how often the guess was wrong (the unfused steps then run from buffer 0 on) and how the last frame was laid out
    // (kicp_pre_get_option "point_tiles" .. "l2_tiles", include/kicp.h): host-side bookkeeping.  `ready` is recorded on `stream` by the
    // caller and waited for on egress.stream by whoever queues the frame's way back, the copy worker included.
    struct {
        bool fused = env_flag("KICP_PRE_FUSED", true);
        uint32_t spec_tiles_b = 0;  // 256-bucket tiles of the previous frame's second-level table (sizes that level's launches)
        uint32_t spec_n0 = 0, spec_n_in = 0;  // (... and the input count it belonged to: the guess scales with the frame)
        uint32_t seq = 0;
        unsigned long long spec_misses = 0, fused_frames = 0;
        uint32_t last_point_tiles = 0, last_l1_tiles = 0, last_l2_workgroups = 0, last_l2_tiles = 0;
        hipEvent_t ready = nullptr;  // chained pre-steps: buffer 0 is complete (its way back may start)
    } chain;

    // ---- WIRE-FORMAT INGEST: what d_in / d_ts currently hold.  The caller writes all of it.  The look-ahead thread, while its job is
    // out, is the only writer of seq, ticket_drawn[1] and counts[1], and may let d_raw grow (where the device cannot read the
    // staging buffer) - every kicp_pre_ingest* call joins it first, so the two never decode at the same time.
    struct IngestCounts {
        unsigned launches = 0, workgroups = 0;  // k_ingest launches / workgroups of the widest of them
        int aligned = 0, wide = 0, direct = 0;
        size_t piece_records = 0;
    };
    struct {
        DevBuf<unsigned char> d_raw;  // the raw message bytes (only where the device cannot read the staging buffer)
        double ts_lo = 0.0, ts_hi = 0.0;  // d_ts holds the stamps in seconds; consumers normalise with these (PreprocessParams::ts_normalise)
        bool ts_raw = false;
        size_t n = 0;
        bool valid = false, stamps = false;  // an ingested cloud is in d_in (kicp_pre_frame_ingested may run) / it has stamps
        DevBuf<unsigned long long> d_ticket;  // [2] the ingest kernels' tickets (never reset), one per record
        unsigned long long ticket_drawn[2] = {0ull, 0ull};
        unsigned long long seq = 0;
        IngestCounts counts[2];  // which way the last ingest_run went ([0] this call's message, [1] the look-ahead's; "ingest_*" / "ahead_*" options)
        hipStream_t stream2 = nullptr;  // this call's message: its pieces' decodes alternate between the handle's stream and this one
    } ingest;

    // ---- LOOK-AHEAD INGEST (kicp_pre_ingest_ahead): the NEXT message is uploaded and decoded into a second slot (d_in2 / d_ts2) on a
    // stream of its own by the kicp_pre_frame* call of the CURRENT one - while that call's kernels run and its thread would only wait -,
    // and the kicp_pre_ingest call for the same message then just swaps the slots.  The caller writes the announcement (data .. pose,
    // state 0 / 1) and job_out; the look-ahead thread, while its job is out, writes state = 2, lo, hi, edge, the second slot's contents,
    // `stream` (created on first use) and `stage`.  ahead_join ends the job before the caller looks at any of it.
    struct Ahead {
        const void *data = nullptr;
        size_t n = 0;
        kicp_cloud_layout layout{};
        bool has_pose = false;
        Pose pose{};
        int state = 0;  // 0 none | 1 announced | 2 in the second slot
        double lo = 0.0, hi = 0.0;
        // what the first and the last 64 bytes of the message were when it was uploaded: a caller that reuses one receive buffer and hands
        // over ANOTHER message of the same size at the same address (against the contract) is caught instead of served the stale cloud
        unsigned char edge[128] = {};
        size_t edge_bytes = 0;
        DevBuf<double> d_in2, d_ts2;
        hipStream_t stream = nullptr;
        HostStage stage;               // its own pinned staging buffer (the calling thread goes on using the handle's meanwhile)
        unsigned long long hits = 0;   // kicp_pre_ingest calls that found their message decoded ahead (kicp_pre_ahead_hits)
        JobThread thread;              // queues the look-ahead upload beside the calling thread's own kernels
        bool job_out = false;          // ... and is only waited for where its result (or a buffer it uses) is needed: ahead_join
    } ahead;

    // ---- 2-D LASERSCAN INGEST (kicp_pre_ingest_scan).  Caller only.  The projector's cosine table in HBM and the key it was built for
    // (kicp_pre_ingest.hpp laser_rules: one table per projector, kept while n, angle_min and angle_max stay the same)
    struct {
        DevBuf<unsigned char> d_cs;  // (doubles; sized in bytes)
        std::vector<double> cs_host;
        bool valid = false;
        size_t n = 0;
        float angle_min = 0.0f, angle_max = 0.0f;
    } scan;

    // ---- THE WAY BACK (kicp_pre_download*, and the frame a kicp_pre_frame* call returns).  The caller writes all of it, and only
    // while no job is out, but for `n`: the chain corrects it to the real count while the job of its frame runs, and the worker never
    // reads it.  The worker reads what its EgressJob says (handed over by value at post), the addresses of `host`, `stream`, `done`
    // and buf[0], chain.ready, and h_rec[kRecPush ..]; it creates the events of piece_done it finds missing when it queues a transfer
    // itself.  egress_settle / kicp_pre_download_finish end the job.
    static constexpr int kCopyPieces = 3;
    struct {
        hipStream_t stream = nullptr;  // the download's own stream
        hipEvent_t done = nullptr;     // ... and the event behind its last transfer
        // a frame-sized transfer goes in pieces, an event behind each: the worker moves piece i into the caller's memory while piece i + 1
        // is on its way (one 3 MB copy behind one 3 MB transfer made the frame wait for the CPU's copy, ~60 us)
        hipEvent_t piece_done[kCopyPieces] = {};
        PinnedBuf<unsigned char> host;  // the landing area (dev() == nullptr: not mapped - the DMA engine moves the frame)
        int buffer = -1;                // the buffer whose download is in flight (-1: none)
        size_t n = 0;                   // the points _finish REPORTS
        size_t rec_bytes = 24;          // bytes per point of the download in flight: 24 (fp64) or 12 (the FLOAT32 records of kicp_pre_frame*_f32)
        void *dst = nullptr;            // where the job out (or the last one) delivers
        JobThread worker;               // moves the landed bytes into the caller's memory while the caller goes on with the pipeline
        bool job_out = false;
        DevBuf<unsigned long long> d_push_tickets;  // [kPushPieces] device counters of k_push_frame, never reset
        unsigned long long push_drawn = 0;
        uint32_t push_seq = 0;
        // read-only diagnostics (kicp_pre_get_option "push_launches" / "push_pieces"): push kernels queued by the caller's thread; pieces
        // the worker has followed to their flag - written by the worker, read once its job has been joined
        unsigned long long push_launches = 0, push_pieces = 0;
        // the registration source (buffer 2, ~100 KB) also lands in host memory as the fused chain's last launch writes it: the pipeline
        // returns it too (KinematicICP.cpp:84), and a copy + stream synchronisation for it cost the frame ~40 us
        PinnedBuf<unsigned char> h_src;  // (dev() == nullptr: not mapped)
        bool src_on_host = false;  // h_src holds buffer 2's current contents - once h_rec[kRecSrcHost] carries src_seq (k_frame_src_host)
        bool src_f32 = false;      // ... as x y z FLOAT32 records (the frame came through kicp_pre_frame*_f32), not as doubles
        uint32_t src_seq = 0;
        DevBuf<float> d_narrow;    // kicp_pre_download_f32 of a buffer without a host copy: its records in HBM
    } egress;
};

namespace kicp {
namespace host {
constexpr const char *kPreLost = "the pre-step kernels finished without handing their result over";  // (wait_word, 2 ms)
// ---- kicp_pre.hip
int pre_ensure(kicp_pre *p, size_t n);  // the ingest slots, flags, counts and tables hold n points (joins the look-ahead before they grow)
// ---- kicp_pre_ingest.hip
int ahead_join(kicp_pre *p);  // the look-ahead upload, if one is out, is over behind this
int ahead_post(kicp_pre *p, bool *posted);  // the announced message, if there is one that fits, goes up now on the look-ahead thread
// ---- kicp_pre_egress.hip
// the frame a chained call returns starts its way back (n_in points at most; `out` == nullptr: nothing to do), behind chain.ready
int egress_start_frame(kicp_pre *p, size_t n_in, void *out, size_t cap_points, bool f32);
void egress_destroy(kicp_pre *p);  // the worker, the stream and the events (kicp_pre_destroy)
}  // namespace host
}  // namespace kicp
