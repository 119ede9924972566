// kicp_map_cloud.hip -- VoxelHashMap::Pointcloud() behind include/kicp.h: from the host map, or - while the HBM copy is the current
// one - gathered on the device in the same table order (kernels: kicp_map_pc.hpp), as doubles (kicp_map_pointcloud) and as the
// FLOAT32 records the node publishes (kicp_map_pointcloud_f32).  kicp_map_internal.hpp says which of the map's units holds what.
#include "kicp_map_internal.hpp"
#include "kicp_map_pc.hpp"
#include "kicp_scan_blocks.hpp"  // k_scan_blocks

using namespace kicp;
using namespace kicp::host;

namespace {

constexpr hipStream_t kMapStream = nullptr;  // the map's kernels run on the null stream

// What both gathers begin with once their own buffers stand: the occupied points of every 256-slot block of the device table, then
// their running sums and, behind them, the total (d_pc_blocks[blocks])
int pc_count_blocks(kicp_map *map, hipStream_t st) {
    DeviceMirror &mr = map->mirror;
    const size_t slots = mr.live_slots, blocks = (slots + 255) / 256;
    if (int rc = mr.d_pc_blocks.reserve(blocks + 1)) return rc;
    hipLaunchKernelGGL(k_pc_count, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, st, mr.d_table.get(), mr.d_keys64.get(), static_cast<uint32_t>(slots), map->host.count_bits(), mr.d_pc_blocks.get());
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, st, mr.d_pc_blocks.get(), static_cast<uint32_t>(blocks), mr.d_pc_blocks.get() + blocks);
    return KICP_OK;
}

// ... and what both hold the table's own count against: the host's counters
int count_mismatch() { return fail(KICP_ERR_HIP, "device map counters disagree with the table"); }

// the HBM copy is the current one: gather the first `want` of its `total` points there (same table order) and download just them
int gather_f64(kicp_map *map, size_t total, size_t want, double *out_xyz) {
    DeviceMirror &mr = map->mirror;
    hipStream_t st = kMapStream;
    if (int rc = set_device(mr.device)) return rc;
    const size_t slots = mr.live_slots, blocks = (slots + 255) / 256;
    if (total > mr.d_pc.capacity() / 3)
        if (int rc = mr.d_pc.reserve((total + total / 4 + 1024) * 3)) return rc;
    if (int rc = pc_count_blocks(map, st)) return rc;
    hipLaunchKernelGGL(k_pc_gather, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, st, mr.d_table.get(), mr.d_keys64.get(), static_cast<uint32_t>(slots),
                       mr.d_pool.get(), map->host.cap(), map->host.count_bits(), mr.d_pc_blocks.get(), mr.d_pc.get());
    HIP_TRY(hipGetLastError());
    uint32_t counted = 0;
    HIP_TRY(hipMemcpy(&counted, mr.d_pc_blocks.get() + blocks, 4, hipMemcpyDeviceToHost));
    if (counted != total) return count_mismatch();
    return staged_download(mr.stage, out_xyz, mr.d_pc.get(), want * 24, st);
}

// the same as FLOAT32 records, written by the GPU into host-mapped landing slots piece by piece
int gather_f32(kicp_map *map, size_t total, size_t want, float *out_xyz) {
    DeviceMirror &mr = map->mirror;
    hipStream_t st = kMapStream;
    constexpr int kSlots = DeviceMirror::kRecSlots;
    // pieces of up to 64 Ki records (768 KB), at least four of them where the map allows, so that the copy of piece i into the
    // caller's memory runs while pieces i + 1 .. i + 3 are on their way; a multiple of 4 records keeps every piece 16-byte aligned
    const size_t piece = std::min<size_t>(65536, std::max<size_t>(1024, ((want + kSlots - 1) / kSlots + 1023) / 1024 * 1024));
    const size_t pieces = (want + piece - 1) / piece;
    if (int rc = set_device(mr.device)) return rc;
    const size_t slots = mr.live_slots, blocks = (slots + 255) / 256;
    if (piece * 12 * kSlots > mr.h_records.capacity())
        if (int rc = mr.h_records.reserve(piece * 12 * kSlots, hipHostMallocDefault)) return rc;
    if (!mr.h_rec_flags.get()) {
        if (int rc = mr.h_rec_flags.reserve(kSlots, hipHostMallocMapped | hipHostMallocCoherent)) return rc;
        std::memset(mr.h_rec_flags.get(), 0, kSlots * sizeof(unsigned long long));
    }
    if (!mr.d_rec_tickets.get()) {
        if (int rc = mr.d_rec_tickets.reserve(kSlots)) return rc;
        HIP_TRY(hipMemset(mr.d_rec_tickets.get(), 0, kSlots * sizeof(unsigned long long)));
        for (int s = 0; s < kSlots; ++s) mr.rec_drawn[s] = 0;
    }
    if (int rc = pc_count_blocks(map, st)) return rc;
    PcRecordParams q{};
    q.table = mr.d_table.get(), q.keys64 = mr.d_keys64.get(), q.slots = static_cast<uint32_t>(slots), q.cap = map->host.cap(), q.cbits = map->host.count_bits();
    q.blocks = static_cast<uint32_t>(blocks), q.pool = mr.d_pool.get(), q.block_offsets = mr.d_pc_blocks.get();
    // workgroups per piece: about as many as the piece has table blocks (the map's average records per block), at most 512
    const size_t per_block = std::max<size_t>(1, total / std::max<size_t>(1, blocks));
    const uint32_t grid = static_cast<uint32_t>(std::min<size_t>({blocks, 512, piece / per_block + 2}));
    uint32_t seqs[kSlots] = {};
    auto queue = [&](size_t i) -> int {
        const int s = static_cast<int>(i % kSlots);
        q.lo = static_cast<uint32_t>(i * piece), q.hi = static_cast<uint32_t>(std::min(want, (i + 1) * piece));
        q.dst = reinterpret_cast<float *>(mr.h_records.dev() + static_cast<size_t>(s) * piece * 12);
        mr.rec_drawn[s] += grid;
        q.ticket = mr.d_rec_tickets.get() + s, q.ticket_done = mr.rec_drawn[s], q.host_flag = mr.h_rec_flags.dev() + s;
        q.seq = ++mr.rec_seq;
        if (q.seq == 0u) q.seq = ++mr.rec_seq;  // (0 is what the flags hold before the first piece)
        seqs[s] = q.seq;
        hipLaunchKernelGGL(k_pc_records, dim3(grid), dim3(256), 0, st, q);
        HIP_TRY(hipGetLastError());
        return KICP_OK;
    };
    for (size_t i = 0; i < std::min<size_t>(pieces, kSlots); ++i)
        if (int rc = queue(i)) return rc;
    // each piece: wait for its flag, check the table's count it carries, copy the piece out, queue the piece that reuses its slot
    const volatile unsigned long long *flags = mr.h_rec_flags.get();
    for (size_t i = 0; i < pieces; ++i) {
        const int s = static_cast<int>(i % kSlots);
        const unsigned long long tag = static_cast<unsigned long long>(seqs[s]) << 32;
        unsigned long long flag = 0;  // (2 s: something is badly wrong then - surface it instead of spinning for ever)
        if (int rc = wait_word(flags + s, tag, 0xFFFFFFFF00000000ull, st, 2000.0, "a piece of the map's records was never announced", &flag)) return rc;
        if (static_cast<uint32_t>(flag & 0xFFFFFFFFull) != total) {
            HIP_TRY(hipStreamSynchronize(st));
            return count_mismatch();
        }
        const size_t lo = i * piece, n = std::min(want, lo + piece) - lo;
        std::memcpy(out_xyz + lo * 3, mr.h_records.get() + static_cast<size_t>(s) * piece * 12, n * 12);
        if (i + kSlots < pieces)
            if (int rc = queue(i + kSlots)) return rc;
    }
    map->update_counts[kCountRecordPieces] += pieces;  // (all of them, or the fallback answers and none counts)
    return KICP_OK;
}

}  // namespace

extern "C" {

size_t kicp_map_pointcloud(const kicp_map *cmap, double *out_xyz, size_t cap_points) {
    KICP_TRACE_CALL();
    if (!cmap) return 0;
    kicp_map *map = const_cast<kicp_map *>(cmap);  // logically const: only scratch buffers / the host copy are touched
    if (map_finish_pending(map) != KICP_OK) return 0;  // (the map this call would list is not the updated one)
    if (!map->device_ahead) return map->host.Pointcloud(out_xyz, out_xyz ? cap_points : 0);
    const size_t total = static_cast<size_t>(map->dev.n_points), want = out_xyz ? std::min(total, cap_points) : 0;
    if (want == 0 || gather_f64(map, total, want, out_xyz) == KICP_OK) return total;
    // a gather that failed, for whatever reason: the host copy, refreshed, is the answer
    return ensure_host_current(map) == KICP_OK ? map->host.Pointcloud(out_xyz, cap_points) : 0;
}
// The local map as the PointCloud2 `data` the node publishes (RosUtils.cpp:40-63 EigenToPointCloud2 of LocalMap(),
// LidarOdometryServer.cpp:240-263): x y z FLOAT32 records, Pointcloud()'s order, static_cast<float> of its doubles.
int kicp_map_pointcloud_f32(const kicp_map *cmap, float *out_xyz, size_t cap_points, size_t *out_total) {
    KICP_TRACE_CALL();
    if (!cmap || (!out_xyz && cap_points)) return fail(KICP_ERR_ARG, "null argument");
    kicp_map *map = const_cast<kicp_map *>(cmap);  // logically const, as kicp_map_pointcloud
    if (int rc = map_finish_pending(map)) return rc;  // (its error is this call's: the map it would list is not the updated one)
    auto on_host = [&]() -> int {  // the host copy is the current one (or has just been made so): narrow it here, the same bits
        const size_t total = map->host.num_points(), want = out_xyz ? std::min(total, cap_points) : 0;
        if (out_total) *out_total = total;
        if (want == 0) return KICP_OK;
        std::vector<double> xyz(want * 3);
        map->host.Pointcloud(xyz.data(), want);
        for (size_t k = 0; k < want * 3; ++k) out_xyz[k] = static_cast<float>(xyz[k]);
        return KICP_OK;
    };
    if (!map->device_ahead) return on_host();
    const size_t total = static_cast<size_t>(map->dev.n_points), want = out_xyz ? std::min(total, cap_points) : 0;
    if (out_total) *out_total = total;
    if (want == 0) return KICP_OK;
    if (total * 3 >= 0xFFFFFFF0ull) return fail(KICP_ERR_CAPACITY, "map too large for 32-bit record offsets");
    const int rc = gather_f32(map, total, want, out_xyz);
    if (rc == KICP_OK || ensure_host_current(map) != KICP_OK) return rc;
    return on_host();  // as kicp_map_pointcloud
}

}  // extern "C"
