/* kicp.h -- C-ABI of the MI355X-native kinematic-ICP registration hot path (libkicp_amd.so).
 *
 * Drop-in boundary #2 of SURVEY.md section 8(b): everything the reference's
 *   kinematic_icp::KinematicRegistration      (cpp/kinematic_icp/registration/Registration.hpp:32-50)
 *   kiss_icp::VoxelHashMap (kiss-icp v1.2.0)  (used at registration/Registration.cpp:63,74,152,157,
 *                                              pipeline/KinematicICP.hpp:79,88,92 and KinematicICP.cpp:79)
 * need from a backend, as plain C: opaque handles, pointers and sizes, no C++/torch types - plus, further down, the
 * steps either side of that path in KinematicICP::RegisterFrame: kicp_pre_* for the wire-format
 * ingest, deskew + crop + downsample (pipeline/KinematicICP.cpp:31-62, ros/.../RosUtils.cpp:30-39,
 * TimeStampHandler.cpp:57-128) and kicp_map_update_pose_device / kicp_map_pointcloud for the map side (KinematicICP.cpp:79,
 * KinematicICP.hpp:92).
 *
 * Conventions
 *   points : contiguous AoS float64 xyz (the memory layout of std::vector<Eigen::Vector3d>, so
 *            `frame.data()->data()` can be passed without a copy).
 *   poses  : double[7] = [qx, qy, qz, qw, tx, ty, tz] (Sophus::SE3d parameter order).
 *   return : 0 = OK;  >0 = warning, result still follows the reference convention (e.g. NaN pose on
 *            zero correspondences, Registration.cpp:56-58,119-125);  <0 = backend error, outputs untouched.
 *   threads: one handle is used by one host thread at a time (the reference is called from a single ROS
 *            executor thread; SURVEY.md section 8b "Threading").
 * There is NO CPU fallback: if no gfx950 device / HIP runtime is usable, *_create fails with KICP_ERR_HIP.
 */
#ifndef KICP_H_
#define KICP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KICP_VERSION 100
#define KICP_MAX_LOG_PASSES 32

enum {
    KICP_OK = 0,
    KICP_WARN_NO_CORRESPONDENCES = 1, /* N_corr == 0 in some pass -> NaN pose, as the reference produces */
    KICP_WARN_TABLE_ORDER = 2,        /* kicp_pre_voxel_downsample: the survivors are the reference's, but a robin-hood probe exceeded the
                                         limit at which tsl::robin_map re-hashes mid-way: their ORDER may differ (kicp_pre_set_probe_limit) */
    KICP_ERR_HIP = -1,                /* HIP runtime / device failure (message in kicp_last_error) */
    KICP_ERR_ARG = -2,                /* bad argument */
    KICP_ERR_CAPACITY = -3,           /* a documented limit exceeded (max_points_per_voxel > 65 535, more voxels than the table's bucket
                                         index addresses - 2^24-2 at <= 255 points per voxel -, a per-point term of the normal
                                         equations >= 2^43: source points ~2 900 km from the base frame, a voxel coordinate beyond
                                         +-2^20 in kicp_pre_voxel_downsample) */
    KICP_ERR_COMM = -4,               /* a multi-GPU exchange failed (RCCL, peer mailboxes, shared segment): a peer did not show up in time */
    KICP_ERR_INTERNAL = -5            /* a bound the library proves for itself did not hold (kicp_grid_potential's round limit): a bug, please report */
};

typedef struct kicp_map kicp_map; /* twin of kiss_icp::VoxelHashMap: host-authoritative voxel map + HBM mirror */
typedef struct kicp_reg kicp_reg; /* twin of kinematic_icp::KinematicRegistration + device workspace/stream */

/* Constructor arguments / public fields of KinematicRegistration (Registration.hpp:33-37,45-49). */
typedef struct kicp_reg_config {
    int32_t max_num_iterations;
    double convergence_criterion;
    int32_t max_num_threads; /* kept for API parity; the HIP path ignores it */
    int32_t use_adaptive_odometry_regularization;
    double fixed_regularization;
} kicp_reg_config;

/* Per-call diagnostics (SURVEY.md section 5 "Metrics"): what the reference computes internally but never exposes. */
typedef struct kicp_stats {
    int32_t iterations; /* ComputePerturbation evaluations executed (Registration.cpp:179-187) */
    int32_t converged;  /* 1 if ||dx|| < convergence_criterion ended the loop (Registration.cpp:184) */
    int32_t empty_map;  /* 1 if the early-out of Registration.cpp:157 fired */
    int32_t reserved;
    double beta;                            /* regularisation used (Registration.cpp:171-177) */
    double n_corr[KICP_MAX_LOG_PASSES];     /* correspondences per pass */
    double sums[KICP_MAX_LOG_PASSES][6];    /* raw JTJ00, JTJ01, JTJ11, JTr0, JTr1, sum||r||^2 per pass */
    double dx[KICP_MAX_LOG_PASSES][2];      /* solved (displacement, yaw) per pass */
    double gpu_ms;                          /* device time of the call, HIP events on the handle's stream ("timing" >= 1) */
    double pass_ms[KICP_MAX_LOG_PASSES];    /* device time of each fused pass kernel, HIP events around the launch ("timing" == 2) */
} kicp_stats;

const char *kicp_last_error(void); /* thread-local, valid until the next failing call on this thread */
int kicp_version(void);
int kicp_device_count(void); /* number of visible HIP devices, <0 on runtime failure */
/* Where the host should run the thread that calls this library for `device`: the NUMA node the GPU is attached to (-1: unknown) and
 * its CPUs as the kernel prints them ("0-63,128-191"; empty: unknown), from /sys/bus/pci/devices/<bdf>/{numa_node,local_cpulist}.
 * The library places its own helper threads and pinned buffers there (KICP_NUMA=0: not); the caller's thread is the caller's to
 * place - a frame is ~5 % faster from that node and ~10 % from inside one L3 domain of it. */
int kicp_device_locality(int device, int *out_numa_node, char *out_cpulist, size_t cap);

/* ---- kiss_icp::VoxelHashMap (kiss-icp v1.2.0 core/VoxelHashMap.hpp) ------------------ */
/* VoxelHashMap(voxel_size, max_distance, max_points_per_voxel)   -- pipeline/KinematicICP.hpp:79 */
int kicp_map_create(double voxel_size, double max_distance, unsigned int max_points_per_voxel, kicp_map **out);
void kicp_map_destroy(kicp_map *map);
/* VoxelHashMap(const VoxelHashMap &): the reference's map is copyable (it holds its tsl::robin_map by value); a deep copy
 * of the newest state (pulled back from the GPU first if the device copy is ahead), with its own HBM mirror on first use */
int kicp_map_clone(const kicp_map *map, kicp_map **out);
int kicp_map_clear(kicp_map *map);                                           /* Clear()  -- KinematicICP.hpp:88 */
int kicp_map_empty(const kicp_map *map);                                     /* Empty()  -- Registration.cpp:157 */
int kicp_map_add_points(kicp_map *map, const double *xyz, size_t n);         /* AddPoints(points) */
int kicp_map_remove_far(kicp_map *map, const double origin[3]);              /* RemovePointsFarFromLocation(origin) */
int kicp_map_update_origin(kicp_map *map, const double *xyz, size_t n, const double origin[3]); /* Update(points, origin) */
int kicp_map_update_pose(kicp_map *map, const double *xyz, size_t n, const double pose_qt[7]);  /* Update(points, pose) -- KinematicICP.cpp:79 */
/* Update(points, pose) with the points already in HBM (e.g. a kicp_pre buffer): transform, AddPoints and
 * RemovePointsFarFromLocation run on the device - every touched voxel's new points are judged in input order with the
 * reference's fp64 rule (one wave per voxel for frame-sized updates, one thread per voxel for bulk insertions), so the
 * accepted points and their order inside each voxel are exactly the sequential reference's.  Table growth / clean-up (a
 * device-side re-hash) and pool growth happen in HBM as well; the host copy is refreshed lazily when a host-side call
 * (AddPoints, kicp_map_check, ...) needs it.  A map that leaves +-2^20 voxels from its origin is updated by the host map
 * from then on (same result). */
int kicp_map_update_pose_device(kicp_map *map, int device, const double *d_points_xyz, size_t n, const double pose_qt[7]);
/* The same update in two halves (round 4): _begin queues the update's kernels and returns WITHOUT waiting for them, so that the caller
 * can do host-side work that does not touch the map meanwhile (the drop-in RegisterFrame collects the frame's two returned clouds);
 * kicp_map_update_finish waits and takes the result over (host fallback included).  d_points_xyz stays borrowed until then.  Only
 * frame-sized updates into a table with room for the worst case are actually deferred; every other case runs to completion inside
 * _begin.  Any other call on the map finishes a pending update first, so forgetting _finish costs nothing but the overlap. */
int kicp_map_update_pose_device_begin(kicp_map *map, int device, const double *d_points_xyz, size_t n, const double pose_qt[7]);
int kicp_map_update_finish(kicp_map *map);
int kicp_map_last_update_on_device(const kicp_map *map); /* 1 if the last kicp_map_update_pose_device ran on the GPU (collects a pending update first) */
/* Updates so far that ran on the GPU and have been collected; unlike every other call on the map this one does NOT wait for a pending
 * update (a diagnostic a timed loop can read without disturbing what it measures). */
unsigned long long kicp_map_device_updates(const kicp_map *map);
/* Which way this map's updates went so far - a read-only diagnostic for tests and tuning: host-side counters only, no device call, and
 * like kicp_map_device_updates it does NOT collect a pending update.  kicp_map_clear keeps them.  out[]:
 *   0  updates queued as ONE queue of kernels (<= 16384 points into a table with room for the worst case)
 *   1  staged updates (claim, ask the device, then apply)        2  second claims of a staged update after a "too tight" re-hash
 *   3  device-side re-hashes                                     4  pool growths that reallocated
 *   5  launches of the wave-per-voxel insertion kernel           6  launches of the thread-per-voxel insertion kernel
 *   7  scans over many workgroups (> 16384 points)               8  updates handed to the host map
 *   9  updates left pending by kicp_map_update_pose_device_begin
 *  10  voxels touched by the last collected device-side update
 *  11  pieces of kicp_map_pointcloud_f32 calls that the device announced and the host copied out (calls answered from the host
 *      copy, the fallback behind a failed device path included, leave it alone) */
int kicp_map_update_counts(const kicp_map *map, unsigned long long out[12]);
/* Preferred device for BULK host-side insertions (not part of the reference API): with device >= 0, kicp_map_add_points /
 * kicp_map_update_origin / kicp_map_update_pose calls of 4096 points or more stage their points into HBM and insert them
 * there (the same map as the sequential host insertion builds, an order of magnitude faster); -1 (default) = always on the
 * host.  Small calls stay on the host either way. */
int kicp_map_set_device(kicp_map *map, int device);
size_t kicp_map_num_points(const kicp_map *map);
size_t kicp_map_num_voxels(const kicp_map *map);
/* Pointcloud() -- KinematicICP.hpp:92.  Writes min(cap_points, total) points, returns total (0 if a pending update fails). */
size_t kicp_map_pointcloud(const kicp_map *map, double *out_xyz, size_t cap_points);
/* The same cloud as the PointCloud2 `data` the node publishes for it (ros/.../utils/RosUtils.cpp:40-63 EigenToPointCloud2 of
 * LocalMap(), called from LidarOdometryServer.cpp:240-263 PublishClouds): x y z FLOAT32 records of 12 bytes (offsets 0 4 8,
 * little-endian), static_cast<float> of kicp_map_pointcloud's doubles, its order and its count.  Writes min(cap_points, total)
 * records (out_xyz may be NULL with cap_points 0: *out_total only).  A map whose HBM copy is the current one is narrowed on the
 * GPU, which writes the records into host-mapped memory piece by piece (kicp_map_pc.hpp k_pc_records; no fp64 copy crosses
 * PCIe); a map that lives on the host is narrowed there, with the same bits.  Unlike kicp_map_pointcloud it returns an error
 * code: a pending deferred update is collected first and its error is returned. */
int kicp_map_pointcloud_f32(const kicp_map *map, float *out_xyz, size_t cap_points, size_t *out_total);
/* GetClosestNeighbor(query) for n queries -- Registration.cpp:74.  Host arrays in/out; runs on `device` the plain fp64 search
 * over the 27 neighbour voxels (kicp_nn_exact.hpp search_global: the reference's loop, and the exact fallback of the fused pass
 * kernels - NOT their mirror pre-selection: what the shipped pass kernels pick per query is what kicp_pass_correspondences returns).
 * No candidate -> nn = (0,0,0), dist = DBL_MAX, exactly like the reference. */
int kicp_map_closest(kicp_map *map, int device, const double *queries_xyz, size_t n, double *out_nn_xyz, double *out_dist);
/* The map as a file: PCD v0.7, DATA binary - FIELDS x y z, SIZE 8 8 8, TYPE F F F, COUNT 1 1 1, WIDTH n, HEIGHT 1, POINTS n, the points of
 * kicp_map_pointcloud in its order - with one comment line `# kicp_map voxel_size=<%.17g> max_distance=<%.17g> max_points_per_voxel=<u>`.
 * Written to `path`.tmp and renamed.  Works wherever the newest state lives; a pending update is collected first, its error returned. */
int kicp_map_save_pcd(const kicp_map *map, const char *path);
/* The three parameters the map was created with (any of the outputs may be null). */
int kicp_map_params(const kicp_map *map, double *out_voxel_size, double *out_max_distance, unsigned int *out_max_points_per_voxel);
/* A new map from a PCD file (this library's or a mapping tool's): binary data only; x, y, z must be TYPE F of SIZE 4 or 8 (floats are
 * widened with static_cast<double>) and COUNT 1, other fields are skipped; header lines in any order, comments anywhere; the number of
 * points is POINTS, or WIDTH x HEIGHT without it.  voxel_size <= 0: the three parameters come from the file's `# kicp_map` line
 * (KICP_ERR_ARG without one).  Non-finite points are dropped and counted; the others are inserted in file order - on `device` through
 * the bulk insertion of kicp_map_set_device(map, device) when device >= 0, otherwise on the host - which reproduces every voxel's points
 * in their order (the order of the voxels among themselves may differ; no registration result depends on it).  DATA ascii /
 * binary_compressed, a missing field, a short file: KICP_ERR_ARG with a message that names the problem, *out = NULL.
 * out_points_read (rows of the file) and out_points_dropped may be null. */
int kicp_map_load_pcd(const char *path, double voxel_size, double max_distance, unsigned int max_points_per_voxel, int device, kicp_map **out,
                      size_t *out_points_read, size_t *out_points_dropped);
/* Debug aid: verifies the table invariants the kernels rely on (neighbour masks, bucket records, halo entries, fp32
 * mirror, counters) on the host copy; returns the number of violations, 0 when consistent. */
size_t kicp_map_check(const kicp_map *map);
/* Make the HBM mirror on `device` current (a no-op when nothing changed since the last upload).
 * kicp_register* call it implicitly; exposed so map upload can be kept out of a timed region. */
int kicp_map_sync(kicp_map *map, int device);
/* What the last upload of the mirror moved: bytes sent host->device and whether it was a full re-send (1) or a delta
 * of the changed table slots / buckets (0).  A re-hash of the table or Clear() forces a full re-send. */
int kicp_map_last_upload(const kicp_map *map, size_t *bytes, int *was_full);

/* ---- kinematic_icp::KinematicRegistration (registration/Registration.hpp:32-50) ------------------------- */
int kicp_reg_create(const kicp_reg_config *config, int device, kicp_reg **out);
void kicp_reg_destroy(kicp_reg *reg);
/* KinematicRegistration(const KinematicRegistration &): the reference's struct is a plain copyable aggregate
 * (Registration.hpp:32-50).  A new handle on the same device with the same parameters and tuning options and workspaces of
 * its own (stream, queue, hand-off buffers).  Multi-GPU exchanges are per handle and are not carried over. */
int kicp_reg_clone(const kicp_reg *reg, kicp_reg **out);
int kicp_reg_get_config(const kicp_reg *reg, kicp_reg_config *out);
int kicp_reg_set_config(kicp_reg *reg, const kicp_reg_config *config); /* the reference's fields are public & mutable */
/* Backend tuning knobs (not part of the reference API).  Twenty settable options; everything that lost its A/B over five rounds
 * (other workgroup sizes and register budgets, the plain fp64 gather, the device-side solve, single-record hand-offs, ...) was deleted
 * in round 6, and the pass kernels' ablation switches ("dbg") exist in libkicp_amd_dbg.so only (make -C kinematic_icp_amd/csrc dbg).
 * Which kernel runs:
 *   "lanes_per_query"  sub-lanes sharing one query of the generic pass kernel (1 | 2 | 4; 0 = by scan size, default: 4 up to 4 096 points,
 *                  2 up to 32 768, else 1)
 *   "latency_kernel" one lane per query: 1 (default) scans of at most 131 072 points - which leave the device two waves per SIMD
 *                  anyway - run the build that has TWO neighbour voxels in flight per round; 2: every such scan; 0: never (the
 *                  four-waves-per-SIMD build)
 *   "pass_tiles"   blocks of 256 queries a workgroup of the one-lane-per-query four-waves build serves before its one epilogue:
 *                  0 (default) by scan size and scans in flight - more than one only while the passes in flight keep at least 1.5
 *                  workgroups per workgroup slot of the device (cfg2 in a batch: 2) -, or 1 | 2 | 4 (other values are clamped to the next of these below).  Changes no bit of a
 *                  result: the sums are exact.  The other builds serve one block per workgroup whatever the value.
 *   "small"        1 (default): scans of at most 16 384 lanes (points x sub-lanes) take the small-scan path - the kernel stays resident for
 *                  the iterations of a call, polling for the next pose; 0: always the generic pass kernel
 *   "small_wave"   1 (default): scans of at most 4 096 points run ONE WAVE PER QUERY (k_pass_wave); 0: sub-lanes per query (k_pass_small)
 *   "small_resident" 1 (default): resident unless the previous call converged in one iteration; 2: always; 0: one launch per iteration.
 *                  A resident kernel holds the CUs it runs on until its host answers (at most "small_timeout_us"): set 0 where several
 *                  threads or processes register small scans on one device
 *   "small_timeout_us" how long a resident workgroup waits for the next command before it leaves on its own (default 20 000; the host
 *                  then launches afresh)
 *   "resident_generic" 1 (default): scans beyond the small-scan kernels and up to 131 072 points keep the generic kernel's latency build
 *                  resident for the later iterations of a call too; 0: one launch per iteration
 * Batches of independent scans (kicp_register_device_batch):
 *   "batch_queues"   (default 8, 0 .. 16) scans in flight at a time, on batch_queues / batch_group handles with an HSA queue each; < 2: off
 *   "batch_group"    (default 4, 1 .. 8) scans whose passes share ONE launch of the pass kernel on such a queue (a 2-D grid: a job per scan);
 *                  1: a launch per scan and pass, each scan on a queue of its own.  That is also what sharded batches, batches too short to
 *                  give every queue two groups and batches in which most scans take another kernel (the small-scan kernels, sub-lanes per
 *                  query) run: on min("batch_queues", 8) queues once the caller has set "batch_queues", on four until then
 *   "batch_resident" 1 (default): batches "batch_queues" does not take keep ONE resident kernel across the batch's scans; 0: scan by scan
 *   "batch_depth"    (default 3, 1 .. 4) scans that kernel has in flight
 *   "batch_threads"  (default 8, 0 .. 9) batches of scans that leave most of the device empty: up to this many resident kernels side by
 *                  side, a host thread of the library's pool each (capped by the CPUs this process may use: cpuset and cgroup quota)
 *   "batch_rotate"   1 (default): the workgroups of a resident kernel take turns at the parts of a scan; 0: fixed shares
 * One frame at many poses (kicp_score_poses, kicp_planar_sums, kicp_refine_poses_planar, kicp_relocalize, kicp_relocalize_planar):
 *   "score_chunk"  (default 8 388 608) queries - pose x point pairs - one launch of the scoring kernel may serve; 0: the default
 * The branch-and-bound search (kicp_search_poses, kicp_relocalize_search):
 *   "search_max_nodes" (default 67 108 864 = 2^26) nodes one call may score before it gives up with KICP_ERR_CAPACITY; 0: the default
 * Transfers and launches:
 *   "bar_frame"    1 (default): kicp_register writes host frames of up to 8 192 points straight into HBM through the PCIe BAR
 *   "fetch_upload" 1 (default): larger host frames are pulled out of the pinned staging buffer by a small kernel per piece; 0: DMA engine
 *   "aql"          1 (default): pass kernels are dispatched with hand-written AQL packets on the handle's own HSA queue; 0: HIP launches
 *   "wait"         0 (default): poll the tagged rows in host memory; 1: hipStreamSynchronize
 *   "timing"       1: kicp_stats.gpu_ms from HIP events; 2: also kicp_stats.pass_ms[]
 * Read only: "small_active" (path of the last call: 0 generic, 1 sub-lanes, 2 wave per query), "resident_passes", "batch_queue_passes",
 *   "batch_resident_passes", "batch_threads_active", "small_relaunches", "score_launches", "score_items_per_workgroup" (the most tile x pose items one
 *   workgroup served in a launch of the last scoring call), "search_nodes_scored", "search_launches", "search_yaw_trips" (yaws one workgroup of
 *   the last call's cell kernel served), "aql_active", "aql_kernarg", "comm_ranks".
 * Test hooks (exercise fall-backs that this hardware does not reach by itself): "small_cmd" 0 - workgroup 0 relays the resident kernels'
 *   commands (platforms without a CPU-writable BAR); "debug_tag" - jump next to the 16-bit pass tag's wrap-around; "debug_stall_us" -
 *   be late with one command; "debug_p2p_one_row" - send this rank's total as one mailbox row, as launches of more than 32 groups
 *   do; "small_trace" - in-kernel time stamps (tools/trace_small.py). */
int kicp_reg_set_option(kicp_reg *reg, const char *name, double value);
double kicp_reg_get_option(const kicp_reg *reg, const char *name);

/* ComputeRobotMotion(frame, voxel_map, last_robot_pose, relative_wheel_odometry, max_correspondence_distance)
 * -- Registration.hpp:39-43 / Registration.cpp:151-190.  `frame_xyz` is a HOST pointer (uploaded inside). */
int kicp_register(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double last_pose_qt[7],
                  const double rel_odom_qt[7], double max_correspondence_distance, double out_pose_qt[7], kicp_stats *stats);
/* Same with the frame still float32 - the wire format of a PointCloud2, which the reference widens on the host with
 * static_cast<double> before it registers anything (ros/src/kinematic_icp_ros/utils/RosUtils.cpp:30-39): half the bytes cross
 * PCIe and the widening (exact) happens on the device, so the result is bit-equal to kicp_register on the widened frame. */
int kicp_register_f32(kicp_reg *reg, kicp_map *map, const float *frame_xyz_f32, size_t n, const double last_pose_qt[7],
                      const double rel_odom_qt[7], double max_correspondence_distance, double out_pose_qt[7], kicp_stats *stats);
/* Same, but the frame is already in HBM: `d_frame_xyz` is a DEVICE pointer on the handle's device
 * (e.g. the output of an on-device pre-step, or a torch tensor's data_ptr()). */
int kicp_register_device(kicp_reg *reg, kicp_map *map, const double *d_frame_xyz, size_t n, const double last_pose_qt[7],
                         const double rel_odom_qt[7], double max_correspondence_distance, double out_pose_qt[7],
                         kicp_stats *stats);
/* A queue of INDEPENDENT registrations against one map (several robots on one map, replayed scans), without a language
 * binding's per-call cost in between.  Every pose is bit-equal to what kicp_register_device returns for that scan alone; the
 * scans share nothing but the read-only map, which must not be updated during the call.  Because the scans do not depend on each
 * other, the call keeps SEVERAL OF THEM IN FLIGHT (one host thread - the caller's - drives them all, except in the first case):
 *   - batches of at least 32 scans that leave most of the device empty (all of at most 4 096 points, or all generic of at most 24 576):
 *     "batch_threads" (default 8) resident kernels side by side - as many as fit the device at once -, each with a contiguous part of
 *     the batch, "batch_depth" scans of it in flight, and a host thread of the library's pool;
 *   - otherwise, batches of at least two scans per queue that hold at least one scan for the generic pass kernel (more than 4 096 points by
 *     default): option "batch_queues" (default 8) scans at a time, "batch_group" (default 4) per launch, on handles + HSA queues of their own (clones of `reg`,
 *     created on first use and kept until kicp_reg_destroy(reg); they follow reg's configuration and kernel-shape options at every
 *     call), every pass an ordinary launch (large scans: the four-waves-per-SIMD build; small scans in such a batch: their own
 *     kernels, one launch per pass); the thread goes round the scans in flight: rows complete -> solve -> next pass or next scan;
 *   - otherwise, batches of eight scans and more of one kind (all small, or all up to 131 072 points): ONE kernel resident across
 *     the batch's scans ("batch_resident"), option "batch_depth" (default 3, at most 4) scans in flight - the command that starts a
 *     pass names the scan it belongs to, and the command of pass k + depth goes out when the rows of pass k are in;
 *   - anything else, and "batch_queues" 0 with "batch_threads" 0 and "batch_depth" 1, or "batch_resident" 0: the scans strictly one after the other
 *     (every scan runs launch -> hand-off -> solve to completion before the next one starts) - what a caller needs whose next
 *     scan depends on the previous result, and what kicp_register_device gives one call at a time.
 * SHARDED batches (round 5): with the shared segment attached (kicp_reg_shm_init) EVERY rank calls with the same count and the same
 * poses and hands over ITS shard of every scan (frame k of rank r = points [n_k r / R, n_k (r + 1) / R) of scan k; an empty shard
 * is legal: n[k] == 0).  "batch_queues" >= 2 then keeps that many SHARDED scans in flight per rank: lane j of the call registers scans
 * j, j + lanes, j + 2 lanes, ... on every rank and exchanges its per-pass totals through an area of its own in the segment, so the
 * lanes' exchanges interleave freely while every lane's sequence of exchanges is the same on every rank.  Poses and iteration counts
 * are bit-equal to the single-GPU batch on the whole scans, on every rank.  A sharded batch that fails half-way leaves the ranks'
 * lane counters in doubt: later sharded batches return KICP_ERR_COMM until kicp_reg_shm_destroy / _init have been redone on every
 * rank.  The same with the RCCL communicator attached (round 6): lane j issues its all-reduces on a sub-communicator of its own
 * (ncclCommSplit on first use) and on its own stream.  (Callback / peer-mailbox exchanges: the scans one after the other.)
 * Poses: count x 7 doubles.  `out_iterations` (nullable): ICP iterations each scan ran.  Returns the first error (< 0) - scans
 * after the first one that failed are then unspecified (some of them may have completed), nothing of the call is still running
 * on the device - otherwise the largest warning code seen (KICP_OK if none). */
int kicp_register_device_batch(kicp_reg *reg, kicp_map *map, size_t count, const double *const *d_frames_xyz, const size_t *n,
                               const double *last_poses_qt, const double *rel_odoms_qt, double max_correspondence_distance,
                               double *out_poses_qt, int *out_iterations);
/* The same queue of INDEPENDENT registrations with `lanes` of them in flight: lane t drives handle regs[t] (its own stream,
 * AQL queue and hand-off buffers; options and config are taken from each handle, except that for the duration of the call
 * small scans are not kept resident and large scans use the four-waves-per-SIMD kernel, which leaves room for the other
 * lanes' workgroups) from a host thread of its own (a pool the library starts on first use and keeps, unpinned - they do not
 * inherit the caller's CPU affinity; the calling thread sleeps until the lanes are done; one concurrent call at a time uses the
 * pool), scans are
 * dealt to the lanes first come, first served.  This is a THROUGHPUT mode for workloads that have independent scans -
 * several robots localising in one map, replayed logs - and nothing the reference's sequential pipeline can use: a scan's
 * initial guess there is the previous scan's result.  Every pose is bit-equal to what kicp_register_device returns for that
 * scan (the lanes share nothing but the read-only map).  The map must not be updated during the call.  Returns like
 * kicp_register_device_batch; after an error the remaining scans are not started and their poses are unspecified. */
int kicp_register_device_concurrent(kicp_reg *const *regs, size_t lanes, kicp_map *map, size_t count, const double *const *d_frames_xyz,
                                    const size_t *n, const double *last_poses_qt, const double *rel_odoms_qt,
                                    double max_correspondence_distance, double *out_poses_qt, int *out_iterations);
/* One fused association+accumulation pass at a fixed pose (DataAssociation + the reduction of
 * ComputePerturbation + the sum of ComputeOdometryRegularization; Registration.cpp:62-81,102-118,51-55).
 * out_sums = {JTJ00, JTJ01, JTJ11, JTr0, JTr1, sum||r||^2, N_corr}, un-normalised.  Host frame pointer. */
int kicp_pass_sums(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double pose_qt[7],
                   double max_correspondence_distance, double out_sums[7]);

/* The correspondences of that pass themselves - what DataAssociation appends (Registration.cpp:73-77) -, one entry per source point,
 * written by the SAME pass kernel build the handle registers a scan of this size with (its EXPORT instantiation: the search, the exact
 * resolution, the tie rule and the acceptance test are the shipped code, with the decision also stored per query):
 *   out_index[i]   index of the chosen map point in the device pool (bucket * max_points_per_voxel + position), -1: no correspondence
 *                  (nothing within max_correspondence_distance)
 *   out_d2[i]      its squared distance to pose * frame[i] (fp64, the reference's operation order); DBL_MAX without a correspondence
 *   out_nn_xyz     its coordinates (3 doubles per point; zeros without a correspondence)
 * Kernel-shape options ("small", "small_wave", "lanes_per_query", "latency_kernel") steer it as they steer kicp_register. */
int kicp_pass_correspondences(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double pose_qt[7],
                              double max_correspondence_distance, int32_t *out_index, double *out_d2, double *out_nn_xyz);

/* Same pass, but returns the raw all-reduce payload: KICP_REDUCE_WORDS int64 words = 3 limbs per sum (value * 2^40 =
 * l0 + l1*2^40 + l2*2^80) + range flag + padding.  Summing the words of disjoint shards element-wise gives exactly the
 * words' value of the union: this is what the multi-GPU mode all-reduces. */
int kicp_pass_words(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double pose_qt[7],
                    double max_correspondence_distance, long long out_words[24]);

/* DataAssociation (Registration.cpp:62-81) of ONE frame at `count` poses in one call: per pose the number of accepted correspondences and
 * the sum of their squared residuals |T s - nn|^2 - elements [6] and [5] of kicp_pass_sums at that pose, bit for bit (the same search,
 * exact resolution, tie rule and acceptance test; the same term, rounded once to 2^-40 and added as an integer, so the result does not
 * depend on how the work is cut into workgroups or launches).  What a registration pass computes beyond these two sums is not computed.
 * The poses (count x 7 doubles, HOST memory) are uploaded once; one launch serves many poses, and no launch serves more than option
 * "score_chunk" queries (pose x point pairs; default 8 388 608, about a millisecond of the device; rounded down to whole tiles of 256
 * source points, at least one) - "score_launches" (read only) tells how many the last call used.  An empty map, n == 0 or count == 0
 * give zeros and KICP_OK; a pose without any correspondence is a result, not a warning; a NaN pose gives what kicp_pass_sums gives
 * (zeros).  A pending kicp_map_update_pose_device_begin is collected first and its error returned.  count > 2^24 or
 * n > 0x7FFFFFF0 / 3: KICP_ERR_CAPACITY.  With a multi-GPU exchange attached: KICP_ERR_ARG (poses are scored per device).
 * kicp_score_poses takes a HOST frame (uploaded inside), kicp_score_poses_device a DEVICE pointer on the handle's device. */
int kicp_score_poses(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *poses_qt /* count x 7 */, size_t count,
                     double max_correspondence_distance, double *out_n_corr, double *out_ssr);
int kicp_score_poses_device(kicp_reg *reg, kicp_map *map, const double *d_frame_xyz, size_t n, const double *poses_qt, size_t count,
                            double max_correspondence_distance, double *out_n_corr, double *out_ssr);
/* Global localisation of one frame in a map that is not updated: score `count` candidate poses, refine the best few, score again.
 * Cost of a pose, lower is better (truncated least squares: a point without a correspondence costs tau^2):
 *     cost = (ssr + ((double)n - n_corr) * (tau * tau)) / (double)n        with tau = max_correspondence_distance
 * (ranking by the number of correspondences is no use on a dense map: the count saturates at many poses).
 *   1. every candidate is scored (kicp_score_poses_device; the frame is uploaded once);
 *   2. the min(top_m, count) cheapest are taken, ties to the lower index;
 *   3. they are refined as independent registrations of the frame (kicp_register_device_batch: last pose = candidate, odometry =
 *      identity, the handle's own configuration and options);
 *   4. the refined poses are scored by one more call;
 *   5. out_pose_qt = the cheapest refined pose (ties to the earlier rank), *out_candidate = the index of the candidate it started
 *      from, *out_cost_before / *out_cost_after = that candidate's cost and the refined pose's (the last three may be null).
 * A refinement that ends without correspondences (NaN pose) is out of the running; if all are - or the frame or the map is empty -
 * the call returns KICP_WARN_NO_CORRESPONDENCES with the cheapest UNREFINED candidate, both costs its own.
 * The refinement moves along the kinematic model only - a forward arc and a yaw (Registration.cpp:159-167) -, so it cannot remove a
 * candidate's lateral offset: with THIS call the candidates' lateral spacing is the caller's accuracy (kicp_relocalize_planar below
 * refines in the plane instead).  count == 0 or top_m == 0: KICP_ERR_ARG. */
int kicp_relocalize(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *candidates_qt, size_t count,
                    double max_correspondence_distance, size_t top_m, double out_pose_qt[7], size_t *out_candidate, double *out_cost_before,
                    double *out_cost_after);

/* The sums of ONE Gauss-Newton step that is free in the plane of the body frame (x, y, yaw), of ONE frame at `count` poses in one call.
 * Per accepted correspondence (s = source point, r = T s - nn, c0 = R UnitX, c1 = R UnitY) J = [c0 | c1 | R (-s.y, s.x, 0)]; per pose
 * eight doubles, in this order:
 *     N      number of accepted correspondences          S_a   sum a,  a = c0 . r
 *     S_x    sum s.x                                     S_b   sum b,  b = c1 . r
 *     S_y    sum s.y                                     S_c   sum (s.x b - s.y a)
 *     S_ss   sum (s.x^2 + s.y^2)                         ssr   sum |r|^2
 * N, -S_y, S_ss, S_a, S_c and ssr are elements [6], [1], [2], [3], [4] and [5] of kicp_pass_sums at that pose, bit for bit (the pass
 * kernels' own terms); S_x and S_b are formed next to them, each term rounded once to 2^-40 and added as an integer.  Everything
 * else - the poses in HOST memory, "score_chunk" / "score_launches", empty inputs (zeros, KICP_OK), a NaN pose (zeros), the pending
 * map update, the limits and the errors - is kicp_score_poses'. */
int kicp_planar_sums(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *poses_qt /* count x 7 */, size_t count,
                     double max_correspondence_distance, double *out_sums /* count x 8 */);
int kicp_planar_sums_device(kicp_reg *reg, kicp_map *map, const double *d_frame_xyz, size_t n, const double *poses_qt, size_t count,
                            double max_correspondence_distance, double *out_sums);
/* One such step on the host from one row of sums (no device, no handle): dx = -A^-1 g with A = [[N, 0, -S_y], [0, N, S_x],
 * [-S_y, S_x, S_ss]] and g = (S_a, S_b, S_c), then out_pose_qt = pose_qt * exp({dx, dy, 0, 0, 0, dtheta}).  No odometry prior, no
 * regularisation.  Returns 1 and writes out_pose_qt and out_dx (dx, dy, dtheta; may be null), or 0 with both untouched when the step
 * is degenerate: N < 1, a sum that is not finite, or N S_ss - S_x^2 - S_y^2 zero (all accepted points share one (x, y)) to within the
 * 2^-40 rounding the sums' terms carry, N 2^-41 (N + 2 |S_x| + 2 |S_y|) + 4 eps N S_ss.  Null sums / pose_qt / out_pose_qt:
 * KICP_ERR_ARG. */
int kicp_planar_step(const double sums[8], const double pose_qt[7], double out_pose_qt[7], double out_dx[3]);
/* Planar refinement of `count` poses of ONE frame, all in lock step: iteration j takes the sums of every pose still active from one
 * kicp_planar_sums_device call (one launch, unless "score_chunk" cuts it), then steps each on the host.  Per pose, independently of
 * every other pose of the call (the sums are integers: a pose's result does not depend on which poses share its launch):
 *     status 0  the step just applied had sqrt(dx^2 + dy^2 + dtheta^2) < convergence
 *     status 1  max_iterations steps applied
 *     status 2  the step was degenerate (kicp_planar_step: no correspondence, one point, a NaN pose): the pose as it stood
 * out_poses_qt (count x 7), out_iterations (steps applied) and out_status (the last two may be null).  An empty map or n == 0: the
 * poses unchanged, status 2.  "score_launches" counts the launches of the whole call.  max_iterations < 1 or convergence < 0:
 * KICP_ERR_ARG; otherwise the limits and errors of kicp_score_poses.  The registration's max_num_iterations does not apply:
 * point-to-point steps in the plane need 20 to 80 iterations where the kinematic model needs a handful. */
int kicp_refine_poses_planar(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *poses_qt, size_t count,
                             double max_correspondence_distance, int max_iterations, double convergence, double *out_poses_qt, int *out_iterations,
                             int *out_status);
int kicp_refine_poses_planar_device(kicp_reg *reg, kicp_map *map, const double *d_frame_xyz, size_t n, const double *poses_qt, size_t count,
                                    double max_correspondence_distance, int max_iterations, double convergence, double *out_poses_qt,
                                    int *out_iterations, int *out_status);
/* kicp_relocalize with step 3 replaced: the finalists are refined by kicp_refine_poses_planar_device on the frame already uploaded,
 * and a refinement with status 2 is out of the running.  Cost, ranking, ties, outputs and the KICP_WARN_NO_CORRESPONDENCES fall-back
 * are kicp_relocalize's.  The step is free in the plane, so a candidate's lateral offset is removed too: the grid only has to put
 * one candidate into the basin of the truth. */
int kicp_relocalize_planar(kicp_reg *reg, kicp_map *map, const double *frame_xyz, size_t n, const double *candidates_qt, size_t count,
                           double max_correspondence_distance, size_t top_m, int max_iterations, double convergence, double out_pose_qt[7],
                           size_t *out_candidate, double *out_cost_before, double *out_cost_after);

/* Candidate poses for kicp_relocalize: center * planar(dx, dy, dyaw) for every offset i * step with |i * step| <= half extent, per axis
 * (a step <= 0 or a half extent of 0 leaves that axis at the centre) - offsets in the centre's BODY frame, x slowest, yaw fastest.
 * Returns the number of poses of the grid and writes the first min(that, cap_poses) of them (out_poses_qt may be null: count only). */
size_t kicp_planar_grid(const double center_qt[7], double half_x, double half_y, double half_yaw, double step_x, double step_y, double step_yaw,
                        double *out_poses_qt, size_t cap_poses);

/* ---- whole-map relocalisation: an occupancy pyramid of the map and a branch-and-bound search over it ----
 * A kicp_occ is a SNAPSHOT of a map as bits: one bit per cell of a world-aligned grid, set where a map point lies within `dilate` cells
 * (Chebyshev) of it.  It owns its device memory and does NOT follow later updates of the map - the use case is the frozen map
 * (build it again after the map changed).  Geometry, per axis, all in fp64 without contraction:
 *     min  = (floor(lowest map coordinate / cell) - (dilate + 1)) * cell
 *     dims = floor((highest map coordinate - min) / cell) + dilate + 2
 *     cell index of a coordinate p: floor((p - min) / cell)
 * (an empty map: min = 0, dims = 1, no bit set).  Level 0 is that grid.  Level h (1 .. levels) has the SAME resolution and is a sliding
 * OR over x and y: occ_h(x, y, z) = OR of occ_0(x + a, y + b, z) over 0 <= a, b < 2^h, cells beyond the grid empty - so occ_h at a cell
 * bounds occ_0 at every cell of the 2^h x 2^h block that starts there, which is what the search rests on.
 * Layout of a level (what kicp_occ_level downloads): 32-bit words, cell (x, y, z) is bit (x & 31) - bit 0 the least significant - of
 * word (z * dims[1] + y) * words_x + (x >> 5), words_x = (dims[0] + 31) / 32; the bits of a row's last word beyond dims[0] are zero.
 * The build reads the map's HBM mirror (made current first; a pending deferred update is collected and its error returned), so a map
 * whose newest state lives on the device needs no host round trip.  cell <= 0 or not finite, dilate outside 0 .. 4, levels outside
 * 0 .. 10: KICP_ERR_ARG.  A pyramid (all levels) of more than 1 GiB, or an axis of 2^24 cells or more: KICP_ERR_CAPACITY, the message
 * names the size. */
typedef struct kicp_occ kicp_occ;
int kicp_occ_build(kicp_map *map, int device, double cell, int dilate, int levels, kicp_occ **out);
void kicp_occ_destroy(kicp_occ *occ);
/* any output may be null; out_set_cells: the number of set bits of level 0 */
int kicp_occ_info(const kicp_occ *occ, double out_min[3], int out_dims[3], double *out_cell, int *out_dilate, int *out_levels,
                  unsigned long long *out_set_cells);
/* one level as words (layout above): writes min(cap_words, total) words, *out_total_words = total (out_words may be null with cap 0) */
int kicp_occ_level(const kicp_occ *occ, int level, unsigned int *out_words, size_t cap_words, size_t *out_total_words);

/* The discretised pose space of a search.  Node (j, ix, iy) is the planar pose with translation (x0 + ix * cell, y0 + iy * cell, z) and
 * rotation yaw0 + j * yaw_step about z (roll = pitch = 0); its index is (j * ny + iy) * nx + ix.  nx, ny <= 2^20, nyaw <= 2^16. */
typedef struct kicp_search_window {
    double x0, y0, z;        /* world position of node (ix = 0, iy = 0); z: the base frame's height */
    unsigned int nx, ny;     /* nodes per axis, ONE CELL of the pyramid apart */
    double yaw0, yaw_step;   /* yaw of j = 0, spacing */
    unsigned int nyaw;
} kicp_search_window;
/* The rotation table the scores are computed from: out_cs[2 j] = std::cos(yaw0 + (double)j * yaw_step), out_cs[2 j + 1] = std::sin of
 * the same angle, on the host; the device uses these doubles and no trigonometry of its own. */
int kicp_search_yaws(const kicp_search_window *w, double *out_cs /* nyaw x 2 */);
/* A window around center_xy: nodes at center + i * cell for |i * cell| <= half extent per axis (the extent rounded down to whole
 * cells), the full circle of yaws from -pi in steps of 2 pi / ceil(2 pi / yaw_step) (yaw_step <= 0: one yaw, 0).  A half extent <= 0
 * (center_xy may then be null): that axis covers the pyramid's whole footprint, nodes on the cell corners min + i * cell. */
int kicp_search_window_around(const kicp_occ *occ, const double center_xy[2], double half_x, double half_y, double z, double yaw_step,
                              kicp_search_window *out);
/* Scores of nodes at one level of the pyramid.  Because the nodes are one cell apart, the cell of frame point p is computed once per
 * yaw j, with (c, s) of kicp_search_yaws, each operation rounded on its own in this order:
 *     cx = floor((((c * p.x - s * p.y) + x0) - min[0]) / cell)
 *     cy = floor((((s * p.x + c * p.y) + y0) - min[1]) / cell)
 *     cz = floor(((p.z + z) - min[2]) / cell)
 * and the score of node (j, ix, iy) at level h is the number of frame points with occ_h set at (cx + ix, cy + iy, cz); a cell outside
 * the grid - or not finite - counts as empty, with one exception that keeps the bound below valid: at level h > 0 an x (or y) in
 * -2^h < x < 0 is read as 0 (the block that starts there reaches into the grid, and the block that starts at the edge covers all of
 * that).  Scores are integers and exact.  At level h the score of (j, ix, iy) is an upper bound of the level-0 score of every node
 * (j, ix + a, iy + b), 0 <= a, b < 2^h.
 * `nodes`: count node indices (any order, repeats allowed), out_hits: count scores.  n == 0: zeros.  level outside 0 .. levels, an index
 * beyond the window, a null argument, a handle on another device than the pyramid's, or a multi-GPU exchange attached: KICP_ERR_ARG. */
int kicp_occ_score_nodes(kicp_reg *reg, const kicp_occ *occ, const double *frame_xyz, size_t n, const kicp_search_window *w, int level,
                         const unsigned long long *nodes, size_t count, unsigned int *out_hits);
/* The best nodes of the whole window: the first min(top_m, nx * ny * nyaw) of ALL its nodes sorted by (level-0 score descending, node
 * index ascending) - exactly what scoring every node and a stable sort give - found by branch and bound: the window is tiled with
 * blocks of 2^levels cells scored at the top level, a greedy dive of the best blocks yields a lower limit L (the top_m-th best leaf it
 * meets), and level by level the four children of every block whose bound is >= L are scored in one go.  out_nodes / out_hits
 * (top entries each), out_poses_qt (top x 7, nullable): the nodes' poses; *out_found = the number of entries written.
 * Option "search_max_nodes" (default 2^26) limits the nodes a call may score: beyond it the call returns KICP_ERR_CAPACITY, never an
 * inexact result.  "search_nodes_scored" and "search_launches" (read only) describe the last call (of
 * kicp_occ_score_nodes too: its `count` and its launches).  top_m == 0: KICP_ERR_ARG; the
 * other errors are those of kicp_occ_score_nodes; an empty frame gives zero scores (the first nodes by index). */
int kicp_search_poses(kicp_reg *reg, const kicp_occ *occ, const double *frame_xyz, size_t n, const kicp_search_window *w, size_t top_m,
                      unsigned long long *out_nodes, unsigned int *out_hits, double *out_poses_qt, size_t *out_found);
/* Relocalisation without a candidate grid of the caller's: kicp_search_poses, then kicp_relocalize_planar with the found poses as the
 * candidates and every one of them a finalist.  The score only selects the finalists; cost, ranking, ties, the refinement and the
 * KICP_WARN_NO_CORRESPONDENCES fall-back are those of kicp_relocalize_planar on `map` (the map the pyramid was built from).
 * *out_node (nullable): the node the returned pose started from. */
int kicp_relocalize_search(kicp_reg *reg, kicp_map *map, const kicp_occ *occ, const double *frame_xyz, size_t n, const kicp_search_window *w,
                           double max_correspondence_distance, size_t top_m, int max_iterations, double convergence, double out_pose_qt[7],
                           unsigned long long *out_node, double *out_cost_before, double *out_cost_after);

/* ---- a 2-D occupancy grid drawn while mapping: hits, and the free space the rays carve (kicp_grid.hip) ----------------------------
 * What a planner reads (nav_msgs/OccupancyGrid, map.pgm + map.yaml) cannot be made from the saved point map afterwards: telling free
 * from unknown needs the ray from the sensor to every return, and the rays exist only while the frames are being registered.
 *
 * The grid is world aligned: width x height cells of side `cell`, lower corner at (origin_x, origin_y), cell (ix, iy) is element
 * iy * width + ix.  Each cell holds two 16-bit counters, hits and misses; both saturate at 65 535.  Everything below is exact and
 * integer from the floor on.
 *
 * A frame is n points in the base frame, the pose and the sensor's origin in the base frame.  A point is USED when its three coordinates
 * are finite, z_min <= p.z < z_max holds for its base-frame z (the band needs no transform), its world coordinates are finite and its
 * endpoint cell passes the reach test.  With R, t of the pose (the registration's pose_to_rt, evaluated on the host):
 *   wx = ((r00 p.x + r01 p.y) + r02 p.z) + t0,  wy likewise with row 1 (every operation rounded on its own),
 *   cx = floor((wx - origin_x) / cell),  cy = floor((wy - origin_y) / cell);
 * the sensor's origin goes through the same arithmetic to the sensor cell (sx, sy).  reach = ceil(max_ray / cell) cells, computed at
 * creation: a point with max(|cx - sx|, |cy - sy|) > reach is skipped - no hit, no ray - so one frame touches at most the
 * (2 reach + 1)^2 cells around the sensor cell.
 * The ray of an endpoint cell (ex, ey), a = |ex - sx|, b = |ey - sy|, m = max(a, b), visits for k = 0 .. m - 1 the cell
 *   (sx + sgn(ex - sx) ((2 k a + m) / (2 m)),  sy + sgn(ey - sy) ((2 k b + m) / (2 m)))      (integer divisions)
 * - the sensor cell first, never the endpoint cell; m = 0 visits nothing.
 * Once per cell per frame: a cell inside the grid is HIT when it is the endpoint cell of at least one used point, otherwise MISS when
 * at least one used point's ray visits it, otherwise untouched; HIT cells get hits = min(hits + 1, 65535), MISS cells get misses =
 * min(misses + 1, 65535).  Cells outside the grid are ignored, but a ray whose endpoint or sensor cell lies outside still marks the
 * cells inside that it visits.  The result depends on the SET of endpoint cells only, not on the points' number or order.
 *
 * Limits: width * height <= 2^28 and reach <= 4095 (KICP_ERR_CAPACITY, the size in the message); cell and max_ray positive and finite,
 * the origin finite, z_min < z_max, width and height >= 1, no null pointer (KICP_ERR_ARG). */
typedef struct kicp_grid kicp_grid;
typedef struct kicp_grid_config {
    double cell, origin_x, origin_y; /* metres */
    unsigned int width, height;      /* cells */
    double z_min, z_max;             /* the band of base-frame heights whose points count: z_min <= p.z < z_max */
    double max_ray;                  /* metres: returns whose cell is farther than ceil(max_ray / cell) cells from the sensor's are skipped */
} kicp_grid_config;
int kicp_grid_create(const kicp_grid_config *config, int device, kicp_grid **out);
void kicp_grid_destroy(kicp_grid *grid);
/* the configuration, reach, and the frames integrated since creation or the last kicp_grid_clear (each nullable) */
int kicp_grid_info(const kicp_grid *grid, kicp_grid_config *out_config, int *out_reach, unsigned long long *out_frames);
int kicp_grid_clear(kicp_grid *grid); /* every counter and the frame count back to zero */
/* One frame.  kicp_grid_integrate takes the points from host memory (through the handle's pinned staging buffer);
 * kicp_grid_integrate_device takes them where they already are in HBM, complete - e.g. kicp_pre_device_ptr(pre, 0, ..) after
 * kicp_pre_frame has returned - and is what the drop-in pipeline calls.  Both return after their kernels have completed.
 * out_stats (nullable): points used, points skipped, cells HIT, cells MISS of this frame.  n == 0 is legal: nothing changes, the frame
 * is counted.  n > 0x7FFFFFF0 / 3: KICP_ERR_CAPACITY. */
int kicp_grid_integrate(kicp_grid *grid, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                        unsigned long long out_stats[4]);
int kicp_grid_integrate_device(kicp_grid *grid, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                               unsigned long long out_stats[4]);
/* The counters, cells x 2: hits then misses of cell 0, of cell 1, ...  cap_cells / cells must be the grid's width * height
 * (KICP_ERR_ARG otherwise).  kicp_grid_set_counts replaces them all: it resumes a mapping run from saved counters (the frame count is
 * not part of them). */
int kicp_grid_counts(const kicp_grid *grid, unsigned short *out, size_t cap_cells);
int kicp_grid_set_counts(kicp_grid *grid, const unsigned short *in, size_t cells);
/* The readout, the `data` of a nav_msgs/OccupancyGrid: width * height bytes, row-major from the origin,
 *   -1 where hits + misses < min_observations (min_observations >= 1, KICP_ERR_ARG otherwise),
 *   (100 hits + (hits + misses) / 2) / (hits + misses) otherwise, in integers: 0 .. 100.
 * kicp_grid_occupancy computes it on the GPU, so one byte per cell crosses PCIe; kicp_grid_occupancy_from_counts is the same arithmetic
 * as pure host code over counters in the layout of kicp_grid_counts and needs no GPU. */
int kicp_grid_occupancy(const kicp_grid *grid, unsigned int min_observations, signed char *out, size_t cap_cells);
int kicp_grid_occupancy_from_counts(const unsigned short *counts, size_t cells, unsigned int min_observations, signed char *out);
/* The grid as the <prefix>.pgm + <prefix>.yaml pair map_server and Nav2 read.  The PGM: "P5\n<width> <height>\n255\n", then the rows
 * from the highest iy down to 0; a pixel is 0 when (double)value > occupied_thresh * 100.0, 254 when value >= 0 and (double)value <
 * free_thresh * 100.0, 205 otherwise (unknown cells too).  The YAML: image (the PGM's base name), mode: trinary, resolution, origin
 * [x, y, 0], negate: 0, occupied_thresh, free_thresh, the numbers as %.17g.  map_server's defaults are occupied_thresh 0.65 and
 * free_thresh 0.25; 0 <= free_thresh < occupied_thresh <= 1, KICP_ERR_ARG otherwise, and KICP_ERR_ARG with the system's reason when
 * a file cannot be written (as kicp_map_save_pcd).  kicp_grid_write_map is pure host code and needs no GPU; kicp_grid_save_map is the
 * readout followed by it. */
int kicp_grid_save_map(const kicp_grid *grid, const char *prefix, unsigned int min_observations, double occupied_thresh, double free_thresh);
int kicp_grid_write_map(const char *prefix, const signed char *occupancy, unsigned int width, unsigned int height, double cell, double origin_x,
                        double origin_y, double occupied_thresh, double free_thresh);
/* THE FILL: the unknown cells of one grid from the readout of another - what puts the free space this grid's rays carve under a grid of
 * classes that kicp_elev_to_grid* wrote (uneven ground, below), as a step of its own between two grids.  With the fill configuration
 * min_observations >= 1, free_max <= 100 and free_max < occupied_min <= 101 (KICP_ERR_ARG otherwise; occupied_min = 101 never takes
 * the source's obstacles), a SOURCE cell with counters (hits, misses) reads v = the readout above at min_observations; it is FREE when
 * 0 <= v <= free_max, OCCUPIED when v >= occupied_min, and otherwise says nothing.  A DESTINATION cell is unknown when both its
 * counters are 0, an obstacle when hits > 0, otherwise traversable.  The fill changes only unknown destination cells: to (hits 0,
 * misses 1) where the source is FREE, to (1, 0) where it is OCCUPIED; every other counter keeps its bits, so the destination always
 * wins where it knows something.  out_counts (nullable) is seven words (KICP_GRID_FILL_COUNTS): kept obstacle, kept traversable,
 * filled free, filled occupied, left unknown - these five sum to the cell count - and two disagreements, as diagnostics: traversable
 * over a source OCCUPIED, and obstacle over a source FREE.  A second call leaves the counters as the first left them and counts the
 * filled cells as kept.
 * kicp_grid_fill_unknown: dst != src, their cell, origin_x, origin_y, width and height bit-equal, both on the same device (KICP_ERR_ARG
 * otherwise, and nothing is written).  src is not changed.  For dst the counters change as under kicp_grid_set_counts - the frame
 * count and the last window stay -, and BESIDE THAT THE PLAN IS INVALIDATED (kicp_grid_has_plan reads 0): the fill is the last step
 * of the chain that prepares the counters a new plan is made on, and a plan of the unfilled grid must not be scored by accident.  The
 * call returns after its kernel has completed.  kicp_grid_fill_unknown_counts is the same arithmetic as pure host code over counters
 * in kicp_grid_counts' layout (dst_counts != src_counts; null pointers only with cells == 0) and needs no GPU. */
typedef struct kicp_grid_fill_config {
    unsigned int min_observations; /* >= 1: the source's readout */
    unsigned int free_max;         /* 0 .. 100: a source value of 0 .. free_max is FREE */
    unsigned int occupied_min;     /* free_max < occupied_min <= 101: a source value of occupied_min or more is OCCUPIED */
} kicp_grid_fill_config;
#define KICP_GRID_FILL_COUNTS 7
int kicp_grid_fill_unknown(kicp_grid *dst, const kicp_grid *src, const kicp_grid_fill_config *config, unsigned long long out_counts[7]);
int kicp_grid_fill_unknown_counts(unsigned short *dst_counts, const unsigned short *src_counts, size_t cells, const kicp_grid_fill_config *config,
                                  unsigned long long out_counts[7]);

/* ---- what a planner plans on: the clearance of every cell and a Nav2-style costmap of the grid (kicp_grid_plan.hip) --------------------
 * Everything below is exact and integer: squared cell distances, and a lookup table for the cost.
 *
 * CLASSES.  With v the readout of a cell at `min_observations` (above), a cell is a SOURCE when (double)v > occupied_thresh * 100.0 -
 * exactly the cells whose pixel in the map image is 0 - UNKNOWN when v < 0, and CLEAR otherwise.  With unknown_is_obstacle != 0 the
 * unknown cells are sources too.  Cells outside the grid are nothing: neither sources nor anything else.
 *
 * CLEARANCE.  With a radius of R = radius_cells, 1 <= R <= 254, the clearance of cell (x, y) is
 *   c(x, y) = min of dx^2 + dy^2 over the sources at (x + dx, y + dy) with dx^2 + dy^2 <= R^2,   R^2 + 1 ("far") when there is none
 * - a squared distance in cells, 0 on a source, as 16 bits: R <= 254 keeps a column distance inside a byte and R^2 + 1 = 64 517 inside
 * 16 bits.  R < 1: KICP_ERR_ARG; R > 254: KICP_ERR_CAPACITY, the limit in the message.
 *
 * RECTANGLE.  Every entry takes x0, y0, w, h: a rectangle of grid cells, inside the grid, w and h >= 1 (KICP_ERR_ARG otherwise), and
 * writes h * w values, row-major from (x0, y0); cap must be w * h (KICP_ERR_ARG otherwise).  Sources within R of the rectangle count
 * whether they lie inside it or not, so the result for a rectangle EQUALS the result for the full grid - the rectangle (0, 0, width,
 * height) - restricted to it.  As the transform is local, a frame can change the result only within R cells of its window:
 * kicp_grid_last_window gives the window of the last integrated frame clipped to the grid, w = h = 0 (and x0 = y0 = 0) when no cell of
 * it lies inside the grid, before any frame and after kicp_grid_clear.  That rectangle grown by R and clipped is all a node has to
 * refresh after a frame.
 *
 * COSTMAP.  One byte per cell with nav2_costmap_2d's constants: 254 lethal, 253 inscribed, 255 no information, 0 free.  The caller
 * passes table[0 .. R^2 + 1], the cost of every clearance (table_len must be R^2 + 2, KICP_ERR_ARG otherwise); t = table[c(x, y)].
 * The cell's base cost is 254 for a source, 255 for an unknown cell that is not a source, 0 for a clear cell.  For a base of 255 the
 * result is t when (inflate_unknown ? t > 0 : t >= 253) and 255 otherwise; for any other base it is max(base, t) - the rule of Nav2's
 * inflation layer over a master grid that holds the base costs.
 * kicp_grid_cost_table_nav2 fills the table Nav2's inflation layer uses (pure host code; cap must be R^2 + 2): table[0] = 254,
 * table[R^2 + 1] = 0, and for 1 <= d2 <= R^2 with d = sqrt((double)d2) * cell: 253 when d <= inscribed_radius, otherwise
 * (unsigned char)(252.0 * exp(-cost_scaling_factor * (d - inscribed_radius))).  cell positive and finite, inscribed_radius and
 * cost_scaling_factor finite and >= 0 (KICP_ERR_ARG otherwise).
 *
 * kicp_grid_clearance and kicp_grid_costmap work on the counters where they are, in HBM, and return after their kernels have completed
 * and the h * w values have arrived; the *_from_occupancy entries are the same arithmetic as pure host code over a readout (width x
 * height values as kicp_grid_occupancy writes them) and need no GPU.  For every entry: a null pointer, min_observations < 1 or an
 * occupied_thresh outside [0, 1] is KICP_ERR_ARG. */
typedef struct kicp_grid_clearance_config {
    unsigned int min_observations; /* of the readout the classes are taken from (the *_from_occupancy entries only check it) */
    double occupied_thresh;        /* a cell is a source when (double)v > occupied_thresh * 100.0 */
    int unknown_is_obstacle;       /* != 0: unknown cells are sources too */
    int radius_cells;              /* R: 1 .. 254 */
} kicp_grid_clearance_config;
int kicp_grid_clearance(const kicp_grid *grid, const kicp_grid_clearance_config *config, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h,
                        unsigned short *out, size_t cap);
int kicp_grid_costmap(const kicp_grid *grid, const kicp_grid_clearance_config *config, const unsigned char *table, size_t table_len, int inflate_unknown,
                      unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, unsigned char *out, size_t cap);
int kicp_grid_clearance_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_grid_clearance_config *config,
                                       unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, unsigned short *out, size_t cap);
int kicp_grid_costmap_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_grid_clearance_config *config,
                                     const unsigned char *table, size_t table_len, int inflate_unknown, unsigned int x0, unsigned int y0, unsigned int w,
                                     unsigned int h, unsigned char *out, size_t cap);
int kicp_grid_cost_table_nav2(double cell, int radius_cells, double inscribed_radius, double cost_scaling_factor, unsigned char *table, size_t cap);
int kicp_grid_last_window(const kicp_grid *grid, unsigned int *x0, unsigned int *y0, unsigned int *w, unsigned int *h);

/* ---- from the costmap to a path: the cost-to-go field a planner spreads from its goal, and the path down it (kicp_grid_plan.hip) --------
 * What Nav2's NavFn calls the potential.  Everything below is exact and integer; the field is the unique least fixed point of its
 * recurrence, so the host and the device entries return equal arrays.
 *
 * INPUTS.  A costmap of width x height bytes, cell (x, y) at y * width + x, as kicp_grid_costmap writes it (any byte array will do).
 * A weight table weight[256] of bytes: q(c) = weight[costmap[c]]; q = 0 means the cell is IMPASSABLE, otherwise 1 <= q <= 255.  A goal
 * list of n_goals >= 1 cells as (x, y) pairs, goals_xy[2 g] = x, goals_xy[2 g + 1] = y: a goal outside the grid is KICP_ERR_ARG, a
 * goal on an impassable cell is ignored (out_stats counts the others; a cell listed twice counts twice).  max_potential with
 * 1 <= max_potential <= 0xFFFFFFFE.
 *
 * EDGES.  A passable cell is joined to each of its eight neighbours that is passable.  There is NO corner rule: a diagonal step
 * between two passable cells is allowed whatever the two cells beside it are - the costmap's inflation is what keeps a path off
 * corners, so plan on an inflated costmap.  With s = q(u) + q(v) an orthogonal step weighs s and a diagonal step (181 * s + 64) >> 7
 * (181 / 128 = 1.4140625).  Edges are symmetric and weigh at least 2 (at most 721).
 *
 * POTENTIAL.  32 bits per cell.  A passable goal has potential 0; every other passable cell min(D, max_potential), where D is the least
 * sum of edge weights over the paths from it to a passable goal; cells without such a path, and impassable cells, read 0xFFFFFFFF.
 * The clamp is part of the definition, not an overflow escape: pot(c) = min over neighbours n of sat(pot(n) + edge(c, n)) with sat
 * saturating at max_potential is monotone, so its least fixed point is exactly min(D, max_potential).  The clamp doubles as a planning
 * horizon: beyond it the field is flat and yields no path.
 *
 * PATH.  From a potential array and a start cell: from the current cell take the FIRST neighbour n, in the order +x, -x, +y, -y,
 * (+x, +y), (-x, +y), (+x, -y), (-x, -y), that is passable (q(n) > 0 and its potential below 0xFFFFFFFF) and has
 * pot[cur] == pot[n] + edge(cur, n); stop at potential 0.  The costmap and the weights must be those the potential was made from:
 * they give `edge`.  The output is the cell list as (x, y) pairs of unsigned int, start and goal included; *out_n is its length.  A
 * start outside the grid, or one whose potential is 0xFFFFFFFF ("unreachable"), is KICP_ERR_ARG.  A walk that reaches a cell above 0
 * where no neighbour satisfies the equality - a start at or inside the zone max_potential clamped - is KICP_ERR_CAPACITY, max_potential
 * named in the message, *out_n = 0.  cap_cells too small is KICP_ERR_CAPACITY as well, with the needed length in *out_n (> cap_cells)
 * and the first cap_cells cells stored; out_xy may be NULL only with cap_cells == 0.  Every step lowers the potential by at least 2,
 * so the walk ends.
 *
 * WEIGHTS.  kicp_plan_weights fills the table NavFn's rule gives (pure host code): for b < lethal_from
 *   weight[b] = min(255, neutral + b * factor_num / factor_den)     (integers; the product in 64 bits)
 * for lethal_from <= b <= 254 it is 0, and weight[255] = unknown_weight - 0 keeps the planner out of unknown space.  Checked
 * (KICP_ERR_ARG): out not null, 1 <= neutral <= 255, factor_den >= 1, lethal_from <= 255, unknown_weight <= 255.  NavFn's own numbers
 * are neutral 50, factor 4 / 5 and lethal_from 253.
 *
 * ENTRIES.  kicp_potential_from_costmap (Dijkstra with 64-bit sums, clamped at the end) and kicp_potential_path are pure host code and
 * need no GPU.  kicp_grid_potential_of_costmap takes a costmap of the grid's width x height from host memory to the GPU;
 * kicp_grid_potential computes the full grid's costmap as kicp_grid_costmap does (same arguments, same bytes) and spreads the field
 * over it where it is: the costmap never leaves HBM.  Both return after their kernels have completed and the width * height values
 * have arrived.  cap must be width * height.  out_stats (nullable): goals used, cells with a potential below max_potential, cells equal
 * to max_potential, relaxation rounds - the last is 0 for the host entry and implementation-defined on the device (it depends on how
 * the work is tiled and batched; do not compare it).  Errors: a null pointer, width or height 0, cap != width * height, n_goals == 0
 * or max_potential out of range are KICP_ERR_ARG; width * height or n_goals above 2^28 is KICP_ERR_CAPACITY; kicp_grid_potential also
 * has the argument errors of kicp_grid_costmap.  The device entries bound their rounds by the number of cells plus one, which a
 * correct build cannot reach: KICP_ERR_INTERNAL. */
typedef struct kicp_plan_config {
    unsigned int max_potential; /* 1 .. 0xFFFFFFFE: potentials are clamped here */
} kicp_plan_config;
int kicp_plan_weights(unsigned int neutral, unsigned int factor_num, unsigned int factor_den, unsigned int lethal_from, unsigned int unknown_weight,
                      unsigned char out[256]);
int kicp_potential_from_costmap(const unsigned char *costmap, unsigned int width, unsigned int height, const unsigned char weight[256],
                                const kicp_plan_config *config, const unsigned int *goals_xy, size_t n_goals, unsigned int *out, size_t cap,
                                unsigned long long out_stats[4]);
int kicp_potential_path(const unsigned int *potential, const unsigned char *costmap, unsigned int width, unsigned int height, const unsigned char weight[256],
                        unsigned int start_x, unsigned int start_y, unsigned int *out_xy, size_t cap_cells, size_t *out_n);
int kicp_grid_potential_of_costmap(const kicp_grid *grid, const unsigned char *costmap, const unsigned char weight[256], const kicp_plan_config *config,
                                   const unsigned int *goals_xy, size_t n_goals, unsigned int *out, size_t cap, unsigned long long out_stats[4]);
int kicp_grid_potential(const kicp_grid *grid, const kicp_grid_clearance_config *clearance, const unsigned char *table, size_t table_len, int inflate_unknown,
                        const unsigned char weight[256], const kicp_plan_config *config, const unsigned int *goals_xy, size_t n_goals, unsigned int *out,
                        size_t cap, unsigned long long out_stats[4]);

/* ---- from the field to a command: a fan of arc trajectories scored on the costmap and the potential (kicp_grid_arcs.hip) -------------
 * What a local planner (DWA / DWB, MPPI) does each control cycle: roll candidate commands forward as arcs, lay the robot's footprint on
 * the costmap at every pose, drop the arcs that collide, rank the rest by how far down the cost-to-go field they end.  Everything below
 * is exact: the only floating-point operations are fp64 + - * / and floor, every operation rounded on its own (the library is built
 * with -ffp-contract=off), and no transcendental is evaluated inside a scoring entry.  The host and the device entry return equal arrays.
 *
 * PLAN.  A successful kicp_grid_potential or kicp_grid_potential_of_costmap leaves a plan in the handle: q = weight[costmap] per cell
 * (1 .. 255, 0 impassable) and the potential, for the grid's width x height, where they lie in HBM.  The plan stays valid until the next
 * call of either entry; a call of theirs that fails - on its arguments too - invalidates it.  Integrating frames does not: the plan is
 * a snapshot.  kicp_grid_clearance and kicp_grid_costmap do not write the plan's buffers and do not invalidate it.  Scoring on a handle
 * without a valid plan is KICP_ERR_ARG.
 *
 * START.  start[4] = x, y, c, s: the base frame's origin in world metres and its heading as a unit vector (cosine, sine; the caller
 * evaluates them).  All four must be finite (KICP_ERR_ARG).
 *
 * ARCS.  arcs holds n_arcs x 4 doubles (dx, dy, dc, ds): ONE step of the arc, expressed in the robot's frame - the reference's motion
 * model, a displacement and a yaw.  The rollout of arc k starts with pose_0 = start; for t = 1 .. n_steps
 *   x_t = x_{t-1} + (c_{t-1} * dx - s_{t-1} * dy)        c_t = c_{t-1} * dc - s_{t-1} * ds
 *   y_t = y_{t-1} + (s_{t-1} * dx + c_{t-1} * dy)        s_t = s_{t-1} * dc + c_{t-1} * ds
 *
 * FOOTPRINT.  n_samples points (fx, fy) in the base frame, footprint_xy[2 p] = fx, footprint_xy[2 p + 1] = fy.  Sample p at pose t lies at
 *   wx = x_t + (c_t * fx - s_t * fy),   wy = y_t + (s_t * fx + c_t * fy)
 * in the cell cx = floor((wx - origin_x) / cell), cy = floor((wy - origin_y) / cell) - the grid's own arithmetic.  Its weight is
 * q(cx, cy) when 0 <= cx < width and 0 <= cy < height, and 0 when the cell is outside the grid or wx or wy is not finite.  Values that
 * are not finite inside arcs or footprint_xy are legal input: they collide.  Pose t COLLIDES when a sample's weight is 0; otherwise
 * its cost m_t is the largest of the samples' weights.  The start pose is not checked: the robot is where it is.
 *
 * RESULT.  Four unsigned int per arc, out[4 k .. 4 k + 3]:
 *   free_steps     the largest f <= n_steps such that the poses 1 .. f do not collide
 *   cost_sum       the sum of m_t over t = 1 .. f
 *   cost_max       the largest of those m_t, 0 when f = 0
 *   end_potential  the plan's potential at the cell of (x_f, y_f) - the base origin at the last free pose, the start when f = 0 -
 *                  and 0xFFFFFFFF when that cell is outside the grid (an impassable or unreached cell reads 0xFFFFFFFF as well)
 *
 * LIMITS.  1 <= n_arcs <= 2^20, 1 <= n_steps <= 1024, 1 <= n_samples <= 4096: above is KICP_ERR_CAPACITY with the limit in the message,
 * 0 or a null pointer KICP_ERR_ARG.  cap must be 4 * n_arcs (KICP_ERR_ARG).
 *
 * ENTRIES.  kicp_grid_score_arcs scores on the handle's plan where it lies in HBM - one launch, a wave per arc - and returns after the
 * n_arcs x 4 words have arrived.  kicp_score_arcs_from_plan is the same arithmetic as pure host code over the caller's arrays (q and
 * potential of width x height, cell (x, y) at y * width + x, with the grid's cell, origin_x, origin_y) and needs no GPU; cell not
 * positive or not finite, an origin that is not finite, width or height 0 are KICP_ERR_ARG, width * height above 2^28
 * KICP_ERR_CAPACITY.  kicp_plan_q makes its q from a costmap: out[c] = weight[costmap[c]] for `cells` cells (pure host code).
 *
 * kicp_arc_steps fills n_arcs x 4 doubles from commands (v, omega) held for dt with the reference's arc (pure host code; sin and cos are
 * the C library's sin() and cos(), each called on its own - not its sincos(), which differs from them in the last bit now and then): d = v[k] * dt, theta = omega[k] * dt,
 *   (dx, dy) = (d, 0)                                                       when |theta| < 1e-9
 *   dx = (d * sin(theta)) / theta,   dy = (d * (1 - cos(theta))) / theta    otherwise
 *   dc = cos(theta),   ds = sin(theta).
 * The branch stands where the reference adds an epsilon to theta, which divides by zero at theta = -epsilon.  n_arcs as above.
 *
 * kicp_footprint_box makes a lattice over a box that includes its boundary (pure host code): nx = ceil((x_max - x_min) / spacing) + 1
 * points x_i = x_min + ((x_max - x_min) * i) / (nx - 1) - x_min alone when nx = 1 - and y likewise; sample j * nx + i is (x_i, y_j).
 * *out_n is nx * ny; cap counts samples (out_xy has room for 2 * cap doubles).  A cap that is too small is KICP_ERR_CAPACITY with the needed count in *out_n (> cap) and the first cap samples
 * stored; out_xy may be NULL only with cap == 0.  A box that is not finite, x_min > x_max, y_min > y_max, spacing not positive or not
 * finite: KICP_ERR_ARG; nx * ny above 4096, a footprint's limit: KICP_ERR_CAPACITY with *out_n = 0.
 *
 * kicp_arcs_best ranks results as the scoring entries write them (pure host code - ranking n_arcs rows is microseconds, so there is no
 * device argmin).  Arc k is ADMISSIBLE when free_steps >= min_free_steps and end_potential != 0xFFFFFFFF.  Its score is
 *   w_potential * end_potential + w_cost * cost_sum + w_blocked * (n_steps - free_steps)
 * each product and the sum in unsigned 64 bits (the sum wraps; n_steps - free_steps counts as 0 when free_steps > n_steps).
 * *out_index is the admissible arc of least score, the lowest index on a tie, and n_arcs when none is admissible.  n_arcs as above. */
int kicp_plan_q(const unsigned char *costmap, size_t cells, const unsigned char weight[256], unsigned char *out);
int kicp_arc_steps(const double *v, const double *omega, double dt, size_t n_arcs, double *out /* n_arcs x 4 */);
int kicp_footprint_box(double x_min, double x_max, double y_min, double y_max, double spacing, double *out_xy, size_t cap, size_t *out_n);
int kicp_arcs_best(const unsigned int *results /* n_arcs x 4 */, size_t n_arcs, unsigned int w_potential, unsigned int w_cost, unsigned int w_blocked,
                   unsigned int n_steps, unsigned int min_free_steps, size_t *out_index);
int kicp_score_arcs_from_plan(const unsigned char *q, const unsigned int *potential, double cell, double origin_x, double origin_y, unsigned int width,
                              unsigned int height, const double start[4], const double *arcs, size_t n_arcs, unsigned int n_steps, const double *footprint_xy,
                              size_t n_samples, unsigned int *out, size_t cap);
int kicp_grid_has_plan(const kicp_grid *grid); /* 1 when the handle holds a valid plan, else 0 (a null handle too) */
int kicp_grid_score_arcs(const kicp_grid *grid, const double start[4], const double *arcs, size_t n_arcs, unsigned int n_steps, const double *footprint_xy,
                         size_t n_samples, unsigned int *out, size_t cap);

/* ---- commands that change along a trajectory: a tree of arc segments scored on the plan (kicp_grid_arc_tree.hip) ---------------------
 * An arc above repeats ONE step n_steps times, so a candidate's command never changes: a fan of arcs cannot turn and then go straight,
 * round a corner or swerve and return.  A tree of segments can: every path from the root is a sequence of primitives, each held for
 * its level's steps.  The B^D sequences of D segments share almost all of their prefixes, and the rollout below is exact and stated
 * operation by operation, so a prefix is rolled once and continued: every node gets the bits a rollout of its whole path from `start`
 * gives.  PLAN, START, FOOTPRINT, the recurrence and the collision rule are those of the section above.
 *
 * TREE.  depth = D, 1 <= D <= 8.  Level d = 1 .. D has branch[d - 1] = B_d >= 1 primitives and steps[d - 1] = L_d >= 1 steps.
 * primitives holds (B_1 + ... + B_D) x 4 doubles, level 1's rows first, then level 2's, and so on; each row is one step
 * (dx, dy, dc, ds), exactly an arc's row (kicp_arc_steps makes them).  Level d has n_d = B_1 * ... * B_d nodes; the tree has
 * N = n_1 + ... + n_D nodes and its paths T = L_1 + ... + L_D steps.
 *
 * NUMBERING.  Nodes are level-major: level d occupies the rows off_d .. off_d + n_d - 1, off_1 = 0, off_{d+1} = off_d + n_d.  Inside
 * a level, the child that takes primitive b under the parent with in-level index j has in-level index j * B_d + b; the path
 * (b_1 .. b_d) of a node follows from its in-level index by repeated division.
 *
 * RESULT.  Four unsigned int per node, out[4 r .. 4 r + 3] for row r, with the meaning they have for an arc.  They describe ONE
 * trajectory: from `start`, L_1 steps of level 1's primitive b_1, then L_2 steps of level 2's primitive b_2, and so on through the
 * node's level d.  Every pose is checked with the footprint, the rollout ends at the first colliding pose, free_steps counts along
 * the whole path (0 .. L_1 + ... + L_d), cost_sum and cost_max run over those free poses, end_potential is read at the last free pose.
 * A node whose parent ended early therefore has its parent's four words.  A tree with D = 1 gives word for word what
 * kicp_grid_score_arcs gives for arcs = primitives, n_steps = L_1.  Values that are not finite in primitives or footprint_xy are
 * legal and collide.
 *
 * LIMITS.  D <= 8, N <= 2^20, T <= 1024 (which keeps cost_sum's bound), n_samples <= 4096: above is KICP_ERR_CAPACITY with the limit in
 * the message.  D = 0, a zero in branch or steps, n_samples = 0, a start that is not finite or a null pointer: KICP_ERR_ARG.  cap must
 * be 4 * N (KICP_ERR_ARG).
 *
 * ENTRIES.  kicp_grid_score_arc_tree scores on the handle's plan where it lies in HBM - one launch per level, a wave per node, each
 * level continuing the records the level above left on the device - and returns after the N x 4 words have arrived; without a valid
 * plan it is KICP_ERR_ARG, as kicp_grid_score_arcs.  kicp_score_arc_tree_from_plan is the same arithmetic as pure host code over the
 * caller's arrays (q, potential, cell, origin_x, origin_y, width, height as kicp_score_arcs_from_plan takes them) and needs no GPU.
 *
 * kicp_arc_tree_nodes performs the checks on depth, branch and steps and returns the counts (pure host code): *out_n_nodes = N,
 * *out_n_leaves = n_D, *out_total_steps = T, and out_level_offset[d - 1] = off_d for the D levels when it is not NULL (the only
 * pointer that may be).  Callers size `out` with it.  On an error the three counts are 0.
 *
 * kicp_arc_tree_best ranks the LEAVES (level D) only, from the N x 4 results as the scoring entries write them (pure host code).
 * Admissibility and score are those of kicp_arcs_best with n_steps = T, ties go to the lowest in-level index.  *out_leaf is the
 * leaf's in-level index, or n_D when no leaf is admissible (0 on an error); out_path[e - 1] = b_e for e = 1 .. D is filled when a leaf
 * was found - out_path[0] is the command to execute now. */
int kicp_arc_tree_nodes(unsigned int depth, const unsigned int *branch, const unsigned int *steps, size_t *out_n_nodes, size_t *out_n_leaves,
                        unsigned int *out_total_steps, size_t *out_level_offset /* depth, nullable */);
int kicp_arc_tree_best(const unsigned int *results /* N x 4 */, unsigned int depth, const unsigned int *branch, const unsigned int *steps, unsigned int w_potential,
                       unsigned int w_cost, unsigned int w_blocked, unsigned int min_free_steps, size_t *out_leaf, unsigned int *out_path /* depth */);
int kicp_score_arc_tree_from_plan(const unsigned char *q, const unsigned int *potential, double cell, double origin_x, double origin_y, unsigned int width,
                                  unsigned int height, const double start[4], unsigned int depth, const unsigned int *branch, const unsigned int *steps,
                                  const double *primitives, const double *footprint_xy, size_t n_samples, unsigned int *out, size_t cap);
int kicp_grid_score_arc_tree(const kicp_grid *grid, const double start[4], unsigned int depth, const unsigned int *branch, const unsigned int *steps,
                             const double *primitives, const double *footprint_xy, size_t n_samples, unsigned int *out, size_t cap);

/* ---- where to go while mapping: the exploration frontiers of the grid, ranked by the plan (kicp_grid_explore.hip) ----------------------
 * A robot that is still mapping has no goal from outside: its goal is the edge of what it has seen.  These entries find the free cells
 * that border unknown space, group them into frontiers and sum ten words per frontier - what explore_lite or a Nav2 exploration node
 * does on a copy of the map.  Everything below is integer and the result is unique: the host and the device entry return equal arrays.
 *
 * CLASSES.  Those of the clearance section above, with unknown_is_obstacle = 0: with v the readout of a cell at `min_observations`, the
 * cell is OCCUPIED (a source) when (double)v > occupied_thresh * 100.0, UNKNOWN when v < 0, and CLEAR otherwise.  Cells outside the
 * grid are nothing: in particular they are not unknown.
 *
 * FRONTIER CELL.  A CLEAR cell is a frontier cell when at least one of its four edge neighbours inside the grid is UNKNOWN.
 *
 * FRONTIER.  Frontier cells are joined to each of their eight neighbours that is a frontier cell.  There is NO corner rule: two
 * frontier cells that touch at a corner are joined whatever the two cells beside them are.  A frontier is a connected component of
 * that graph.
 *
 * LABEL.  The label of a frontier is the least cell index y * width + x among its cells.  The label plane is width * height words of
 * unsigned int: a frontier cell holds its frontier's label, every other cell 0xFFFFFFFF.  width * height <= 2^28, so labels fit.
 *
 * ROW.  Per frontier KICP_FRONTIER_WORDS = 10 words of unsigned long long:
 *   0           the label
 *   1           the size in cells
 *   2, 3        the sum of x and the sum of y over its cells (the centroid is the caller's division: none enters the contract)
 *   4, 5, 6, 7  min x, max x, min y, max y
 *   8           best_potential: the least pot(c) over its cells
 *   9           best_cell: the least cell index among the cells that attain it
 * pot(c) is the potential of the PLAN the handle holds (the section above) when use_plan != 0 - for the host entry: potential[c] when
 * `potential` is not null - and 0xFFFFFFFF for every cell otherwise; then word 8 is 0xFFFFFFFF and word 9 equals the label.  Words 8
 * and 9 together are the minimum of the 64-bit key pot(c) * 2^32 + c.  With the robot's cell as the plan's one goal, word 8 is the cost
 * of driving to the frontier and word 9 the cell to drive to; a frontier that lies wholly in unreached space reads 0xFFFFFFFF.
 *
 * OUTPUT.  Frontiers with size < min_size are dropped (min_size >= 1; anything else is KICP_ERR_ARG); the others are written in
 * ascending label order.  The label plane is NOT filtered by min_size.
 *
 * CAPACITY.  *out_n is the number of frontiers that pass the filter.  When it exceeds cap_rows, the first cap_rows rows are stored and
 * the call returns KICP_ERR_CAPACITY with the needed number in *out_n - kicp_potential_path's convention.  out_rows may be NULL only
 * with cap_rows == 0.  out_labels is nullable: cap_labels must be width * height with a label plane and 0 without one.
 *
 * ENTRIES.  kicp_frontiers_from_occupancy is pure host code over a readout (width x height values as kicp_grid_occupancy writes them;
 * min_observations is only checked) and needs no GPU; width or height 0 is KICP_ERR_ARG, width * height above 2^28 KICP_ERR_CAPACITY.
 * kicp_grid_frontiers works on the counters where they are, in HBM, and returns after its kernels have completed and the rows - and
 * the label plane, if one was asked for - have arrived.  THE PLAN IS A SNAPSHOT, THE FRONTIERS COME FROM THE CURRENT COUNTERS: frames
 * integrated since the potential call move the frontiers and not the potentials they are ranked by.  That is intended - a node plans
 * at a lower rate than it maps - and a caller who wants both of one moment calls kicp_grid_potential first.  The call reads the plan
 * and never writes it: a plan stays valid, its q and potential unchanged, and the counters are untouched too.  use_plan != 0 on a
 * handle without a valid plan (kicp_grid_has_plan) is KICP_ERR_ARG; the message says to call kicp_grid_potential first.
 * For both entries a null handle / occupancy, config or out_n, min_observations < 1, an occupied_thresh outside [0, 1], min_size < 1
 * and a cap_labels that is neither 0 nor width * height are KICP_ERR_ARG; *out_n is 0 after any of them. */
typedef struct kicp_frontier_config {
    unsigned int min_observations; /* >= 1 */
    double occupied_thresh;        /* in [0, 1] */
    unsigned int min_size;         /* >= 1: frontiers of fewer cells are not output */
} kicp_frontier_config;
#define KICP_FRONTIER_WORDS 10
int kicp_frontiers_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_frontier_config *config,
                                  const unsigned int *potential, unsigned long long *out_rows, size_t cap_rows, size_t *out_n,
                                  unsigned int *out_labels, size_t cap_labels);
int kicp_grid_frontiers(const kicp_grid *grid, const kicp_frontier_config *config, int use_plan, unsigned long long *out_rows, size_t cap_rows,
                        size_t *out_n, unsigned int *out_labels, size_t cap_labels);

/* ---- what the robot would see from there: the unknown cells a sensor reveals from candidate viewpoints (kicp_grid_explore.hip) ----------
 * The frontiers above say how far each frontier is; these entries say what lies behind it.  An exploration planner that goes past
 * "nearest frontier" scores candidate viewpoints by information gain: it casts the sensor's rays from the candidate over the map, stops
 * them at obstacles and counts the unknown cells they cross.  Everything below is integer and the result is unique: the host and the
 * device entry return equal arrays.
 *
 * CLASSES.  Those of the frontier section: with v the readout of a cell at `min_observations`, the cell is OCCUPIED when
 * (double)v > occupied_thresh * 100.0, UNKNOWN when v < 0, and CLEAR otherwise.  Cells outside the grid are nothing.
 *
 * VIEWPOINT.  A cell index y * width + x, an unsigned int below width * height: word 9 (best_cell) of a frontier's row can be passed
 * as it is.
 *
 * RAYS.  Let R = range_cells, 1 <= R <= 361.  From a viewpoint (vx, vy) whose cell is CLEAR, 8 R rays are walked, one to each offset
 * (dx, dy) with max(|dx|, |dy|) == R.  Ray (dx, dy) visits the offsets (ox, oy) of steps k = 1, 2, .., R in that order, by the
 * integrator's own walk with m = R:  ox = sign(dx) * ((2 k |dx| + R) / (2 R)),  oy = sign(dy) * ((2 k |dy| + R) / (2 R)),  integer
 * divisions.  k = 0, the viewpoint's own cell, is not visited.  At each step these tests apply IN THIS ORDER:
 *   1. ox * ox + oy * oy > R * R: the ray ends and nothing is counted - the range is a disc;
 *   2. the cell (vx + ox, vy + oy) lies outside the grid: the ray ends and counts as LEFT;
 *   3. the cell is OCCUPIED: the ray ends and counts as BLOCKED; the cell is not seen;
 *   4. the cell is UNKNOWN: it is SEEN and the ray goes on - unknown space does not stop a ray, the optimistic sensor model that
 *      exploration planners use;
 *   5. the cell is CLEAR: the ray goes on.
 * A ray that completes step k = R ends and counts as neither LEFT nor BLOCKED.  On an empty plane the rays visit every offset of the
 * disc except (0, 0), about 2.2 visits per cell of it (70 096 at R = 100).
 *
 * ROW.  Per viewpoint KICP_GAIN_WORDS = 4 words of unsigned int, in the order of the viewpoints (duplicates give duplicate rows):
 *   0  the number of DISTINCT cells SEEN: a cell that several rays cross counts once
 *   1  rays BLOCKED
 *   2  rays LEFT
 *   3  the class of the viewpoint's own cell: 0 clear, 1 unknown, 2 occupied
 * When word 3 is not 0 no ray is walked and words 0 to 2 are 0.
 *
 * EXAMPLE.  Rows top down with y = 0 first, x left to right; 0 clear, 1 unknown, 2 occupied:
 *      111111111        viewpoint (x, y)   R = 1     R = 2     R = 3      R = 4
 *      100000211        (3, 3)             0,0,0,0   0,3,0,0   3,5,0,0    15,7,3,0
 *      100020111        (1, 1)             2,0,0,0   5,0,2,0   7,1,13,0   9,2,21,0
 *      100000011        (7, 5)             2,0,0,0   6,0,2,0   9,0,13,0   13,0,21,0
 *      120000001        (4, 2)             0,0,0,2   0,0,0,2   0,0,0,2    0,0,0,2
 *      100000001        (0, 0)             0,0,0,1   0,0,0,1   0,0,0,1    0,0,0,1
 *      111111111
 *
 * ENTRIES.  kicp_gain_from_occupancy is pure host code over a readout (width x height values as kicp_grid_occupancy writes them;
 * min_observations is only checked) and needs no GPU; width or height 0 is KICP_ERR_ARG, width * height above 2^28 KICP_ERR_CAPACITY.
 * kicp_grid_gain works on the counters where they are, in HBM, on the grid's stream (one workgroup per viewpoint, the window's bit
 * plane in LDS: that is where the limit of 361 cells comes from) and returns after the rows have arrived.  It writes neither the
 * counters nor the plan: kicp_grid_has_plan, the plan's words and kicp_grid_counts read the same afterwards.
 * n_views == 0 is KICP_OK and writes nothing.  cap_out is the number of words `out` holds and must be 4 * n_views -
 * kicp_grid_score_arcs's convention.  For both entries a null handle / occupancy or config, null views or out with n_views > 0,
 * min_observations < 1, an occupied_thresh outside [0, 1], range_cells outside 1 .. 361, a cap_out other than 4 * n_views and a
 * viewpoint >= width * height - checked on the host before anything is launched; the message names the first bad one - are
 * KICP_ERR_ARG with nothing written; more than 2^24 viewpoints in one call are KICP_ERR_CAPACITY. */
typedef struct kicp_gain_config {
    unsigned int min_observations; /* >= 1 */
    double occupied_thresh;        /* in [0, 1] */
    unsigned int range_cells;      /* R, 1 .. 361 */
} kicp_gain_config;
#define KICP_GAIN_WORDS 4
int kicp_gain_from_occupancy(const signed char *occupancy, unsigned int width, unsigned int height, const kicp_gain_config *config, const unsigned int *views,
                             size_t n_views, unsigned int *out /* n_views x 4 */, size_t cap_out);
int kicp_grid_gain(const kicp_grid *grid, const kicp_gain_config *config, const unsigned int *views, size_t n_views, unsigned int *out, size_t cap_out);

/* ---- what stands in known free space right now: the transient obstacles of one frame (kicp_grid_transient.hip) --------------------------
 * A cell the rays have crossed m times becomes a source of the clearance only after more than (occupied_thresh / (1 - occupied_thresh)) m
 * hits: somebody who steps into a corridor that was carved 200 times is lethal in the costmap half a minute later.  Nav2 closes that gap
 * with an obstacle layer fed by the current observation; these entries are its counterpart.  DETECTION finds the returns of one frame that
 * end in cells the counters know as free and groups them into transients, one row of integers each.  THE SWITCH makes those cells sources
 * of the clearance, the costmap and the potential.  Everything below is integer from the floor on and the result is unique: the host
 * and the device entries return equal arrays.
 *
 * USED POINT, ENDPOINT CELL, SENSOR CELL (sx, sy).  Exactly kicp_grid_integrate's: the same arithmetic, the same z band, the same reach
 * test.  The sensor cell may lie outside the grid.  n(c) is the number of used points whose endpoint cell is c, for c inside the grid;
 * endpoints outside the grid count nowhere.  n == 0 is legal; n > 0x7FFFFFF0 / 3 is KICP_ERR_CAPACITY, as for kicp_grid_integrate.
 *
 * TRANSIENT CELL.  With v the readout of the cell's counters as they stand at the call, at `min_observations`: cell c is a transient cell
 * when n(c) >= min_points and 0 <= v <= free_max.  An unknown cell (v < 0) never is one.  The call reads the counters and never writes
 * them; call it BEFORE integrating the same frame, so that the frame's own hit is not part of v yet.
 *
 * TRANSIENT.  Transient cells are joined to each of their eight neighbours that is a transient cell, with no corner rule.  A transient
 * is a connected component; its label is the least cell index y * width + x among its cells.  The label plane is width * height words
 * of unsigned int: the label on a transient cell, 0xFFFFFFFF on every other, and is NOT filtered by min_size.
 *
 * ROW.  Per transient KICP_TRANSIENT_WORDS = 10 words of unsigned long long:
 *   0           the label
 *   1           the size in cells
 *   2           the returns: the sum of n(c) over its cells
 *   3, 4        the sums of n(c) * x and n(c) * y (the centroid is the caller's division by word 2: none enters the contract)
 *   5, 6, 7, 8  min x, max x, min y, max y
 *   9           nearest: the least key d2(c) * 2^32 + c over its cells, d2(c) = (x - sx)^2 + (y - sy)^2
 * The reach test keeps |x - sx| and |y - sy| at or below 4095, so d2 < 2^25: the high half of word 9 is the squared distance in cells
 * from the sensor to the transient's nearest cell, the low half that cell - among equally near cells the least index.
 *
 * OUTPUT.  The rows with size >= min_size, in ascending label order.  *out_n, cap_rows, KICP_ERR_CAPACITY, out_labels and cap_labels
 * behave exactly as in kicp_grid_frontiers.  out_stats is nullable, four words: the points used, the used points whose endpoint cell
 * lies inside the grid, the cells with n(c) > 0, and the transient cells before min_size.
 *
 * THE TRANSIENT PLANE.  The handle keeps a byte per cell: 1 on the cells of the transients of the last call that passed min_size.  It is
 * all 0 before the first call, after kicp_grid_clear, and after a call with n == 0 or without any transient.  Every call replaces it
 * completely: nothing of the previous frame stays.  A call that returns KICP_ERR_CAPACITY for its rows has still replaced the plane; a
 * call that fails its argument checks leaves it as it was.  kicp_grid_transient_plane downloads it (cap_cells must be width * height).
 *
 * THE SWITCH.  kicp_grid_use_transients sets it, kicp_grid_uses_transients reads it; it is off at creation and kicp_grid_clear does not
 * change it.  While it is on, a cell whose plane byte is 1 is a SOURCE in kicp_grid_clearance, kicp_grid_costmap and kicp_grid_potential
 * whatever its counters say, and its base cost is 254.  Nothing else in those contracts changes: the result for a rectangle still
 * equals the full grid's restricted to it, and for occupied_thresh < 1 it equals what the kicp_grid_*_from_occupancy entries return over
 * the readout with those cells set to 100.  Occupancy, save_map and counts, kicp_grid_fill_unknown, kicp_grid_potential_of_costmap,
 * kicp_grid_frontiers and kicp_grid_gain ignore the plane whatever the switch says: a person is not a wall and must not open or close a
 * frontier.  A plan is a snapshot as before: it holds the transients of the moment kicp_grid_potential ran, and a later
 * kicp_grid_transients neither changes nor invalidates it.  What a node has to refresh after a frame is the union of the last two
 * frames' windows grown by R: the old plane's cells lay in the previous window.
 *
 * ENTRIES.  kicp_grid_transients takes the frame from host memory, kicp_grid_transients_device from HBM (the registered frame of the
 * pre-steps, say).  Both take the handle non-const because the plane is state they leave behind on purpose; they change no counter, not
 * the frame count, not the last window and not the plan, and return with the stream drained.  kicp_transients_from_counts is pure host
 * code over counters in kicp_grid_counts' layout and the grid's configuration (checked as kicp_grid_create checks it) and needs no GPU;
 * out_plane is nullable: cap_plane must be width * height with a plane and 0 without one.
 * A null handle / counts / configuration, pose, sensor, config or out_n, null points with n > 0, min_observations < 1, free_max > 100,
 * min_points < 1, min_size < 1 and a bad cap_labels or cap_plane are KICP_ERR_ARG; *out_n is 0 after any of them. */
typedef struct kicp_transient_config {
    unsigned int min_observations; /* >= 1 */
    unsigned int free_max;         /* 0 .. 100: known free is 0 <= v <= free_max; floor(occupied_thresh * 100) leaves no gap below the sources */
    unsigned int min_points;       /* >= 1: returns a cell needs */
    unsigned int min_size;         /* >= 1: cells a transient needs to be output and to enter the plane */
} kicp_transient_config;
#define KICP_TRANSIENT_WORDS 10
int kicp_grid_transients(kicp_grid *grid, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                         const kicp_transient_config *config, unsigned long long *out_rows, size_t cap_rows, size_t *out_n, unsigned int *out_labels,
                         size_t cap_labels, unsigned long long out_stats[4]);
int kicp_grid_transients_device(kicp_grid *grid, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                                const kicp_transient_config *config, unsigned long long *out_rows, size_t cap_rows, size_t *out_n,
                                unsigned int *out_labels, size_t cap_labels, unsigned long long out_stats[4]);
int kicp_transients_from_counts(const unsigned short *counts, const kicp_grid_config *grid_config, const double *frame_xyz, size_t n, const double pose_qt[7],
                                const double sensor_xyz[3], const kicp_transient_config *config, unsigned long long *out_rows, size_t cap_rows,
                                size_t *out_n, unsigned int *out_labels, size_t cap_labels, unsigned long long out_stats[4], unsigned char *out_plane,
                                size_t cap_plane /* 0 or width * height */);
int kicp_grid_transient_plane(const kicp_grid *grid, unsigned char *out, size_t cap_cells);
int kicp_grid_use_transients(kicp_grid *grid, int on);
int kicp_grid_uses_transients(const kicp_grid *grid);

/* ---- uneven ground: a column of heights per cell, and traversability by height over the local ground (kicp_elev.hip) -----------------
 * The grid above calls a return an obstacle when its BASE-FRAME z lies in a fixed band.  Where the floor is not one plane that is
 * wrong: a ramp ahead rises into the band and becomes a wall, a kerb or a drop below the band is invisible, a ceiling or a table top is
 * an obstacle or not by where z_max was put.  What decides is height over the LOCAL GROUND, so this layer keeps which world heights have
 * ever returned in every cell, and reads three classes off that.  Everything below is exact and integer from the floor on.
 *
 * THE LAYER is world aligned with the grid's geometry - width x height cells of side `cell` from (origin_x, origin_y), cell (ix, iy) at
 * iy * width + ix, max_ray - so its arrays overlay a kicp_grid of equal geometry, and a vertical one: z_origin and slab, in metres.
 * Each cell holds one 64-bit COLUMN: bit b is set when some used return ever had a world height in [z_origin + b slab, z_origin +
 * (b + 1) slab).  kicp_elev_integrate only ever sets bits; kicp_elev_update (CARVING, below) also clears them.
 *
 * A FRAME is n points in the base frame, the pose and the sensor's origin in the base frame, exactly as for kicp_grid_integrate.  With R,
 * t of the pose (pose_to_rt, evaluated once on the host):
 *   wx = ((r00 p.x + r01 p.y) + r02 p.z) + t0,  wy with row 1 and wz with row 2 likewise (every operation rounded on its own),
 *   cx = floor((wx - origin_x) / cell),  cy = floor((wy - origin_y) / cell),  s = floor((wz - z_origin) / slab);
 * the sensor's origin goes through the same arithmetic to the sensor cell (sx, sy); reach = ceil(max_ray / cell).  Each point falls into
 * exactly one of four classes, tested in this order, every comparison on doubles before any conversion:
 *   1 SKIPPED         p.x, p.y or p.z not finite, or wx, wy or wz not finite, or max(|cx - sx|, |cy - sy|) > reach (a comparison with
 *                     a NaN is false: a sensor cell that is not finite skips every point);
 *   2 OUTSIDE_GRID    not (0 <= cx < width and 0 <= cy < height);
 *   3 OUTSIDE_COLUMN  not (0 <= s <= 63);
 *   4 USED            bit s of the column of cell (cx, cy) is set.
 * There is no height band: every return counts.  The frame's statistics are six words: used, skipped, outside_grid, outside_column,
 * new_bits - bits that were clear before this frame - and new_cells - columns that were zero before this frame.  The first four sum to
 * n; all six depend only on the SET of (cell, slab) pairs of the frame and on the columns before it, not on the points' number or
 * order.  n == 0 is legal: nothing changes, the frame is counted.  n > 0x7FFFFFF0 / 3: KICP_ERR_CAPACITY.
 *
 * TRAVERSABILITY.  With step_slabs = S, 0 <= S <= 62, and robot_slabs = H, S < H <= 64 (KICP_ERR_ARG otherwise), a cell with column c is
 *   -1 (unknown) when c == 0; otherwise, with g the index of the lowest set bit of c - the GROUND -,
 *   BODY  when some bit b of c has g + S < b <= g + H: something between step height and robot height over the ground; bits above
 *         g + H are overhead and ignored;
 *   STEP  when some 8-neighbour inside the grid has a column that is not zero whose ground g_n satisfies g - g_n > S: the HIGHER cell
 *         of an edge is marked, which keeps the robot off a kerb it would hit and off a ledge it would fall from;
 *   100 when BODY or STEP, else 0.  Neighbours outside the grid and unknown neighbours say nothing.
 * The entries take a rectangle x0, y0, w, h by the clearance entries' rule above: inside the grid, w and h >= 1, cap == w * h
 * (KICP_ERR_ARG otherwise), h * w values row-major from (x0, y0), and the result for a rectangle EQUALS the full grid's restricted to
 * it.  They write `out`, signed char classes in kicp_grid_occupancy's convention; out_ground (nullable), one unsigned char per cell: g,
 * 255 for an unknown cell; out_counts (nullable), four words: unknown, traversable, BODY, STEP only.  A frame changes classes only
 * inside its window grown by one cell; kicp_elev_last_window gives that window by kicp_grid_last_window's rules.
 * kicp_elev_traversability works on the columns where they are, in HBM, and returns after its kernel has completed and the values
 * have arrived; kicp_elev_traversability_from_columns is the same arithmetic as pure host code over columns in kicp_elev_columns'
 * layout (width * height <= 2^28, KICP_ERR_CAPACITY otherwise) and needs no GPU.
 *
 * INTO THE PLANNER'S CHAIN.  kicp_elev_to_grid writes the class of every cell into the counters of a kicp_grid whose cell, origin_x,
 * origin_y, width and height are bit-equal to the layer's, on the same device (KICP_ERR_ARG otherwise): an obstacle becomes (hits 1,
 * misses 0), a traversable cell (0, 1), an unknown cell (0, 0).  It replaces ALL counters, with the consequences kicp_grid_set_counts
 * has; the caller dedicates a grid handle to it.  At min_observations = 1 every GPU entry of that grid - kicp_grid_costmap,
 * kicp_grid_potential, kicp_grid_score_arcs, kicp_grid_frontiers, kicp_grid_gain - then runs on traversability, without a byte
 * crossing PCIe.
 *
 * THE SLOPE LIMIT.  BODY looks at one column and STEP at neighbours one cell away, so neither sees a gradient: at 0.1 m cells, 0.0625 m
 * slabs and S = 2, STEP fires only above 2 slabs per cell, 51 degrees.  Grounds are quantised to a slab and most ground cells between a
 * lidar's rings are unknown, so a slope comes from a least-squares plane through the known grounds of a window, in exact integers.
 * With the slope configuration L = radius_cells (1 .. 8), K = gate_slabs (0 .. 63), min_cells (3 .. 289), rise_slabs (0 .. 65535) and
 * run_cells (1 .. 65535) (KICP_ERR_ARG otherwise; the traversability configuration is checked as above), the FIT SET of a known cell
 * (x, y) with ground g is the cells (x + dx, y + dy) with |dx|, |dy| <= L that lie inside the grid, whose column is not zero and whose
 * ground g_n satisfies |g_n - g| <= K; the cell itself always belongs.  With z = g_n - g, nine integer sums are taken over the set:
 * n, Sx = sum dx, Sy, Sxx, Sxy, Syy, Sz, Sxz, Syz.  The normal equations of z ~ a dx + b dy + c give by Cramer's rule
 *   D  = Sxx (Syy n - Sy Sy) - Sxy (Sxy n - Sy Sx) + Sx (Sxy Sy - Syy Sx)
 *   Da = Sxz (Syy n - Sy Sy) - Sxy (Syz n - Sy Sz) + Sx (Syz Sy - Syy Sz)
 *   Db = Sxx (Syz n - Sz Sy) - Sxz (Sxy n - Sy Sx) + Sx (Sxy Sz - Syz Sx)
 * The cell HAS A FIT when n >= min_cells and D > 0 (D is a Gram determinant: 0 when the set lies on one line); the gradient is then
 * (Da / D, Db / D) slabs per cell, and the cell is
 *   SLOPE when it has a fit and (Da^2 + Db^2) run_cells^2 > rise_slabs^2 D^2 - strictly, on exact integers, without a division.
 * A cell without a fit is not SLOPE: like an unknown neighbour, it says nothing.  The value of a cell is -1 when it is unknown, 100 when
 * BODY, STEP or SLOPE, else 0; BODY and STEP are exactly as above, so wherever a cell is not "SLOPE only" its value equals
 * kicp_elev_traversability's.  out_counts (nullable) is five words (KICP_ELEV_SLOPE_COUNTS): unknown, traversable, BODY, STEP only,
 * SLOPE only - SLOPE without BODY or STEP.  out_fit (nullable): w * h triples D, Da, Db, row-major as `out`; 0, 0, 0 where the cell has
 * no fit.  The widths: at L = 8, n <= 289, Sxx <= 6 936, |Sxy| <= 5 184, |Sz| <= 18 207 and |Sxz| <= 77 112, so the sums fit 32-bit
 * integers; D < 2^34 and |Da|, |Db| < 2^41, so the determinants fit 64-bit ones; the two sides of the comparison stay below 2^115 and
 * 2^100 and are formed as 128-bit products - never in fp64.  The rectangle rules are the ones above: a rectangle's result EQUALS the
 * full layer's restricted to it - window cells outside the rectangle but inside the grid count, cells outside the grid do not - and
 * a frame changes the result only inside kicp_elev_last_window grown by max(1, L) cells.  ADVICE: choose K >= (S + 1) L; whatever STEP
 * does not catch then stays in the fit set.  kicp_elev_traversability_slope_from_columns is the same arithmetic as pure host code
 * and needs no GPU; kicp_elev_to_grid_slope follows kicp_elev_to_grid's rules - the same checks, the same counters written.
 * kicp_elev_slope_limit turns a tangent into a limit for a layer's cell and slab: run_cells = 1024 and rise_slabs =
 * floor(((max_tangent cell) / slab) 1024), each operation rounded on its own; KICP_ERR_ARG when that is not finite, is negative or
 * exceeds 65 535 (of the configuration only cell and slab are read: positive and finite).
 *
 * ROUGH.  BODY, STEP and SLOPE do not look at how badly the grounds fit the plane: rubble whose neighbouring grounds differ by less
 * than S slabs around a level plane passes all three.  kicp_elev_traversability_rough adds the class ROUGH from the residual of the SAME
 * fit: the fit set, the window, the gate, min_cells and "HAS A FIT" are the slope limit's, unchanged.  A tenth sum is taken over the fit
 * set, Szz = sum z^2 (at most 289 * 63^2 = 1 147 041), and a fourth determinant, the intercept's:
 *   Dc = Sxx (Syy Sz - Sy Syz) - Sxy (Sxy Sz - Sx Syz) + Sxz (Sxy Sy - Syy Sx)
 *   Q  = D Szz - Da Sxz - Db Syz - Dc Sz
 * Q is D times the residual sum of squares of the fit set to its least-squares plane: in exact arithmetic 0 <= Q <= D Szz < 2^55.  With
 * the rough configuration num (0 .. 65535) and den (1 .. 65535) (KICP_ERR_ARG otherwise) a cell is
 *   ROUGH when it has a fit and Q den > num n D - strictly, on exact integers, without a division or floating point:
 * the mean squared residual exceeds num / den slabs^2.  The value of a cell is -1 when it is unknown, 100 when BODY, STEP, SLOPE or
 * ROUGH, else 0; BODY, STEP and SLOPE are exactly as above, so wherever a cell is not "ROUGH only" its value equals
 * kicp_elev_traversability_slope's.  out_counts (nullable) is six words (KICP_ELEV_ROUGH_COUNTS): unknown, traversable, BODY, STEP only,
 * SLOPE only, ROUGH only - ROUGH without BODY, STEP or SLOPE.  out_fit (nullable): w * h times five values D, Da, Db, Q, n, all zero where
 * the cell has no fit; the first three equal the slope entry's triple.  The widths, at L = 8 and K = 63: |Sx|, |Sy| <= 612 < 2^10, Sxx,
 * Syy, |Sxy| < 2^13, |Sz| < 2^15, |Sxz|, |Syz| < 2^17, Szz < 2^21, so each of Dc's three terms stays below 2^42 and |Dc| < 2^44; the four
 * products of Q stay below 2^55 (D Szz), 2^58 (Da Sxz, Db Syz) and 2^59 (Dc Sz), together below 2^61, so Q is formed in 64-bit
 * integers with no partial sum near the sign bit.  Q den reaches 2^71 and is a 128-bit product; num n D stays below 2^59.  The
 * rectangle and window rules are the slope limit's: a rectangle's result equals the full layer's restricted to it, and a frame changes
 * results only inside kicp_elev_last_window grown by max(1, L).  kicp_elev_traversability_rough_from_columns is the same arithmetic as
 * pure host code and needs no GPU; kicp_elev_to_grid_rough follows kicp_elev_to_grid's rules - the same checks, the same counters
 * written.  kicp_elev_rough_limit turns an r.m.s. residual in metres into a limit for a layer's slab: den = 1024 and num =
 * floor(((rms / slab) (rms / slab)) 1024), each operation rounded on its own; KICP_ERR_ARG when that is not finite, is negative or
 * exceeds 65 535 (of the configuration only slab is read: positive and finite).
 *
 * WHAT THE LAYER DOES NOT KNOW.  The layer knows only cells that returned a point; between a lidar's rings most of the floor is
 * unknown to it, while the mapping grid's rays have carved those cells free.  kicp_grid_fill_unknown (with the grid, above) fills the
 * unknown cells of the grid that kicp_elev_to_grid* wrote from the mapping grid, on the GPU, and never changes a cell the layer knows.
 * A filled cell has no ground, so it takes no part in STEP or in a fit, and a hole that the rays cross is free, as it is in the grid.
 *
 * CARVING ALONG THE FRAME'S RAYS.  kicp_elev_integrate only ever sets bits.  An UPDATE of a frame (kicp_elev_update*) is a CARVE - bits
 * that the frame's rays pass through are cleared - and then the mark that kicp_elev_integrate does, so a frame's own returns always
 * survive it.  With the carve configuration G = margin_steps, W = widen_slabs (0 .. 64) and keep_ground (0 or 1; KICP_ERR_ARG
 * otherwise):
 *   the sensor's slab is ss = floor((wz_sensor - z_origin) / slab), wz_sensor from row 2 of the pose exactly as a point's wz; when ss
 *   does not satisfy -32768 <= ss <= 32767 (a NaN fails it) the frame carves nothing.
 *   A point is ELIGIBLE when its class (the four above, unchanged) is not SKIPPED and its s satisfies -32768 <= s <= 32767, compared
 *   on doubles; s of an OUTSIDE_GRID point is computed as for any other.  OUTSIDE_GRID and OUTSIDE_COLUMN points do carve - without
 *   the rays of ceiling returns nothing above the sensor would ever clear -; points skipped for reach do not, as in the grid.
 *   THE RAY of a distinct triple (ex, ey, es) of an eligible point, with dx = ex - sx, dy = ey - sy, d = es - ss, m = max(|dx|, |dy|),
 *   takes the steps k = 0 .. m - 1 - G: none when m <= G, and m = 0 never carves.  The cell of step k is the grid's walk's (step k
 *   visits (sx + sgn(dx) ((2 k |dx| + m) / (2 m)), sy + sgn(dy) ((2 k |dy| + m) / (2 m))), integer divisions): it starts at the
 *   sensor's cell and never reaches the endpoint cell.  The slab of the ray at parameter j / (2 m) is
 *     u(j) = ss + sgn(d) ((j |d| + m) / (2 m))   (integer division; u(0) = ss, u(2 m) = es; j <= 8191, |d| <= 65535: below 2^29).
 *   Step k spans a = u(max(2 k - 1, 0)) to b = u(2 k + 1); lo = min(a, b) - W, hi = max(a, b) + W; its MASK is the bits max(lo, 0) ..
 *   min(hi, 63), empty when hi < 0 or lo > 63.
 *   THE COLUMNS.  For a cell inside the grid with column c before the frame, let M be the OR of the masks of all steps of all rays that
 *   visit it.  The carved column is c & ~(M & ~keep), keep = c & -c - the column's lowest set bit, which is then never cleared - with
 *   keep_ground, else 0.  The mark then ORs in the frame's USED bits as above.  Cells outside the grid are ignored; a ray whose sensor
 *   cell or endpoint cell lies outside still carves the cells inside that it visits.
 * The statistics are nine words (KICP_ELEV_UPDATE_STATS): the six above, new_bits and new_cells counted relative to the CARVED columns;
 * carve_points, the eligible points (0 when ss is out of range); bits_cleared; cells_emptied, the columns that were not zero before and
 * are zero after the carve (always 0 with keep_ground).  The columns, bits_cleared and cells_emptied depend only on the SET of triples
 * and on the columns before the frame.  Every visited cell lies within reach of the sensor's cell, so kicp_elev_last_window and
 * "classes change only inside the window grown by one cell" hold for an update as for an integrate.  kicp_elev_update and
 * kicp_elev_update_device mirror the two integrate entries in arguments, errors, frame count, last window and n == 0;
 * kicp_elev_update_columns is the same arithmetic as pure host code over columns in kicp_elev_columns' layout (`cells` must be the
 * configuration's width * height; the configuration is checked as kicp_elev_create checks it) and needs no GPU.
 *
 * KNOWN LIMITATIONS.  Bits clear only under kicp_elev_update*: kicp_elev_integrate never clears one.  Returns beyond reach do not
 * carve.  With keep_ground, a cell whose floor was never seen keeps a passer-by's lowest bit until a floor return arrives; without it
 * grazing rays erode the floor.  One spurious low return lowers a cell's ground for good: keep_ground keeps exactly that bit.  A cell that has only
 * ever returned an overhang, its ground unseen, reads as a high ground and is marked STEP until a ground return arrives - conservative
 * by choice.  SLOPE and ROUGH are classes, not costs, and the fit has no robustness to outliers beyond the gate.
 *
 * Limits: width * height <= 2^28 and reach <= 4095 (KICP_ERR_CAPACITY, the size in the message); cell, max_ray and slab positive and
 * finite, the origin and z_origin finite, width and height >= 1, no null pointer but the nullable outputs (KICP_ERR_ARG).  Every
 * entry returns after its work on the GPU has completed. */
typedef struct kicp_elev kicp_elev;
typedef struct kicp_elev_config {
    double cell, origin_x, origin_y; /* metres */
    unsigned int width, height;      /* cells */
    double z_origin, slab;           /* metres: bit b of a column is the world heights [z_origin + b slab, z_origin + (b + 1) slab) */
    double max_ray;                  /* metres: returns whose cell is farther than ceil(max_ray / cell) cells from the sensor's are skipped */
} kicp_elev_config;
typedef struct kicp_elev_traversability_config {
    unsigned int step_slabs;  /* S: the highest step the robot takes, in slabs: 0 .. 62 */
    unsigned int robot_slabs; /* H: the robot's height in slabs: S < H <= 64 */
} kicp_elev_traversability_config;
typedef struct kicp_elev_carve_config {
    unsigned int margin_steps; /* G: the last G steps of every ray before its endpoint cell are not carved */
    unsigned int widen_slabs;  /* W: 0 .. 64, each step's span of slabs is widened by W on both sides */
    unsigned int keep_ground;  /* 0 or 1: the lowest set bit of a column is never cleared */
} kicp_elev_carve_config;
#define KICP_ELEV_STATS 6
#define KICP_ELEV_UPDATE_STATS 9
int kicp_elev_create(const kicp_elev_config *config, int device, kicp_elev **out);
void kicp_elev_destroy(kicp_elev *elev);
/* the configuration, reach, and the frames integrated since creation or the last kicp_elev_clear (each nullable) */
int kicp_elev_info(const kicp_elev *elev, kicp_elev_config *out_config, int *out_reach, unsigned long long *out_frames);
int kicp_elev_clear(kicp_elev *elev); /* every column and the frame count back to zero */
/* One frame: from host memory (through the handle's pinned staging buffer), or where the points already are in HBM, complete - what
 * the drop-in pipeline calls.  out_stats (nullable): the six words above. */
int kicp_elev_integrate(kicp_elev *elev, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                        unsigned long long out_stats[6]);
int kicp_elev_integrate_device(kicp_elev *elev, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                               unsigned long long out_stats[6]);
/* One frame as an UPDATE: the carve along its rays, then the mark.  out_stats (nullable): the nine words above. */
int kicp_elev_update(kicp_elev *elev, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                     const kicp_elev_carve_config *carve_config, unsigned long long out_stats[9]);
int kicp_elev_update_device(kicp_elev *elev, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                            const kicp_elev_carve_config *carve_config, unsigned long long out_stats[9]);
int kicp_elev_update_columns(const kicp_elev_config *config, unsigned long long *columns, size_t cells, const double *frame_xyz, size_t n,
                             const double pose_qt[7], const double sensor_xyz[3], const kicp_elev_carve_config *carve_config,
                             unsigned long long out_stats[9]);
/* The columns, one 64-bit word per cell; cap_cells / cells must be the layer's width * height (KICP_ERR_ARG otherwise).
 * kicp_elev_set_columns replaces them all (the frame count is not part of them). */
int kicp_elev_columns(const kicp_elev *elev, unsigned long long *out, size_t cap_cells);
int kicp_elev_set_columns(kicp_elev *elev, const unsigned long long *in, size_t cells);
int kicp_elev_last_window(const kicp_elev *elev, unsigned int *x0, unsigned int *y0, unsigned int *w, unsigned int *h);
int kicp_elev_traversability(const kicp_elev *elev, const kicp_elev_traversability_config *config, unsigned int x0, unsigned int y0, unsigned int w,
                             unsigned int h, signed char *out, unsigned char *out_ground, unsigned long long out_counts[4], size_t cap);
int kicp_elev_traversability_from_columns(const unsigned long long *columns, unsigned int width, unsigned int height,
                                          const kicp_elev_traversability_config *config, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h,
                                          signed char *out, unsigned char *out_ground, unsigned long long out_counts[4], size_t cap);
int kicp_elev_to_grid(const kicp_elev *elev, const kicp_elev_traversability_config *config, kicp_grid *grid);
/* The slope limit (THE SLOPE LIMIT above): the traversability with the class SLOPE from a plane fit over each cell's window. */
typedef struct kicp_elev_slope_config {
    unsigned int radius_cells; /* L: 1 .. 8, the window is (2L+1) x (2L+1) cells around the cell */
    unsigned int gate_slabs;   /* K: 0 .. 63, a window cell counts only when its ground differs from the cell's by at most K */
    unsigned int min_cells;    /* 3 .. 289: fewer cells in the fit say nothing */
    unsigned int rise_slabs;   /* 0 .. 65535 */
    unsigned int run_cells;    /* 1 .. 65535: the limit is rise_slabs slabs of height per run_cells cells of distance */
} kicp_elev_slope_config;
#define KICP_ELEV_SLOPE_COUNTS 5
int kicp_elev_traversability_slope(const kicp_elev *elev, const kicp_elev_traversability_config *config, const kicp_elev_slope_config *slope_config,
                                   unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, signed char *out, unsigned char *out_ground,
                                   long long *out_fit, unsigned long long out_counts[5], size_t cap);
int kicp_elev_traversability_slope_from_columns(const unsigned long long *columns, unsigned int width, unsigned int height,
                                                const kicp_elev_traversability_config *config, const kicp_elev_slope_config *slope_config,
                                                unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, signed char *out,
                                                unsigned char *out_ground, long long *out_fit, unsigned long long out_counts[5], size_t cap);
int kicp_elev_to_grid_slope(const kicp_elev *elev, const kicp_elev_traversability_config *config, const kicp_elev_slope_config *slope_config,
                            kicp_grid *grid);
int kicp_elev_slope_limit(const kicp_elev_config *config, double max_tangent, unsigned int *rise_slabs, unsigned int *run_cells);
/* ROUGH (above): the traversability with the classes SLOPE and ROUGH from the plane fit and its residual. */
typedef struct kicp_elev_rough_config {
    unsigned int num; /* 0 .. 65535 */
    unsigned int den; /* 1 .. 65535: the limit is a mean squared residual of num / den slabs^2 */
} kicp_elev_rough_config;
#define KICP_ELEV_ROUGH_COUNTS 6
int kicp_elev_traversability_rough(const kicp_elev *elev, const kicp_elev_traversability_config *config, const kicp_elev_slope_config *slope_config,
                                   const kicp_elev_rough_config *rough_config, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h,
                                   signed char *out, unsigned char *out_ground, long long *out_fit, unsigned long long out_counts[6], size_t cap);
int kicp_elev_traversability_rough_from_columns(const unsigned long long *columns, unsigned int width, unsigned int height,
                                                const kicp_elev_traversability_config *config, const kicp_elev_slope_config *slope_config,
                                                const kicp_elev_rough_config *rough_config, unsigned int x0, unsigned int y0, unsigned int w,
                                                unsigned int h, signed char *out, unsigned char *out_ground, long long *out_fit,
                                                unsigned long long out_counts[6], size_t cap);
int kicp_elev_to_grid_rough(const kicp_elev *elev, const kicp_elev_traversability_config *config, const kicp_elev_slope_config *slope_config,
                            const kicp_elev_rough_config *rough_config, kicp_grid *grid);
int kicp_elev_rough_limit(const kicp_elev_config *config, double rms_metres, unsigned int *num, unsigned int *den);

/* ---- the map follows the robot: scrolling the grid and the height layer (kicp_grid.hip, kicp_elev.hip; kernel kicp_scroll.hpp) ---------
 * A handle's width, height and cell are fixed, its origin is not: a SCROLL moves the window of the world the handle covers by whole
 * cells, on the GPU, and keeps every cell that stays inside.  Everything below is exact: integers, and two rounded fp64 operations for
 * the origin.
 *
 * THE SHIFT OF A PLANE.  A plane is width x height elements, element (ix, iy) at iy * width + ix.  Shifted by (dx, dy), element
 * (ix, iy) of the result is the input's element (ix + dx, iy + dy) where that lies inside the plane, and 0 elsewhere.  dx > 0 moves the
 * window towards +x: the columns 0 .. dx - 1 leave, and dx empty columns enter at the high end.  |dx| >= width or |dy| >= height leaves
 * all zeros; (0, 0) is the identity.  kicp_shift_plane is that shift as pure host code for elements of elem_bytes = 1, 2, 4 or 8 - the
 * host twin for the transient plane, a single counter plane, the counter pairs and the height columns; `in` and `out` must not overlap,
 * width and height >= 1 (KICP_ERR_ARG otherwise), width * height <= 2^28 (KICP_ERR_CAPACITY).  It needs no GPU.
 *
 * kicp_grid_scroll by (dx, dy):
 *   - shifts the counters, one 32-bit element per cell - the hits and misses pair -, and the transient plane if it is allocated;
 *   - sets origin_x = origin_x + (double)dx * cell - the product rounded, then the sum rounded, never one fused operation - and origin_y
 *     likewise with dy;
 *   - translates the last frame's window by (-dx, -dy); kicp_grid_last_window clips it as before, so it may come out empty (a window
 *     pushed more than 2^30 cells from the grid is forgotten, as if no frame had been integrated: no shift brings a cell of it back);
 *   - INVALIDATES THE PLAN (kicp_grid_has_plan reads 0 until the next potential call): the plan's cells no longer mean what they meant;
 *   - leaves the frame count, the transient switch and every field of the configuration but the origin as they are.
 * There is no hidden state: after the call the handle is indistinguishable from one created with the configuration kicp_grid_info now
 * reports and given the shifted counters by kicp_grid_set_counts (and the shifted plane); every later entry returns the same bytes on
 * both.  dx == dy == 0 changes nothing, the plan included.  A new origin that is not finite is KICP_ERR_ARG, and nothing changes.  The
 * shift writes into a second buffer of the counters' size, which the handle allocates at the first shift that needs it and keeps - a
 * scrolled handle holds its counters twice -; when that allocation fails the call fails as any allocation does, and nothing has
 * changed.  A shift that empties the plane needs no second buffer.  The call returns after its work on the GPU has completed.
 * kicp_elev_scroll is the same for the height columns, one 64-bit element per cell, with the layer's origin and last window.  A planner
 * grid fed by kicp_elev_to_grid* is scrolled by the same (dx, dy) by its owner; the same sequence of shifts gives both the same origin,
 * bit for bit, because the rule is the same arithmetic.
 *
 * FOLLOWING.  kicp_follow_shift is the rule for one axis, pure host code: for a cell index c on an axis of `size` cells, *d = 0 when
 * margin <= c < size - margin; for c < margin, *d = -step * ceil((margin - c) / step); for c >= size - margin,
 * *d = step * ceil((c - (size - margin) + 1) / step), in integers.  It requires margin >= 1, step >= 1 and 2 * margin + step <= size
 * (KICP_ERR_ARG otherwise, and when d would leave 64 bits); under these the cell lands in the band: margin <= c - d < size - margin.
 * kicp_grid_follow computes the cell of (x, y) with the grid's own arithmetic, floor((x - origin_x) / cell) and floor((y - origin_y) /
 * cell), applies the rule per axis with width and height, scrolls ONCE by both and reports the shift applied (out_dx, out_dy, each
 * nullable).  (0, 0) is the common case: host arithmetic only, no launch.  A position that is not finite, or whose cell lies beyond
 * +-2^30, and a bad margin or step are KICP_ERR_ARG with nothing changed.  kicp_elev_follow does the same for the height layer.
 *
 * RECTANGLES OF COUNTERS.  kicp_grid_counts_rect and kicp_grid_set_counts_rect are kicp_grid_counts and kicp_grid_set_counts
 * restricted to the rectangle x0, y0, w, h: inside the grid, w and h >= 1, cap_cells / cells == w * h (KICP_ERR_ARG otherwise); the
 * layout is row-major from (x0, y0), two words per cell.  kicp_grid_set_counts_rect invalidates nothing and is otherwise a write like
 * kicp_grid_set_counts.  With them a caller pages what leaves the window into a larger map of their own: before a scroll by (dx, dy)
 * the cells that leave are the |dx| columns at the low (dx > 0) or high (dx < 0) end over all rows, and the |dy| rows at the low or
 * high end over the remaining columns; after a scroll back the same two rectangles take them again.
 *
 * NOT THERE.  A grid that grows; toroidal addressing; automatic paging; rectangles of height columns; a plan carried across a scroll;
 * a voxel map that scrolls. */
int kicp_grid_scroll(kicp_grid *grid, int dx, int dy);
int kicp_grid_follow(kicp_grid *grid, double x, double y, unsigned int margin, unsigned int step, int *out_dx, int *out_dy);
int kicp_grid_counts_rect(const kicp_grid *grid, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, unsigned short *out, size_t cap_cells);
int kicp_grid_set_counts_rect(kicp_grid *grid, unsigned int x0, unsigned int y0, unsigned int w, unsigned int h, const unsigned short *in, size_t cells);
int kicp_elev_scroll(kicp_elev *elev, int dx, int dy);
int kicp_elev_follow(kicp_elev *elev, double x, double y, unsigned int margin, unsigned int step, int *out_dx, int *out_dy);
int kicp_shift_plane(const void *in, void *out, unsigned int width, unsigned int height, unsigned int elem_bytes, int dx, int dy);
int kicp_follow_shift(long long c, unsigned int size, unsigned int margin, unsigned int step, long long *d);

/* ---- map points the new frame sees through: a cube-map depth test (kicp_view.hip) ----------------------------------------------------
 * The local map loses points by distance only (RemovePointsFarFromLocation); whatever stood in view for one frame - a person crossing,
 * a forklift, a door leaf - stays until the robot is max_range away.  A kicp_view holds a depth image of ONE frame, and
 * kicp_map_remove_seen_through removes the map points that frame looks past.  Everything below is exact: subtractions, divisions,
 * floor and comparisons in fp64, every operation rounded on its own - no atan2, no sqrt.
 *
 * The image is a cube map of depths around the sensor, 6 faces of res x res pixels, the faces aligned to the WORLD axes.  Per frame:
 *   c = pose * sensor_xyz,   w = pose * p per point (quaternion rotation + translation, the very transform of kicp_map_update_pose: a
 *   point lands where Update(points, pose) files it),   v = w - c per component,   m = max(|v.x|, |v.y|, |v.z|)  - the depth (Chebyshev).
 * A point is USED iff p, w and m are finite and 0 < m <= max_ray; every other point is skipped.  A pose or sensor that is not finite
 * uses no point.  Face: the first axis in the order x, y, z whose |v| equals m, with that component's sign: 2 axis + (negative ? 1 : 0).
 * The other two components (a, b) are (y, z) for an x face, (x, z) for a y face, (x, y) for a z face.  Pixel:
 *   u  = min(res - 1, (int)floor((a / m + 1.0) * (res / 2.0))),   w_ = min(res - 1, (int)floor((b / m + 1.0) * (res / 2.0))),
 * element (face * res + w_) * res + u of the image.  A pixel holds the minimum over the frame's used points in it of (float)m (round to
 * nearest even), +inf when there is none: a minimum over the SET of points, whatever their order.
 *
 * The verdict for a world point q: v, m, face and pixel as above from q - c.  q is IN RANGE iff m is finite and 0 < m <= max_ray.  Of
 * the pixels (u + du, w_ + dw), |du|, |dw| <= window, that lie inside the SAME face (the window is clipped at the face's edges), N is
 * the number that are not empty and D the smallest value.  q is SEEN THROUGH iff it is in range, N >= min_rays and
 *   m + (margin + margin_per_metre * m) < (double)D        (fp64 as written, strict).
 * The window is what keeps a surface seen at a grazing angle: it then also holds nearer returns of the same surface.  (2 window + 1)
 * pixels must span the sensor's vertical beam spacing.
 *
 * kicp_map_remove_seen_through gives every point of every occupied voxel the verdict.  Seen-through points leave their bucket, the
 * survivors keep their relative order (a voxel's first point is then its first survivor), and a voxel that loses all its points is
 * erased as RemovePointsFarFromLocation erases one.  It collects a pending kicp_map_update_pose_device_begin first (and returns its
 * error), brings the map to the view's device if need be, runs there and leaves the HBM copy the current one; a map whose updates stay
 * on the host (a voxel beyond +-2^20) is swept on the host with the same verdict over the downloaded image.  An empty map or a view
 * that never rendered a frame: nothing is removed, KICP_OK.  out_stats (nullable): points in range, points removed, voxels that lost at
 * least one point, voxels erased.
 *
 * Limits: res even and 8 .. 1024, window 0 .. 4 (larger: KICP_ERR_CAPACITY), 1 <= min_rays <= (2 window + 1)^2, max_ray positive and
 * finite, both margins finite and not negative, no null pointer (KICP_ERR_ARG); n > 0x7FFFFFF0 / 3 points: KICP_ERR_CAPACITY. */
typedef struct kicp_view kicp_view;
typedef struct kicp_view_config {
    unsigned int res;        /* pixels per face edge */
    int window;              /* the verdict looks at (2 window + 1)^2 pixels */
    unsigned int min_rays;   /* of them at least this many must hold a return */
    double max_ray;          /* metres (Chebyshev): farther frame points are skipped, farther map points kept */
    double margin, margin_per_metre; /* metres, and metres per metre of depth */
} kicp_view_config;
int kicp_view_create(const kicp_view_config *config, int device, kicp_view **out);
void kicp_view_destroy(kicp_view *view);
/* the configuration, the sensor's world position c of the last frame (NaN before the first, or when that frame's pose or sensor was not
 * finite) and the frames rendered since creation (each nullable) */
int kicp_view_info(const kicp_view *view, kicp_view_config *out_config, double out_sensor_world[3], unsigned long long *out_frames);
/* One frame REPLACES the image.  kicp_view_render takes the points from host memory, kicp_view_render_device where they already are in
 * HBM, complete (kicp_pre_device_ptr(pre, 0, ..) after kicp_pre_frame has returned: what the drop-in pipeline calls).  Both return
 * after their kernel has completed.  out_stats (nullable): points used, points skipped.  n == 0 is legal: the image is empty then. */
int kicp_view_render(kicp_view *view, const double *frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                     unsigned long long out_stats[2]);
int kicp_view_render_device(kicp_view *view, const double *d_frame_xyz, size_t n, const double pose_qt[7], const double sensor_xyz[3],
                            unsigned long long out_stats[2]);
/* the image: 6 res^2 floats, face-major; cap must be that number (KICP_ERR_ARG otherwise) */
int kicp_view_depth(const kicp_view *view, float *out, size_t cap);
/* The verdict for n world points in host memory, one byte each: bit 0 (value 1) seen through, bit 1 (value 2) in range - so 0, 2 or 3.
 * Useful on its own, e.g. to filter a cloud before it is published. */
int kicp_view_classify(kicp_view *view, const double *points_xyz, size_t n, unsigned char *out);
int kicp_map_remove_seen_through(kicp_map *map, kicp_view *view, unsigned long long out_stats[4]);

/* ---- pre-steps of the pipeline on the GPU (pipeline/KinematicICP.cpp:54-62) -----------
 * A kicp_pre owns KICP_PRE_BUFFERS device point buffers.  Results stay in HBM (feed kicp_register_device with
 * kicp_pre_device_ptr) and are downloaded only when the host needs them (map update, return values). */
#define KICP_PRE_BUFFERS 4
typedef struct kicp_pre kicp_pre;
int kicp_pre_create(int device, kicp_pre **out);
void kicp_pre_destroy(kicp_pre *pre);
/* kiss_icp::Preprocessor::Preprocess(frame, timestamps, relative_motion) followed by transform_points(., lidar_to_base):
 * optional constant-velocity deskew to the scan end (when `deskew` and n_timestamps != 0), crop to
 * min_range < |p| < max_range in the sensor frame, then into the base frame.  Order preserved.  Host input. */
int kicp_pre_preprocess(kicp_pre *pre, const double *frame_xyz, size_t n, const double *timestamps, size_t n_timestamps,
                        const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range, double min_range,
                        int deskew, int dst_buffer, size_t *out_n);
/* PointCloud2 wire-format ingest: the raw message bytes go to the GPU (point_step bytes per
 * point instead of 32 B of fp64 xyz + stamp) and are decoded there.  Replaces
 *   ros/src/kinematic_icp_ros/utils/RosUtils.cpp:30-39        PointCloud2ToEigen(msg, T): FLOAT32 x,y,z -> T * Vector3d
 *   ros/src/kinematic_icp_ros/utils/TimeStampHandler.cpp:57-104  per-point stamp (UINT32 / FLOAT32 / FLOAT64) -> seconds as
 *                                                             double; values with more than 10 integer digits are ns
 *   ros/src/kinematic_icp_ros/utils/TimeStampHandler.cpp:106,121-128  min / max and normalisation (t - min) / (max - min)
 * `data` = msg->data.data(), n_points = width * height, borrowed for the call.  sensor_pose_qt may be NULL (= the identity
 * LidarOdometryServer.cpp:203 passes).  out_min/max_stamp (seconds; 0 when the cloud has no stamp field or is empty)
 * are what ProcessTimestamps needs for its begin/end-stamp logic (TimeStampHandler.cpp:111-119).  Any other stamp
 * datatype -> KICP_ERR_ARG ("timestamp field type not supported", TimeStampHandler.cpp:103). */
#define KICP_FIELD_UINT32 6  /* sensor_msgs::msg::PointField datatype codes */
#define KICP_FIELD_FLOAT32 7
#define KICP_FIELD_FLOAT64 8
typedef struct kicp_cloud_layout {
    unsigned int point_step;                  /* msg->point_step */
    unsigned int offset_x, offset_y, offset_z; /* offsets of the FLOAT32 fields "x", "y", "z" */
    int stamp_datatype;                       /* 0 = no "t"/"timestamp"/"time"/"stamps" field, else its datatype code */
    unsigned int offset_stamp;
} kicp_cloud_layout;
int kicp_pre_ingest(kicp_pre *pre, const void *data, size_t n_points, const kicp_cloud_layout *layout, const double sensor_pose_qt[7],
                    double *out_min_stamp, double *out_max_stamp);
/* 2-D LaserScan ingest: the raw ranges of a sensor_msgs::msg::LaserScan go to the GPU (4 bytes per beam) and are projected there,
 * into the slot kicp_pre_ingest fills.  Replaces the 2-D LiDAR mode of the node:
 *   ros/src/kinematic_icp_ros/nodes/online_node.cpp:44-58  laser_projector_.projectLaser(*msg, cloud, -1.0, channel_option::Timestamp)
 *                                                          (laser_geometry 2.x: the cosine table, cached per projector - here per
 *                                                          handle -, the range cutoff, x y z and the per-beam field "stamps")
 *   then, on that cloud, what kicp_pre_ingest replaces: TimeStampHandler.cpp:42-52,57-106,121-128 (the FLOAT32 stamp branch, min /
 *   max, normalisation - including its 0/0 when every kept stamp is equal) and RosUtils.cpp:30-39 (float x y z widened to double).
 * laser_geometry is not part of the reference tree: its rules are RECALLED, all in one place (kicp_pre_ingest.hpp, laser_rules).
 * range_cutoff < 0 (what the node passes) means range_max.  Afterwards kicp_pre_ingested_count is the number of kept beams,
 * kicp_pre_ingested returns the projected cloud (has_stamps = 1 when a beam was kept), and kicp_pre_preprocess_ingested /
 * kicp_pre_frame_ingested work on it.  out_min/max_stamp: the kept beams' stamps in seconds (0 when none was kept).  A pending
 * kicp_pre_ingest_ahead announcement is void.  No validation beyond the pointers: a NaN angle gives NaN points, as in laser_geometry. */
typedef struct kicp_laser_scan { /* the sensor_msgs::msg::LaserScan fields projectLaser reads */
    float angle_min, angle_max, angle_increment, time_increment, range_min, range_max;
} kicp_laser_scan;
int kicp_pre_ingest_scan(kicp_pre *pre, const float *ranges, size_t n_ranges, const kicp_laser_scan *scan, double range_cutoff,
                         double *out_min_stamp, double *out_max_stamp);
/* LOOK-AHEAD (round 5; a node that knows its next message - a bag replay, a queue of depth 2): announce the NEXT cloud.  Nothing is
 * copied yet; the next kicp_pre_frame[_ingested] call - the pre-steps of the CURRENT cloud - uploads and decodes the announced one into
 * a second slot on a stream of its own once its own kernels are queued, so the 2 MB of message k + 1 cross PCIe while the GPU works on
 * message k and the calling thread would only wait.  The kicp_pre_ingest call for the same message (same pointer, count, layout and
 * sensor pose) then finds it decoded and returns at once; any other message voids the announcement.  `data` must stay valid and
 * unchanged until that kicp_pre_ingest call.  Results are those of the plain kicp_pre_ingest, bit for bit. */
int kicp_pre_ingest_ahead(kicp_pre *pre, const void *data, size_t n_points, const kicp_cloud_layout *layout, const double sensor_pose_qt[7]);
unsigned long long kicp_pre_ahead_hits(const kicp_pre *pre); /* kicp_pre_ingest calls so far that found their message decoded ahead */
/* kicp_pre_preprocess on the ingested cloud (no host input; deskews only if the cloud carried stamps) */
int kicp_pre_preprocess_ingested(kicp_pre *pre, const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range,
                                 double min_range, int deskew, int dst_buffer, size_t *out_n);
/* Download the decoded cloud (fp64 xyz) and its normalised stamps: what PointCloud2ToEigen / ProcessTimestamps return. */
int kicp_pre_ingested(const kicp_pre *pre, double *out_xyz, double *out_stamps, size_t cap_points, size_t *out_n, int *out_has_stamps);
/* kiss_icp::VoxelDownsample(buffer src, voxel_size) -> buffer dst: the first point (lowest index) of every voxel, in the
 * ITERATION ORDER of the reference's tsl::robin_map after reserve(frame.size()) - the order the second downsample and the map
 * update of the pipeline depend on (kiss-icp v1.2.0 core/VoxelUtils.cpp; call sites pipeline/KinematicICP.cpp:40,42).
 * KICP_ERR_CAPACITY when a voxel coordinate leaves +-2^20 (the handle stays usable).  A coordinate that is not finite counts as
 * out of range: NaN and +-inf give KICP_ERR_CAPACITY too (the reference's float-to-int conversion of such a value is undefined). */
int kicp_pre_voxel_downsample(kicp_pre *pre, int src_buffer, double voxel_size, int dst_buffer, size_t *out_n);
/* Largest robin-hood displacement (in buckets) the last kicp_pre_voxel_downsample saw while replaying the reference's table
 * (0 when every probe stayed below 32).  tsl::robin_map grows its table when an insertion's probe exceeds the container's
 * limit (128 in robin-map 0.6.x once the load factor is >= 0.15, 8192 in 1.x) - a re-hash the replay does not model: a value at
 * or beyond the limit of the robin-map the reference was built against means the ORDER of that output may differ from the
 * reference's (the set of survivors never does). */
unsigned int kicp_pre_last_max_probe(const kicp_pre *pre);
/* The probe length beyond which the reference's container grows its table (default 128 = robin-map 0.6.x, what Ubuntu 22.04 ships
 * and USE_SYSTEM_TSL-ROBIN-MAP picks up; 8192 for robin-map 1.x; also KICP_ROBIN_PROBE_LIMIT in the environment).  A downsample whose
 * replay sees a longer probe returns KICP_WARN_TABLE_ORDER (> 0: the output is complete, its order is not vouched for). */
int kicp_pre_set_probe_limit(kicp_pre *pre, unsigned int limit);
/* The pre-steps of one frame as ONE call behind one host synchronisation (pipeline/KinematicICP.cpp:54-62): Preprocess +
 * transform_points into buffer 0, VoxelDownsample(buffer 0, voxel_a) into buffer 1, VoxelDownsample(buffer 1, voxel_b) into
 * buffer 2 - the results of kicp_pre_preprocess[_ingested] + two kicp_pre_voxel_downsample calls, element for element; each
 * step's survivor count stays on the device as the next step's input count.  out_counts = {points of buffer 0, 1, 2}.
 * out_frame_xyz (nullable; room for every INPUT point, cap_points >= n): buffer 0 starts travelling there in the background as
 * soon as it is complete - collect it with kicp_pre_download_finish(pre, 0, ...), whose out_n is out_counts[0]; the first
 * out_counts[0] points are the frame.  kicp_pre_frame: host input as kicp_pre_preprocess; kicp_pre_frame_ingested: the cloud
 * of the last kicp_pre_ingest (kicp_pre_ingested_count points).  May return KICP_WARN_TABLE_ORDER like the downsample.
 * Buffers 1 and 3 take turns between calls (round 6): the previous call's buffer 1 - device memory a map update begun with
 * kicp_map_update_pose_device_begin may still be reading - is buffer 3 afterwards, unchanged until the call after this one; a pointer
 * taken with kicp_pre_device_ptr(pre, 1, ..) stays valid that long. */
int kicp_pre_frame(kicp_pre *pre, const double *frame_xyz, size_t n, const double *timestamps, size_t n_timestamps,
                   const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range, double min_range, int deskew,
                   double voxel_a, double voxel_b, double *out_frame_xyz, size_t cap_points, size_t out_counts[3]);
int kicp_pre_frame_ingested(kicp_pre *pre, const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range,
                            double min_range, int deskew, double voxel_a, double voxel_b, double *out_frame_xyz, size_t cap_points,
                            size_t out_counts[3]);
/* kicp_pre_frame / kicp_pre_frame_ingested with the returned frame as the PointCloud2 `data` the node publishes for it
 * (RosUtils.cpp:40-63 EigenToPointCloud2 of the frame, LidarOdometryServer.cpp:240-263 PublishClouds): out_frame_xyz receives
 * x y z FLOAT32 records, static_cast<float> of the fp64 frame's doubles - the GPU narrows them on the way out, so 12 bytes per
 * point cross PCIe (kicp_pre_egress.hpp k_push_frame_f32).  out_frame_xyz may be NULL: then nothing is pushed at all (the node's "no
 * subscriber" case).  Otherwise collect it with kicp_pre_download_finish(pre, 0, NULL, 0, &n), as the fp64 entries' frame; the
 * first out_counts[0] records are the frame.  Buffer 2's host copy then holds records too: kicp_pre_download_f32(pre, 2, ...)
 * reads it; kicp_pre_download(pre, 2, ...) still returns the doubles (from HBM).  Everything else as the fp64 entries. */
int kicp_pre_frame_f32(kicp_pre *pre, const double *frame_xyz, size_t n, const double *timestamps, size_t n_timestamps,
                       const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range, double min_range, int deskew,
                       double voxel_a, double voxel_b, float *out_frame_xyz, size_t cap_points, size_t out_counts[3]);
int kicp_pre_frame_ingested_f32(kicp_pre *pre, const double relative_motion_qt[7], const double lidar_to_base_qt[7], double max_range,
                                double min_range, int deskew, double voxel_a, double voxel_b, float *out_frame_xyz, size_t cap_points,
                                size_t out_counts[3]);
size_t kicp_pre_ingested_count(const kicp_pre *pre);
/* Backend knobs of the chained pre-steps (not part of the reference API):
 *   "fused"  1 (default; KICP_PRE_FUSED=0 in the environment): kicp_pre_frame* run the frame's pre-steps as FIVE launches
 *            (kicp_pre.hpp: k_frame_*) and hand the three counts over through host memory the call polls; 0: one launch per
 *            step (preprocess, compact, 2 x {claim, replay, gather}) and a copy + stream synchronisation at the end.  Same results.
 *   "guess"  the survivor count from which the fused chain sizes its first table before it knows the real one (default: the
 *            previous frame's; the first frame: the input count).  A wrong power-of-two bracket costs the frame the unfused
 *            downsamples, never a different result.
 *   "fused_frames" / "guess_misses" (read only): frames the fused chain served / of those, frames whose guess was wrong.
 *   "point_tiles" / "l1_tiles" / "l2_workgroups" / "l2_tiles" (read only, host-side bookkeeping; 0 before the first fused frame):
 *            the last fused frame's 256-point tiles, 256-bucket tiles of its guessed first table, workgroups of its second-level
 *            launches and 256-bucket tiles of its second table (from the returned count; 0 when the guess was wrong).
 *   "scan_launches" (read only): launches of the separate block-count scan this handle has made so far - one per compaction
 *            or gather whose grid exceeds 4 096 workgroups.
 *   "push_launches" / "push_pieces" (read only): launches of the kernel that pushes a chained call's returned frame into host
 *            memory, piece by piece / pieces the copy worker has followed to their flag, summed over frames (it stops behind the
 *            first piece shorter than the frame's piece size; read it after kicp_pre_download_finish has collected the frame).
 * Which way the last decode went (read only, host-side bookkeeping; for tests that must prove the regime they ran in).
 * "ingest_*": the last kicp_pre_ingest that decoded its message itself (not one that took a look-ahead slot, not an empty one);
 * "ahead_*": the last look-ahead decode (kicp_pre_ingest_ahead + the chained pre-steps; read it after the kicp_pre_ingest call
 * that collects the message).  All are 0 before the first such decode.
 *   "ingest_launches"       launches of the decode kernel: one per piece of the message
 *   "ingest_workgroups"     workgroups of the widest of these launches (a look-ahead launch has at most 48, KICP_PRE_AHEAD_WGS,
 *                           and walks the piece's 256-record tiles with them)
 *   "ingest_piece_records"  records per piece: max(256, P / point_step / 256 * 256) with integer divisions, P = 512 KiB
 *                           (a look-ahead message: KICP_PRE_AHEAD_PIECE_KB, default 512 too)
 *   "ingest_aligned"        1: every field sits at a multiple of its size - point_step and the offsets of x, y, z multiples of 4,
 *                           the stamp's offset and point_step multiples of the stamp's size - and is read with plain loads;
 *                           0: byte-wise loads
 *   "ingest_wide"           1: point_step > 128, records read field by field from where they are; 0: staged through LDS
 *   "ingest_direct"         1: the kernel read the pinned staging buffer itself; 0: the bytes were copied into device memory first
 * Unknown names return -1. */
int kicp_pre_set_option(kicp_pre *pre, const char *name, double value);
double kicp_pre_get_option(const kicp_pre *pre, const char *name);
int kicp_pre_upload(kicp_pre *pre, int buffer, const double *xyz, size_t n);
int kicp_pre_download(const kicp_pre *pre, int buffer, double *out_xyz, size_t cap_points, size_t *out_n);
/* The same buffer as x y z FLOAT32 records, static_cast<float> of its doubles (RosUtils.cpp:40-63 EigenToPointCloud2,
 * LidarOdometryServer.cpp:240-263 PublishClouds: buffer 2 is the published keypoints).  After a kicp_pre_frame*_f32 call buffer 2's
 * records are already in host memory (narrowed by the chain's last launch); otherwise the GPU narrows the buffer and 12 bytes per
 * point are downloaded. */
int kicp_pre_download_f32(const kicp_pre *pre, int buffer, float *out_xyz, size_t cap_points, size_t *out_n);
/* The same download in the background: _begin queues the copy of the buffer's current contents on a stream of its own
 * (pinned landing area) and returns at once; the caller goes on with the pipeline's next steps and collects the points
 * with _finish.  One download in flight per handle; the buffer must not be refilled in between.  (RegisterFrame returns the
 * whole preprocessed frame - pipeline/KinematicICP.cpp:84 - 3 MB that nothing on the device waits for.) */
int kicp_pre_download_begin(kicp_pre *pre, int buffer);
/* Same, and a helper thread of the handle also moves the landed points into `out_xyz` (room for cap_points points, which must
 * stay valid until _finish) while the caller goes on: _finish with the same pointer (or NULL) then only waits for it. */
int kicp_pre_download_begin_into(kicp_pre *pre, int buffer, double *out_xyz, size_t cap_points);
int kicp_pre_download_finish(kicp_pre *pre, int buffer, double *out_xyz, size_t cap_points, size_t *out_n);
const double *kicp_pre_device_ptr(const kicp_pre *pre, int buffer, size_t *out_n);

/* Diagnostics: the demangled-name prefixes under which the registration's direct-dispatch path looks its kernels up in the
 * embedded code object, newline separated (tests check each against build/kicp_reg.hsaco, so a change of the compiler's
 * mangling or of a template signature fails a CPU test instead of silently disabling the path).  Returns the bytes needed. */
size_t kicp_aql_kernel_names(char *out, size_t cap);

/* Diagnostic behind bench.py's latency model: `workgroups` x `block` lanes each walk their own chain of `steps` DEPENDENT loads
 * through a random cyclic permutation of the 128-byte lines of a `working_set_bytes` buffer (the pass kernel's situation: a
 * wave's step costs the slowest of its 64 lanes' accesses, with the whole launch's accesses in flight around it).  Returns the
 * time per dependent step (whole-launch duration / steps, best of three warm launches, HIP events). */
int kicp_probe_dependent_load(int device, size_t working_set_bytes, int workgroups, int block, int steps, double *out_ns_per_step);
/* Bytes of the map's device copy a query can touch: table entries (occupied + halo, 128 B each) and the occupied voxels' buckets
 * (fp64 pool + 16-bit mirror), without the head-room around them; 0 before the first upload. */
size_t kicp_map_device_bytes(const kicp_map *map);

/* ---- device memory helpers for callers without a HIP runtime binding of their own ------------------------ */
int kicp_device_malloc(int device, size_t bytes, void **out_dptr);
int kicp_device_free(int device, void *dptr);
int kicp_device_upload(int device, void *dst_dptr, const void *src_host, size_t bytes);
int kicp_device_synchronize(int device);

/* ---- multi-GPU: scan points sharded across ranks, map replicated, one tiny all-reduce per ICP iteration
 *      (SURVEY.md section 8e).  Every rank calls kicp_register* with ITS shard and gets the identical pose.
 *      The payload is KICP_REDUCE_WORDS int64 values: the seven sums (JTJ00, JTJ01, JTJ11, JTr0, JTr1, sum||r||^2,
 *      N_corr) are accumulated exactly as 3 x 40-bit fixed-point limbs each, so an integer sum-all-reduce makes the
 *      result independent of the number of ranks, bit for bit. ---- */
#define KICP_REDUCE_WORDS 24
#define KICP_COMM_ID_BYTES 128
int kicp_comm_unique_id(char id[KICP_COMM_ID_BYTES]); /* rank 0 creates, the caller broadcasts the bytes */
int kicp_reg_comm_init(kicp_reg *reg, int nranks, int rank, const char id[KICP_COMM_ID_BYTES]); /* RCCL comm on reg's device */
int kicp_reg_comm_destroy(kicp_reg *reg);
/* Single-node alternative without any device collective: all ranks map one POSIX shared-memory segment (`name`, created
 * by rank 0 - call it there first, e.g. before a barrier).  Each rank's 24 limb totals + a sequence word go into its own slot
 * of the segment - written by its host, which has just added its GPU's tagged group rows exactly as in the single-GPU
 * hand-off -; every rank's host polls all slots, adds the integers and solves.  The "all-reduce" thus costs no more than the single-GPU hand-off (a 192-byte RCCL all-reduce
 * costs tens of microseconds per ICP iteration, as long as the kernel itself).  Every rank must issue the same sequence
 * of kicp_register* calls. */
int kicp_reg_shm_init(kicp_reg *reg, int nranks, int rank, const char *name);
int kicp_reg_shm_destroy(kicp_reg *reg);
/* One-shot exchange over peer mappings: no collective library, no host shared segment.  Every
 * rank (one process per GPU) owns a mailbox in its HBM.  The pass kernel's first reduction level ends in groups of 32
 * workgroups; the last workgroup of every group writes the group's row of 24 exact limb sums - tagged - into ALL ranks'
 * mailboxes (the peers' through IPC mappings: stores over xGMI), and the last workgroup of group 0 adds the rows of all
 * ranks' groups as they arrive in its own mailbox (integers, fixed order: bit-identical on every rank) and hands the totals
 * to its host, which solves - no second reduction level, no collective.  (A launch of more than 32 groups - 262 144 lanes
 * per rank - reduces on two levels and sends one row.)  Usage: every rank calls kicp_reg_p2p_export, the caller all-gathers the handles (any
 * transport), every rank calls kicp_reg_p2p_connect with the nranks handles in rank order; a barrier between connect and
 * the first registration, and before kicp_reg_p2p_destroy, is the caller's.  nranks <= KICP_P2P_MAX_RANKS.
 * Recovery contract: the ranks stay in step only while every exchange completes on every rank.  When a registration fails
 * after it has started an exchange (a peer's slot did not arrive within 0.8 x KICP_WAIT_TIMEOUT_S - the in-kernel wait is
 * derived from the host's setting -, a device fault), this rank's state is POISONED: every later kicp_register* call on the
 * handle returns KICP_ERR_COMM until kicp_reg_p2p_destroy, kicp_reg_p2p_export and kicp_reg_p2p_connect have been redone
 * (on every rank: the step counters restart from zero). */
#define KICP_P2P_HANDLE_BYTES 64
#define KICP_P2P_MAX_RANKS 16
int kicp_reg_p2p_export(kicp_reg *reg, int nranks, int rank, char handle[KICP_P2P_HANDLE_BYTES]);
int kicp_reg_p2p_connect(kicp_reg *reg, const char *handles /* nranks * KICP_P2P_HANDLE_BYTES, rank order */);
int kicp_reg_p2p_destroy(kicp_reg *reg);
/* Alternative to the built-in RCCL communicator: the caller supplies the sum-all-reduce (e.g. torch.distributed).
 * Called once per ICP iteration with a device buffer of `count` int64 values to be sum-reduced IN PLACE, ordered
 * on `stream` (a hipStream_t).  Return 0 on success.  Pass NULL to remove. */
typedef int (*kicp_allreduce_fn)(void *user, long long *d_buf, int count, void *stream);
int kicp_reg_set_allreduce(kicp_reg *reg, kicp_allreduce_fn fn, void *user);

#ifdef __cplusplus
}
#endif
#endif /* KICP_H_ */
