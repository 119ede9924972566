"""kinematic_icp::KinematicRegistration (kicp_reg_*, kicp_register*, kicp_pass_*, and the relocalisation entries that take a
registration handle): the hot path, its batch forms, pose scoring and refinement, the multi-GPU exchanges."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import Handle, _check, _d, _declare, _dp, _hp, _intp, _pose_ptr, _szp, _u32, _u32p, _u64, _u64p, lib
from .device import ALLREDUCE_FN, DeviceFrame
from .search import SearchWindow

MAX_LOG_PASSES = 32
P2P_HANDLE_BYTES = 64


class RegConfig(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("convergence_criterion", C.c_double), ("max_num_threads", C.c_int32),
                ("use_adaptive_odometry_regularization", C.c_int32), ("fixed_regularization", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("empty_map", C.c_int32), ("reserved", C.c_int32),
                ("beta", C.c_double), ("n_corr", C.c_double * MAX_LOG_PASSES), ("sums", (C.c_double * 6) * MAX_LOG_PASSES),
                ("dx", (C.c_double * 2) * MAX_LOG_PASSES), ("gpu_ms", C.c_double), ("pass_ms", C.c_double * MAX_LOG_PASSES)]


_vp, _f64, _sz = C.c_void_p, C.c_double, C.c_size_t
_register = (C.c_int, [_vp, _vp, _vp, _sz, _dp, _dp, _f64, _dp, C.POINTER(Stats)])  # (reg, map, points, n, last, rel, tau, pose out, stats)
_window = C.POINTER(SearchWindow)

_ENTRIES = _declare({
    "kicp_reg_create": (C.c_int, [C.POINTER(RegConfig), C.c_int, _hp]),
    "kicp_reg_destroy": (None, [_vp]),
    "kicp_reg_clone": (C.c_int, [_vp, _hp]),
    "kicp_reg_get_config": (C.c_int, [_vp, C.POINTER(RegConfig)]),
    "kicp_reg_set_config": (C.c_int, [_vp, C.POINTER(RegConfig)]),
    "kicp_reg_set_option": (C.c_int, [_vp, C.c_char_p, _f64]),
    "kicp_reg_get_option": (_f64, [_vp, C.c_char_p]),
    "kicp_register": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _dp, _f64, _dp, C.POINTER(Stats)]),
    "kicp_register_f32": _register,
    "kicp_register_device": _register,
    "kicp_register_device_batch": (C.c_int, [_vp, _vp, _sz, _hp, _szp, _dp, _dp, _f64, _dp, _intp]),
    "kicp_register_device_concurrent": (C.c_int, [_hp, _sz, _vp, _sz, _hp, _szp, _dp, _dp, _f64, _dp, _intp]),
    "kicp_pass_sums": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _f64, _dp]),
    "kicp_pass_correspondences": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _f64, C.POINTER(C.c_int32), _dp, _dp]),
    "kicp_pass_words": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _f64, C.POINTER(C.c_longlong)]),
    "kicp_score_poses": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _sz, _f64, _dp, _dp]),
    "kicp_score_poses_device": (C.c_int, [_vp, _vp, _vp, _sz, _dp, _sz, _f64, _dp, _dp]),
    "kicp_relocalize": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _sz, _f64, _sz, _dp, _szp, _dp, _dp]),
    "kicp_planar_sums": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _sz, _f64, _dp]),
    "kicp_planar_sums_device": (C.c_int, [_vp, _vp, _vp, _sz, _dp, _sz, _f64, _dp]),
    "kicp_planar_step": (C.c_int, [_dp, _dp, _dp, _dp]),
    "kicp_planar_grid": (_sz, [_dp, _f64, _f64, _f64, _f64, _f64, _f64, _dp, _sz]),
    "kicp_refine_poses_planar": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _sz, _f64, C.c_int, _f64, _dp, _intp, _intp]),
    "kicp_refine_poses_planar_device": (C.c_int, [_vp, _vp, _vp, _sz, _dp, _sz, _f64, C.c_int, _f64, _dp, _intp, _intp]),
    "kicp_relocalize_planar": (C.c_int, [_vp, _vp, _dp, _sz, _dp, _sz, _f64, _sz, C.c_int, _f64, _dp, _szp, _dp, _dp]),
    "kicp_occ_score_nodes": (C.c_int, [_vp, _vp, _dp, _sz, _window, C.c_int, _u64p, _sz, _u32p]),
    "kicp_search_poses": (C.c_int, [_vp, _vp, _dp, _sz, _window, _sz, _u64p, _u32p, _dp, _szp]),
    "kicp_relocalize_search": (C.c_int, [_vp, _vp, _vp, _dp, _sz, _window, _f64, _sz, C.c_int, _f64, _dp, _u64p, _dp, _dp]),
    "kicp_reg_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p]),
    "kicp_reg_comm_destroy": (C.c_int, [_vp]),
    "kicp_reg_shm_init": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p]),
    "kicp_reg_shm_destroy": (C.c_int, [_vp]),
    "kicp_reg_p2p_export": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p]),
    "kicp_reg_p2p_connect": (C.c_int, [_vp, C.c_char_p]),
    "kicp_reg_p2p_destroy": (C.c_int, [_vp]),
    "kicp_reg_set_allreduce": (C.c_int, [_vp, ALLREDUCE_FN, _vp]),
    "kicp_aql_kernel_names": (_sz, [C.c_char_p, _sz]),
})


def planar_step(sums, pose):
    """kicp_planar_step: one planar Gauss-Newton step on the host from one row of PlanarSums -> (pose[7], dx[3]), or None when the step is
    degenerate (N < 1, a non-finite sum, all accepted points on one (x, y))."""
    s = np.ascontiguousarray(np.asarray(sums, dtype=np.float64).reshape(8))
    q = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(7))
    out, dx = np.zeros(7, dtype=np.float64), np.zeros(3, dtype=np.float64)
    rc = lib().kicp_planar_step(s.ctypes.data_as(_dp), q.ctypes.data_as(_dp), out.ctypes.data_as(_dp), dx.ctypes.data_as(_dp))
    if rc < 0:
        _check(rc)
    return (out, dx) if rc == 1 else None


def planar_grid(center, half_x, half_y, half_yaw, step_x, step_y, step_yaw):
    """Candidate poses for Relocalize (kicp_planar_grid): center * planar(dx, dy, dyaw) for every offset i * step with |i * step| <= half
    extent, per axis - offsets in the centre's body frame, x slowest, yaw fastest -> (count, 7)."""
    _, c = _d(center)
    args = (float(half_x), float(half_y), float(half_yaw), float(step_x), float(step_y), float(step_yaw))
    n = lib().kicp_planar_grid(c, *args, None, 0)
    out = np.empty((n, 7), dtype=np.float64)
    lib().kicp_planar_grid(c, *args, out.ctypes.data_as(_dp), n)
    return out


class _Batch:
    pass


class KinematicRegistration(Handle):
    """kinematic_icp::KinematicRegistration (registration/Registration.hpp:32-50) on one MI355X."""

    _destroy = "kicp_reg_destroy"

    def __init__(self, max_num_iteration=10, convergence_criterion=1e-3, max_num_threads=1,
                 use_adaptive_odometry_regularization=True, fixed_regularization=0.0, device=0):
        cfg = RegConfig(max_num_iteration, convergence_criterion, max_num_threads, int(use_adaptive_odometry_regularization),
                        fixed_regularization)
        self._create("kicp_reg_create", C.byref(cfg), device)
        self._begin(device)

    def _begin(self, device):
        """what a handle starts with, created or cloned -> self"""
        self.device = device
        self.last_stats, self.last_status = Stats(), 0
        self._stats_ref = C.byref(self.last_stats)
        self._out = np.zeros(7, dtype=np.float64)
        self._out_p = C.cast(self._out.ctypes.data, _dp)
        self._cb = None
        self._lib = _ffi._lib  # loaded by now: ComputeRobotMotion* call through it without lib()'s check
        return self

    def copy(self):
        """KinematicRegistration(const KinematicRegistration &): the reference's struct is copyable (Registration.hpp:32-50);
        same parameters and tuning options, workspaces of its own (kicp_reg_clone)."""
        return KinematicRegistration._from("kicp_reg_clone", self._h)._begin(self.device)

    # the reference exposes its five parameters as public mutable fields (Registration.hpp:45-49)
    def _cfg(self):
        c = RegConfig()
        _check(lib().kicp_reg_get_config(self._h, C.byref(c)))
        return c

    def _set(self, **kw):
        c = self._cfg()
        for k, v in kw.items():
            setattr(c, k, v)
        _check(lib().kicp_reg_set_config(self._h, C.byref(c)))

    max_num_iterations_ = property(lambda s: s._cfg().max_num_iterations, lambda s, v: s._set(max_num_iterations=int(v)))
    convergence_criterion_ = property(lambda s: s._cfg().convergence_criterion, lambda s, v: s._set(convergence_criterion=float(v)))
    max_num_threads_ = property(lambda s: s._cfg().max_num_threads, lambda s, v: s._set(max_num_threads=int(v)))
    use_adaptive_odometry_regularization_ = property(lambda s: bool(s._cfg().use_adaptive_odometry_regularization),
                                                     lambda s, v: s._set(use_adaptive_odometry_regularization=int(bool(v))))
    fixed_regularization_ = property(lambda s: s._cfg().fixed_regularization, lambda s, v: s._set(fixed_regularization=float(v)))

    def set_option(self, name, value):
        _check(lib().kicp_reg_set_option(self._h, name.encode(), float(value)))

    def get_option(self, name):
        return lib().kicp_reg_get_option(self._h, name.encode())

    def ComputeRobotMotion(self, frame, voxel_map, last_robot_pose, relative_wheel_odometry, max_correspondence_distance):
        """frame: (N,3) float64 host array, or a DeviceFrame already resident in HBM."""
        lp, ro = _pose_ptr(last_robot_pose), _pose_ptr(relative_wheel_odometry)
        if isinstance(frame, DeviceFrame):
            rc = self._lib.kicp_register_device(self._h, voxel_map._h, frame.ptr, frame.n, lp, ro, max_correspondence_distance,
                                                self._out_p, self._stats_ref)
        elif isinstance(frame, np.ndarray) and frame.dtype == np.float32:
            # float32 xyz as a PointCloud2 carries it: widened on the device (kicp_register_f32), half the bytes over PCIe
            a = np.ascontiguousarray(frame)
            rc = self._lib.kicp_register_f32(self._h, voxel_map._h, a.ctypes.data, a.size // 3, lp, ro, max_correspondence_distance,
                                             self._out_p, self._stats_ref)
        else:
            a, p = _d(frame)
            rc = self._lib.kicp_register(self._h, voxel_map._h, p, a.size // 3, lp, ro, max_correspondence_distance,
                                         self._out_p, self._stats_ref)
        self.last_status = rc if rc >= 0 else _check(rc)
        return self._out.copy()

    def prepare_batch(self, frames, last_robot_poses, relative_wheel_odometries):
        """Marshal a queue of independent scans (DeviceFrames + their poses) once; run it with ComputeRobotMotionBatch."""
        k = len(frames)
        b = _Batch()
        b.frames = list(frames)  # keep the device buffers alive
        b.ptrs = (C.c_void_p * k)(*[f.ptr.value for f in frames])
        b.ns = (C.c_size_t * k)(*[f.n for f in frames])
        b.last = np.ascontiguousarray(np.asarray(last_robot_poses, dtype=np.float64).reshape(k, 7))
        b.rel = np.ascontiguousarray(np.asarray(relative_wheel_odometries, dtype=np.float64).reshape(k, 7))
        b.out = np.zeros((k, 7), dtype=np.float64)
        b.iterations = np.zeros(k, dtype=np.int32)
        b.count = k
        return b

    def ComputeRobotMotionBatch(self, batch, voxel_map, max_correspondence_distance):
        """kicp_register_device_batch: a queue of INDEPENDENT scans against one map; the library keeps several of them in flight
        (options "batch_queues" / "batch_depth"; 0 and 1: strictly one after the other), every pose bit-equal to
        ComputeRobotMotionDevice on that scan alone.  Returns the (count, 7) poses; batch.iterations holds the iteration counts."""
        rc = self._lib.kicp_register_device_batch(self._h, voxel_map._h, batch.count, batch.ptrs, batch.ns, batch.last.ctypes.data_as(_dp),
                                                  batch.rel.ctypes.data_as(_dp), max_correspondence_distance, batch.out.ctypes.data_as(_dp),
                                                  batch.iterations.ctypes.data_as(_intp))
        self.last_status = rc if rc >= 0 else _check(rc)
        return batch.out

    def ComputeRobotMotionConcurrent(self, others, batch, voxel_map, max_correspondence_distance):
        """kicp_register_device_concurrent: the batch's INDEPENDENT scans with 1 + len(others) of them in flight, one lane per
        handle (this one and `others`).  Same poses as ComputeRobotMotionBatch, bit for bit."""
        handles = (C.c_void_p * (1 + len(others)))(self._h, *[o._h for o in others])
        rc = self._lib.kicp_register_device_concurrent(handles, len(handles), voxel_map._h, batch.count, batch.ptrs, batch.ns,
                                                       batch.last.ctypes.data_as(_dp), batch.rel.ctypes.data_as(_dp), max_correspondence_distance,
                                                       batch.out.ctypes.data_as(_dp), batch.iterations.ctypes.data_as(_intp))
        self.last_status = rc if rc >= 0 else _check(rc)
        return batch.out

    def pass_sums(self, frame, voxel_map, pose, max_correspondence_distance):
        """One fused association+accumulation pass at a fixed pose -> [JTJ00,JTJ01,JTJ11,JTr0,JTr1,ssq,N]."""
        a, p = _d(frame)
        _, q = _d(pose)
        out = np.zeros(7, dtype=np.float64)
        _check(lib().kicp_pass_sums(self._h, voxel_map._h, p, a.size // 3, q, max_correspondence_distance, out.ctypes.data_as(_dp)))
        return out

    def pass_correspondences(self, frame, voxel_map, pose, max_correspondence_distance):
        """kicp_pass_correspondences: DataAssociation's output per source point from the pass kernel this handle registers a scan of this
        size with -> (index[n] int32, -1 = none; d2[n]; nn[n, 3])."""
        a, p = _d(frame)
        _, q = _d(pose)
        n = a.size // 3
        idx = np.empty(n, dtype=np.int32)
        d2 = np.empty(n, dtype=np.float64)
        nn = np.empty((n, 3), dtype=np.float64)
        _check(lib().kicp_pass_correspondences(self._h, voxel_map._h, p, n, q, max_correspondence_distance, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                               d2.ctypes.data_as(_dp), nn.ctypes.data_as(_dp)))
        return idx, d2, nn

    def ScorePoses(self, frame, voxel_map, poses, max_correspondence_distance):
        """kicp_score_poses: DataAssociation of ONE frame ((N,3) host array or DeviceFrame) at every pose of `poses` (count, 7) in one call
        -> (n_corr[count], ssr[count]): pass_sums(...)[6] and [5] at each pose, bit for bit."""
        q = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 7))
        count = q.shape[0]
        n_corr, ssr = np.zeros(count, dtype=np.float64), np.zeros(count, dtype=np.float64)
        if isinstance(frame, DeviceFrame):
            _check(lib().kicp_score_poses_device(self._h, voxel_map._h, frame.ptr, frame.n, q.ctypes.data_as(_dp), count, max_correspondence_distance,
                                                 n_corr.ctypes.data_as(_dp), ssr.ctypes.data_as(_dp)))
        else:
            a, p = _d(frame)
            _check(lib().kicp_score_poses(self._h, voxel_map._h, p, a.size // 3, q.ctypes.data_as(_dp), count, max_correspondence_distance,
                                          n_corr.ctypes.data_as(_dp), ssr.ctypes.data_as(_dp)))
        return n_corr, ssr

    def Relocalize(self, frame, voxel_map, candidates, max_correspondence_distance, top_m=8):
        """kicp_relocalize: score the candidate poses (count, 7), refine the top_m cheapest as independent registrations, score again ->
        (pose[7], candidate index, cost before, cost after); cost = (ssr + (n - n_corr) tau^2) / n.  last_status is
        KICP_WARN_NO_CORRESPONDENCES when no refinement kept a correspondence (the cheapest unrefined candidate is returned then).  The
        refinement moves along the kinematic model only: the candidates' lateral spacing is the caller's accuracy."""
        a, p = _d(frame)
        q = np.ascontiguousarray(np.asarray(candidates, dtype=np.float64).reshape(-1, 7))
        pose = np.zeros(7, dtype=np.float64)
        cand, before, after = C.c_size_t(), C.c_double(), C.c_double()
        rc = lib().kicp_relocalize(self._h, voxel_map._h, p, a.size // 3, q.ctypes.data_as(_dp), q.shape[0], max_correspondence_distance, int(top_m),
                                   pose.ctypes.data_as(_dp), C.byref(cand), C.byref(before), C.byref(after))
        self.last_status = rc if rc >= 0 else _check(rc)
        return pose, cand.value, before.value, after.value

    def PlanarSums(self, frame, voxel_map, poses, max_correspondence_distance):
        """kicp_planar_sums: the sums of one planar 3-DoF Gauss-Newton step of ONE frame ((N,3) host array or DeviceFrame) at every pose of
        `poses` (count, 7) -> (count, 8): N, S_x, S_y, S_ss, S_a, S_b, S_c, ssr (include/kicp.h)."""
        q = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 7))
        count = q.shape[0]
        sums = np.zeros((count, 8), dtype=np.float64)
        if isinstance(frame, DeviceFrame):
            _check(lib().kicp_planar_sums_device(self._h, voxel_map._h, frame.ptr, frame.n, q.ctypes.data_as(_dp), count, max_correspondence_distance,
                                                 sums.ctypes.data_as(_dp)))
        else:
            a, p = _d(frame)
            _check(lib().kicp_planar_sums(self._h, voxel_map._h, p, a.size // 3, q.ctypes.data_as(_dp), count, max_correspondence_distance,
                                          sums.ctypes.data_as(_dp)))
        return sums

    def RefinePosesPlanar(self, frame, voxel_map, poses, max_correspondence_distance, max_iterations=100, convergence=1e-4):
        """kicp_refine_poses_planar: planar (x, y, yaw) Gauss-Newton refinement of every pose of `poses` (count, 7) against ONE frame
        ((N,3) host array or DeviceFrame), all poses in lock step -> (poses[count, 7], iterations[count], status[count]); status 0:
        converged, 1: max_iterations steps applied, 2: degenerate (the pose as it stood)."""
        q = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 7))
        count = q.shape[0]
        out = np.zeros((count, 7), dtype=np.float64)
        iterations, status = np.zeros(count, dtype=np.int32), np.zeros(count, dtype=np.int32)
        tail = (q.ctypes.data_as(_dp), count, max_correspondence_distance, int(max_iterations), float(convergence), out.ctypes.data_as(_dp),
                iterations.ctypes.data_as(_intp), status.ctypes.data_as(_intp))
        if isinstance(frame, DeviceFrame):
            _check(lib().kicp_refine_poses_planar_device(self._h, voxel_map._h, frame.ptr, frame.n, *tail))
        else:
            a, p = _d(frame)
            _check(lib().kicp_refine_poses_planar(self._h, voxel_map._h, p, a.size // 3, *tail))
        return out, iterations, status

    def RelocalizePlanar(self, frame, voxel_map, candidates, max_correspondence_distance, top_m=8, max_iterations=100, convergence=1e-4):
        """kicp_relocalize_planar: Relocalize with the top_m finalists refined in the plane (RefinePosesPlanar) instead of along the kinematic
        model -> (pose[7], candidate index, cost before, cost after); a candidate's lateral offset is removed too.  Like Relocalize it
        takes a HOST frame (uploaded once inside)."""
        a, p = _d(frame)
        q = np.ascontiguousarray(np.asarray(candidates, dtype=np.float64).reshape(-1, 7))
        pose = np.zeros(7, dtype=np.float64)
        cand, before, after = C.c_size_t(), C.c_double(), C.c_double()
        rc = lib().kicp_relocalize_planar(self._h, voxel_map._h, p, a.size // 3, q.ctypes.data_as(_dp), q.shape[0], max_correspondence_distance, int(top_m),
                                          int(max_iterations), float(convergence), pose.ctypes.data_as(_dp), C.byref(cand), C.byref(before), C.byref(after))
        self.last_status = rc if rc >= 0 else _check(rc)
        return pose, cand.value, before.value, after.value

    def ScoreNodes(self, frame, occ, window, level, nodes):
        """kicp_occ_score_nodes: per node index of `nodes` the number of frame points whose cell - at the node's yaw, shifted by the node's
        (ix, iy) - is set in level `level` of the pyramid -> uint32[count]; exact integers"""
        a, p = _d(frame)
        q = np.ascontiguousarray(np.asarray(nodes, dtype=np.uint64).reshape(-1))
        hits = np.zeros(q.size, dtype=np.uint32)
        _check(lib().kicp_occ_score_nodes(self._h, occ._h, p, a.size // 3, C.byref(window), int(level), _u64(q), q.size, _u32(hits)))
        return hits

    def SearchPoses(self, frame, occ, window, top_m=8):
        """kicp_search_poses: the first min(top_m, all) nodes of the window by (level-0 score descending, node index ascending), found by
        branch and bound over the pyramid -> (nodes uint64[k], hits uint32[k], poses[k, 7]).  Option "search_max_nodes" bounds the work
        (KicpError with KICP_ERR_CAPACITY beyond it); "search_nodes_scored" / "search_launches" describe the last call."""
        a, p = _d(frame)
        k = min(int(top_m), window.nodes)
        nodes, hits, poses = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint32), np.zeros((k, 7), dtype=np.float64)
        found = C.c_size_t()
        _check(lib().kicp_search_poses(self._h, occ._h, p, a.size // 3, C.byref(window), int(top_m), _u64(nodes), _u32(hits), poses.ctypes.data_as(_dp),
                                       C.byref(found)))
        return nodes[:found.value], hits[:found.value], poses[:found.value]

    def RelocalizeSearch(self, frame, voxel_map, occ, window, max_correspondence_distance, top_m=8, max_iterations=100, convergence=1e-4):
        """kicp_relocalize_search: SearchPoses over the whole window, then RelocalizePlanar with the found poses as candidates and every one
        of them a finalist -> (pose[7], node index, cost before, cost after).  `occ` must be a pyramid of `voxel_map`."""
        a, p = _d(frame)
        pose = np.zeros(7, dtype=np.float64)
        node, before, after = C.c_ulonglong(), C.c_double(), C.c_double()
        rc = lib().kicp_relocalize_search(self._h, voxel_map._h, occ._h, p, a.size // 3, C.byref(window), max_correspondence_distance, int(top_m),
                                          int(max_iterations), float(convergence), pose.ctypes.data_as(_dp), C.byref(node), C.byref(before), C.byref(after))
        self.last_status = rc if rc >= 0 else _check(rc)
        return pose, node.value, before.value, after.value

    def pass_words(self, frame, voxel_map, pose, max_correspondence_distance):
        """The same pass as raw int64[24] limb words (the multi-GPU all-reduce payload; see sharding.py)."""
        a, p = _d(frame)
        _, q = _d(pose)
        out = np.zeros(24, dtype=np.int64)
        _check(lib().kicp_pass_words(self._h, voxel_map._h, p, a.size // 3, q, max_correspondence_distance,
                                     out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    # ---- multi-GPU ----
    def comm_init(self, nranks, rank, unique_id):
        _check(lib().kicp_reg_comm_init(self._h, nranks, rank, unique_id))

    def comm_destroy(self):
        _check(lib().kicp_reg_comm_destroy(self._h))

    def shm_init(self, nranks, rank, name):
        """Single-node multi-process mode without a device collective (see kicp.h); rank 0 first, then the others."""
        _check(lib().kicp_reg_shm_init(self._h, nranks, rank, name.encode()))

    def shm_destroy(self):
        _check(lib().kicp_reg_shm_destroy(self._h))

    def p2p_export(self, nranks, rank):
        """Peer-mailbox exchange (kicp.h): allocate this rank's mailbox, return its IPC handle (bytes) for the all-gather."""
        buf = C.create_string_buffer(P2P_HANDLE_BYTES)
        _check(lib().kicp_reg_p2p_export(self._h, nranks, rank, buf))
        return buf.raw

    def p2p_connect(self, handles):
        """handles: every rank's handle in rank order (list of bytes, or their concatenation)."""
        blob = handles if isinstance(handles, (bytes, bytearray)) else b"".join(handles)
        _check(lib().kicp_reg_p2p_connect(self._h, bytes(blob)))

    def p2p_destroy(self):
        _check(lib().kicp_reg_p2p_destroy(self._h))

    def set_allreduce(self, fn):
        """fn(device_ptr:int, count:int, stream:int) -> None: sum-all-reduce `count` doubles in place on `stream`."""
        if fn is None:
            self._cb = None
            _check(lib().kicp_reg_set_allreduce(self._h, C.cast(None, ALLREDUCE_FN), None))
            return

        def tramp(user, buf, count, stream):
            try:
                fn(buf or 0, count, stream or 0)
                return 0
            except Exception:  # noqa: BLE001 - must not unwind through C
                import traceback
                traceback.print_exc()
                return 1

        self._cb = ALLREDUCE_FN(tramp)
        _check(lib().kicp_reg_set_allreduce(self._h, self._cb, None))
