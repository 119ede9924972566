"""kinematic_icp_amd -- MI355X-native backend of the kinematic-ICP registration hot path.

Python mirror of the reference's operator interface for this path, bound with ctypes to the C-ABI of
include/kicp.h (libkicp_amd.so, hand-written HIP for gfx950):

    kinematic_icp::KinematicRegistration   /root/reference/cpp/kinematic_icp/registration/Registration.hpp:32-50
    kiss_icp::VoxelHashMap (v1.2.0)        call sites Registration.cpp:63,74,157; KinematicICP.hpp:79,88,92; KinematicICP.cpp:79

Names, argument order and argument meaning follow the reference.  Poses are 7-vectors
[qx, qy, qz, qw, tx, ty, tz] (Sophus::SE3d parameter order); point clouds are (N, 3) float64 arrays.

There is NO CPU fallback: importing works anywhere, but creating a KinematicRegistration (or running any
device operation) without the built extension or without a visible gfx950 device raises KicpError.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkicp_amd.so")
MAX_LOG_PASSES = 32
P2P_HANDLE_BYTES = 64
COMM_ID_BYTES = 128

KICP_OK = 0
KICP_WARN_NO_CORRESPONDENCES = 1
KICP_WARN_TABLE_ORDER = 2
KICP_ERR_HIP, KICP_ERR_ARG, KICP_ERR_CAPACITY, KICP_ERR_COMM, KICP_ERR_INTERNAL = -1, -2, -3, -4, -5


class KicpError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("kicp error %d: %s" % (code, message))
        self.code = code


class RegConfig(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("convergence_criterion", C.c_double), ("max_num_threads", C.c_int32),
                ("use_adaptive_odometry_regularization", C.c_int32), ("fixed_regularization", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("empty_map", C.c_int32), ("reserved", C.c_int32),
                ("beta", C.c_double), ("n_corr", C.c_double * MAX_LOG_PASSES), ("sums", (C.c_double * 6) * MAX_LOG_PASSES),
                ("dx", (C.c_double * 2) * MAX_LOG_PASSES), ("gpu_ms", C.c_double), ("pass_ms", C.c_double * MAX_LOG_PASSES)]


class SearchWindow(C.Structure):
    """kicp_search_window: node (j, ix, iy) is the planar pose at (x0 + ix cell, y0 + iy cell, z) with yaw yaw0 + j yaw_step; its index
    is (j * ny + iy) * nx + ix"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("z", C.c_double), ("nx", C.c_uint), ("ny", C.c_uint), ("yaw0", C.c_double),
                ("yaw_step", C.c_double), ("nyaw", C.c_uint)]

    @property
    def nodes(self):
        return int(self.nx) * int(self.ny) * int(self.nyaw)


class GridConfig(C.Structure):
    """kicp_grid_config: width x height cells of side `cell` from (origin_x, origin_y); points with z_min <= z < z_max (base frame) whose
    cell lies within ceil(max_ray / cell) cells of the sensor's count"""
    _fields_ = [("cell", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double), ("width", C.c_uint), ("height", C.c_uint),
                ("z_min", C.c_double), ("z_max", C.c_double), ("max_ray", C.c_double)]


class GridClearanceConfig(C.Structure):
    """kicp_grid_clearance_config: the readout's min_observations, the threshold above which a cell is a source, whether unknown cells
    are sources too, and the radius R in cells (1 .. 254)"""
    _fields_ = [("min_observations", C.c_uint), ("occupied_thresh", C.c_double), ("unknown_is_obstacle", C.c_int), ("radius_cells", C.c_int)]


class PlanConfig(C.Structure):
    """kicp_plan_config: potentials are clamped at max_potential (1 .. 0xFFFFFFFE), which doubles as a planning horizon"""
    _fields_ = [("max_potential", C.c_uint)]


class FrontierConfig(C.Structure):
    """kicp_frontier_config: the readout's min_observations, the threshold above which a cell is occupied, and the least size in cells
    of a frontier that is output"""
    _fields_ = [("min_observations", C.c_uint), ("occupied_thresh", C.c_double), ("min_size", C.c_uint)]


class GainConfig(C.Structure):
    """kicp_gain_config: the readout's min_observations, the threshold above which a cell is occupied, and the sensor's range R in cells
    (1 .. 361)"""
    _fields_ = [("min_observations", C.c_uint), ("occupied_thresh", C.c_double), ("range_cells", C.c_uint)]


class ElevationConfig(C.Structure):
    """kicp_elev_config: the grid's geometry - width x height cells of side `cell` from (origin_x, origin_y), max_ray - and a vertical
    one: bit b of a cell's 64-bit column is the world heights [z_origin + b slab, z_origin + (b + 1) slab)"""
    _fields_ = [("cell", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double), ("width", C.c_uint), ("height", C.c_uint),
                ("z_origin", C.c_double), ("slab", C.c_double), ("max_ray", C.c_double)]


class ElevationTraversabilityConfig(C.Structure):
    """kicp_elev_traversability_config: the highest step the robot takes (0 .. 62) and its height (step_slabs < robot_slabs <= 64), in slabs"""
    _fields_ = [("step_slabs", C.c_uint), ("robot_slabs", C.c_uint)]


class ElevationCarveConfig(C.Structure):
    """kicp_elev_carve_config: the last margin_steps steps of every ray before its endpoint cell are not carved, each step's span of slabs
    is widened by widen_slabs (0 .. 64) on both sides, and with keep_ground (0 or 1) the lowest set bit of a column is never cleared"""
    _fields_ = [("margin_steps", C.c_uint), ("widen_slabs", C.c_uint), ("keep_ground", C.c_uint)]


class ElevationSlopeConfig(C.Structure):
    """kicp_elev_slope_config: the plane fit of the slope limit - a window of radius_cells (1 .. 8) around each cell, of which the cells
    count whose ground differs from the cell's by at most gate_slabs (0 .. 63); at least min_cells (3 .. 289) of them; the limit is
    rise_slabs (0 .. 65535) slabs of height per run_cells (1 .. 65535) cells of distance"""
    _fields_ = [("radius_cells", C.c_uint), ("gate_slabs", C.c_uint), ("min_cells", C.c_uint), ("rise_slabs", C.c_uint), ("run_cells", C.c_uint)]


class ElevationRoughConfig(C.Structure):
    """kicp_elev_rough_config: the class ROUGH of the slope limit's plane fit - a cell with a fit is ROUGH when the mean squared residual
    of its fit set to the fitted plane exceeds num (0 .. 65535) / den (1 .. 65535) slabs^2"""
    _fields_ = [("num", C.c_uint), ("den", C.c_uint)]


class GridFillConfig(C.Structure):
    """kicp_grid_fill_config: how OccupancyGrid.fill_unknown reads its source - the readout at min_observations (>= 1) is FREE at
    0 .. free_max (<= 100), OCCUPIED from occupied_min (free_max < occupied_min <= 101; 101: never) and otherwise says nothing"""
    _fields_ = [("min_observations", C.c_uint), ("free_max", C.c_uint), ("occupied_min", C.c_uint)]


class ViewConfig(C.Structure):
    """kicp_view_config: a cube map of res x res pixels per face; the verdict looks at (2 window + 1)^2 pixels, needs min_rays returns
    among them and a gap of more than margin + margin_per_metre * depth; max_ray bounds the (Chebyshev) depth on both sides"""
    _fields_ = [("res", C.c_uint), ("window", C.c_int), ("min_rays", C.c_uint), ("max_ray", C.c_double), ("margin", C.c_double),
                ("margin_per_metre", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)

_dp = C.POINTER(C.c_double)
_lib = None

# every symbol include/kicp.h declares: (restype, argtypes)
_SIGNATURES = {
    "kicp_last_error": (C.c_char_p, []),
    "kicp_version": (C.c_int, []),
    "kicp_device_count": (C.c_int, []),
    "kicp_device_locality": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "kicp_map_create": (C.c_int, [C.c_double, C.c_double, C.c_uint, C.POINTER(C.c_void_p)]),
    "kicp_map_destroy": (None, [C.c_void_p]),
    "kicp_map_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "kicp_map_clear": (C.c_int, [C.c_void_p]),
    "kicp_map_empty": (C.c_int, [C.c_void_p]),
    "kicp_map_add_points": (C.c_int, [C.c_void_p, _dp, C.c_size_t]),
    "kicp_map_remove_far": (C.c_int, [C.c_void_p, _dp]),
    "kicp_map_update_origin": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp]),
    "kicp_map_update_pose": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp]),
    "kicp_map_update_pose_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, _dp]),
    "kicp_map_update_pose_device_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, _dp]),
    "kicp_map_update_finish": (C.c_int, [C.c_void_p]),
    "kicp_map_last_update_on_device": (C.c_int, [C.c_void_p]),
    "kicp_map_device_updates": (C.c_ulonglong, [C.c_void_p]),
    "kicp_map_update_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "kicp_map_set_device": (C.c_int, [C.c_void_p, C.c_int]),
    "kicp_map_num_points": (C.c_size_t, [C.c_void_p]),
    "kicp_map_num_voxels": (C.c_size_t, [C.c_void_p]),
    "kicp_map_pointcloud": (C.c_size_t, [C.c_void_p, _dp, C.c_size_t]),
    "kicp_map_pointcloud_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_map_closest": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, _dp, _dp]),
    "kicp_map_check": (C.c_size_t, [C.c_void_p]),
    "kicp_map_sync": (C.c_int, [C.c_void_p, C.c_int]),
    "kicp_map_last_upload": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "kicp_view_create": (C.c_int, [C.POINTER(ViewConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "kicp_view_destroy": (None, [C.c_void_p]),
    "kicp_view_info": (C.c_int, [C.c_void_p, C.POINTER(ViewConfig), _dp, C.POINTER(C.c_ulonglong)]),
    "kicp_view_render": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp, _dp, C.POINTER(C.c_ulonglong)]),
    "kicp_view_render_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _dp, _dp, C.POINTER(C.c_ulonglong)]),
    "kicp_view_depth": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_size_t]),
    "kicp_view_classify": (C.c_int, [C.c_void_p, _dp, C.c_size_t, C.POINTER(C.c_ubyte)]),
    "kicp_map_remove_seen_through": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "kicp_reg_create": (C.c_int, [C.POINTER(RegConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "kicp_reg_destroy": (None, [C.c_void_p]),
    "kicp_reg_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "kicp_reg_get_config": (C.c_int, [C.c_void_p, C.POINTER(RegConfig)]),
    "kicp_reg_set_config": (C.c_int, [C.c_void_p, C.POINTER(RegConfig)]),
    "kicp_reg_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "kicp_reg_get_option": (C.c_double, [C.c_void_p, C.c_char_p]),
    "kicp_register": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, _dp, C.c_double, _dp, C.POINTER(Stats)]),
    "kicp_register_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _dp, _dp, C.c_double, _dp, C.POINTER(Stats)]),
    "kicp_register_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _dp, _dp, C.c_double, _dp, C.POINTER(Stats)]),
    "kicp_register_device_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), _dp, _dp,
                                             C.c_double, _dp, C.POINTER(C.c_int)]),
    "kicp_register_device_concurrent": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                  _dp, _dp, C.c_double, _dp, C.POINTER(C.c_int)]),
    "kicp_pass_sums": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, C.c_double, _dp]),
    "kicp_pass_correspondences": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, C.c_double, C.POINTER(C.c_int32), _dp, _dp]),
    "kicp_pass_words": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, C.c_double, C.POINTER(C.c_longlong)]),
    "kicp_score_poses": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, C.c_size_t, C.c_double, _dp, _dp]),
    "kicp_score_poses_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _dp, C.c_size_t, C.c_double, _dp, _dp]),
    "kicp_relocalize": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, C.c_size_t, C.c_double, C.c_size_t, _dp, C.POINTER(C.c_size_t), _dp, _dp]),
    "kicp_planar_sums": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, C.c_size_t, C.c_double, _dp]),
    "kicp_planar_sums_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _dp, C.c_size_t, C.c_double, _dp]),
    "kicp_planar_step": (C.c_int, [_dp, _dp, _dp, _dp]),
    "kicp_refine_poses_planar": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, C.c_size_t, C.c_double, C.c_int, C.c_double, _dp,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kicp_refine_poses_planar_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _dp, C.c_size_t, C.c_double, C.c_int, C.c_double, _dp,
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kicp_relocalize_planar": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, _dp, C.c_size_t, C.c_double, C.c_size_t, C.c_int, C.c_double, _dp,
                                         C.POINTER(C.c_size_t), _dp, _dp]),
    "kicp_occ_build": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "kicp_occ_destroy": (None, [C.c_void_p]),
    "kicp_occ_info": (C.c_int, [C.c_void_p, _dp, C.POINTER(C.c_int), _dp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
    "kicp_occ_level": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_search_yaws": (C.c_int, [C.POINTER(SearchWindow), _dp]),
    "kicp_search_window_around": (C.c_int, [C.c_void_p, _dp, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(SearchWindow)]),
    "kicp_occ_score_nodes": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, C.POINTER(SearchWindow), C.c_int, C.POINTER(C.c_ulonglong), C.c_size_t,
                                       C.POINTER(C.c_uint)]),
    "kicp_search_poses": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_size_t, C.POINTER(SearchWindow), C.c_size_t, C.POINTER(C.c_ulonglong),
                                    C.POINTER(C.c_uint), _dp, C.POINTER(C.c_size_t)]),
    "kicp_relocalize_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_size_t, C.POINTER(SearchWindow), C.c_double, C.c_size_t, C.c_int,
                                         C.c_double, _dp, C.POINTER(C.c_ulonglong), _dp, _dp]),
    "kicp_grid_create": (C.c_int, [C.POINTER(GridConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "kicp_grid_destroy": (None, [C.c_void_p]),
    "kicp_grid_info": (C.c_int, [C.c_void_p, C.POINTER(GridConfig), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
    "kicp_grid_clear": (C.c_int, [C.c_void_p]),
    "kicp_grid_integrate": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp, _dp, C.POINTER(C.c_ulonglong)]),
    "kicp_grid_integrate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _dp, _dp, C.POINTER(C.c_ulonglong)]),
    "kicp_grid_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_ushort), C.c_size_t]),
    "kicp_grid_set_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_ushort), C.c_size_t]),
    "kicp_grid_occupancy": (C.c_int, [C.c_void_p, C.c_uint, C.POINTER(C.c_byte), C.c_size_t]),
    "kicp_grid_occupancy_from_counts": (C.c_int, [C.POINTER(C.c_ushort), C.c_size_t, C.c_uint, C.POINTER(C.c_byte)]),
    "kicp_grid_save_map": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint, C.c_double, C.c_double]),
    "kicp_grid_write_map": (C.c_int, [C.c_char_p, C.POINTER(C.c_byte), C.c_uint, C.c_uint, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "kicp_grid_clearance": (C.c_int, [C.c_void_p, C.POINTER(GridClearanceConfig), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_ushort), C.c_size_t]),
    "kicp_grid_costmap": (C.c_int, [C.c_void_p, C.POINTER(GridClearanceConfig), C.POINTER(C.c_ubyte), C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                    C.POINTER(C.c_ubyte), C.c_size_t]),
    "kicp_grid_clearance_from_occupancy": (C.c_int, [C.POINTER(C.c_byte), C.c_uint, C.c_uint, C.POINTER(GridClearanceConfig), C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                                     C.POINTER(C.c_ushort), C.c_size_t]),
    "kicp_grid_costmap_from_occupancy": (C.c_int, [C.POINTER(C.c_byte), C.c_uint, C.c_uint, C.POINTER(GridClearanceConfig), C.POINTER(C.c_ubyte), C.c_size_t, C.c_int,
                                                   C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_ubyte), C.c_size_t]),
    "kicp_grid_cost_table_nav2": (C.c_int, [C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_ubyte), C.c_size_t]),
    "kicp_grid_last_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "kicp_plan_weights": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_ubyte)]),
    "kicp_potential_from_costmap": (C.c_int, [C.POINTER(C.c_ubyte), C.c_uint, C.c_uint, C.POINTER(C.c_ubyte), C.POINTER(PlanConfig), C.POINTER(C.c_uint), C.c_size_t,
                                              C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_ulonglong)]),
    "kicp_potential_path": (C.c_int, [C.POINTER(C.c_uint), C.POINTER(C.c_ubyte), C.c_uint, C.c_uint, C.POINTER(C.c_ubyte), C.c_uint, C.c_uint, C.POINTER(C.c_uint),
                                      C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_grid_potential_of_costmap": (C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.POINTER(PlanConfig), C.POINTER(C.c_uint), C.c_size_t,
                                                 C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_ulonglong)]),
    "kicp_grid_potential": (C.c_int, [C.c_void_p, C.POINTER(GridClearanceConfig), C.POINTER(C.c_ubyte), C.c_size_t, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(PlanConfig),
                                      C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_ulonglong)]),
    "kicp_plan_q": (C.c_int, [C.POINTER(C.c_ubyte), C.c_size_t, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "kicp_arc_steps": (C.c_int, [_dp, _dp, C.c_double, C.c_size_t, _dp]),
    "kicp_footprint_box": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_arcs_best": (C.c_int, [C.POINTER(C.c_uint), C.c_size_t, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_size_t)]),
    "kicp_score_arcs_from_plan": (C.c_int, [C.POINTER(C.c_ubyte), C.POINTER(C.c_uint), C.c_double, C.c_double, C.c_double, C.c_uint, C.c_uint, _dp, _dp, C.c_size_t, C.c_uint,
                                            _dp, C.c_size_t, C.POINTER(C.c_uint), C.c_size_t]),
    "kicp_grid_has_plan": (C.c_int, [C.c_void_p]),
    "kicp_grid_score_arcs": (C.c_int, [C.c_void_p, _dp, _dp, C.c_size_t, C.c_uint, _dp, C.c_size_t, C.POINTER(C.c_uint), C.c_size_t]),
    "kicp_arc_tree_nodes": (C.c_int, [C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_uint),
                                      C.POINTER(C.c_size_t)]),
    "kicp_arc_tree_best": (C.c_int, [C.POINTER(C.c_uint), C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_uint)]),
    "kicp_score_arc_tree_from_plan": (C.c_int, [C.POINTER(C.c_ubyte), C.POINTER(C.c_uint), C.c_double, C.c_double, C.c_double, C.c_uint, C.c_uint, _dp, C.c_uint,
                                                C.POINTER(C.c_uint), C.POINTER(C.c_uint), _dp, _dp, C.c_size_t, C.POINTER(C.c_uint), C.c_size_t]),
    "kicp_grid_score_arc_tree": (C.c_int, [C.c_void_p, _dp, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint), _dp, _dp, C.c_size_t, C.POINTER(C.c_uint), C.c_size_t]),
    "kicp_frontiers_from_occupancy": (C.c_int, [C.POINTER(C.c_byte), C.c_uint, C.c_uint, C.POINTER(FrontierConfig), C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong), C.c_size_t,
                                                C.POINTER(C.c_size_t), C.POINTER(C.c_uint), C.c_size_t]),
    "kicp_grid_frontiers": (C.c_int, [C.c_void_p, C.POINTER(FrontierConfig), C.c_int, C.POINTER(C.c_ulonglong), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint),
                                      C.c_size_t]),
    "kicp_gain_from_occupancy": (C.c_int, [C.POINTER(C.c_byte), C.c_uint, C.c_uint, C.POINTER(GainConfig), C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_uint), C.c_size_t]),
    "kicp_grid_gain": (C.c_int, [C.c_void_p, C.POINTER(GainConfig), C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_uint), C.c_size_t]),
    "kicp_elev_create": (C.c_int, [C.POINTER(ElevationConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "kicp_elev_destroy": (None, [C.c_void_p]),
    "kicp_elev_info": (C.c_int, [C.c_void_p, C.POINTER(ElevationConfig), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
    "kicp_elev_clear": (C.c_int, [C.c_void_p]),
    "kicp_elev_integrate": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp, _dp, C.POINTER(C.c_ulonglong)]),
    "kicp_elev_integrate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _dp, _dp, C.POINTER(C.c_ulonglong)]),
    "kicp_elev_update": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp, _dp, C.POINTER(ElevationCarveConfig), C.POINTER(C.c_ulonglong)]),
    "kicp_elev_update_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _dp, _dp, C.POINTER(ElevationCarveConfig), C.POINTER(C.c_ulonglong)]),
    "kicp_elev_update_columns": (C.c_int, [C.POINTER(ElevationConfig), C.POINTER(C.c_ulonglong), C.c_size_t, _dp, C.c_size_t, _dp, _dp, C.POINTER(ElevationCarveConfig),
                                           C.POINTER(C.c_ulonglong)]),
    "kicp_elev_columns": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_size_t]),
    "kicp_elev_set_columns": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_size_t]),
    "kicp_elev_last_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "kicp_elev_traversability": (C.c_int, [C.c_void_p, C.POINTER(ElevationTraversabilityConfig), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_byte),
                                           C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong), C.c_size_t]),
    "kicp_elev_traversability_from_columns": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_uint, C.c_uint, C.POINTER(ElevationTraversabilityConfig), C.c_uint, C.c_uint, C.c_uint,
                                                        C.c_uint, C.POINTER(C.c_byte), C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong), C.c_size_t]),
    "kicp_elev_to_grid": (C.c_int, [C.c_void_p, C.POINTER(ElevationTraversabilityConfig), C.c_void_p]),
    "kicp_elev_traversability_slope": (C.c_int, [C.c_void_p, C.POINTER(ElevationTraversabilityConfig), C.POINTER(ElevationSlopeConfig), C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                                 C.POINTER(C.c_byte), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong), C.c_size_t]),
    "kicp_elev_traversability_slope_from_columns": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_uint, C.c_uint, C.POINTER(ElevationTraversabilityConfig),
                                                              C.POINTER(ElevationSlopeConfig), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_byte), C.POINTER(C.c_ubyte),
                                                              C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong), C.c_size_t]),
    "kicp_elev_to_grid_slope": (C.c_int, [C.c_void_p, C.POINTER(ElevationTraversabilityConfig), C.POINTER(ElevationSlopeConfig), C.c_void_p]),
    "kicp_elev_slope_limit": (C.c_int, [C.POINTER(ElevationConfig), C.c_double, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "kicp_elev_traversability_rough": (C.c_int, [C.c_void_p, C.POINTER(ElevationTraversabilityConfig), C.POINTER(ElevationSlopeConfig), C.POINTER(ElevationRoughConfig),
                                                 C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_byte), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong),
                                                 C.POINTER(C.c_ulonglong), C.c_size_t]),
    "kicp_elev_traversability_rough_from_columns": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_uint, C.c_uint, C.POINTER(ElevationTraversabilityConfig),
                                                              C.POINTER(ElevationSlopeConfig), C.POINTER(ElevationRoughConfig), C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                                              C.POINTER(C.c_byte), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong), C.c_size_t]),
    "kicp_elev_to_grid_rough": (C.c_int, [C.c_void_p, C.POINTER(ElevationTraversabilityConfig), C.POINTER(ElevationSlopeConfig), C.POINTER(ElevationRoughConfig), C.c_void_p]),
    "kicp_elev_rough_limit": (C.c_int, [C.POINTER(ElevationConfig), C.c_double, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "kicp_grid_fill_unknown": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GridFillConfig), C.POINTER(C.c_ulonglong)]),
    "kicp_grid_fill_unknown_counts": (C.c_int, [C.POINTER(C.c_ushort), C.POINTER(C.c_ushort), C.c_size_t, C.POINTER(GridFillConfig), C.POINTER(C.c_ulonglong)]),
    "kicp_planar_grid": (C.c_size_t,[_dp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _dp, C.c_size_t]),
    "kicp_map_save_pcd": (C.c_int, [C.c_void_p, C.c_char_p]),
    "kicp_map_load_pcd": (C.c_int, [C.c_char_p, C.c_double, C.c_double, C.c_uint, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "kicp_map_params": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(C.c_uint)]),
    "kicp_pre_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "kicp_pre_destroy": (None, [C.c_void_p]),
    "kicp_pre_preprocess": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp, C.c_size_t, _dp, _dp, C.c_double, C.c_double, C.c_int, C.c_int,
                                      C.POINTER(C.c_size_t)]),
    "kicp_pre_ingest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, _dp, _dp, _dp]),
    "kicp_pre_ingest_ahead": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, _dp]),
    "kicp_pre_ingest_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_double, _dp, _dp]),
    "kicp_pre_ahead_hits": (C.c_ulonglong, [C.c_void_p]),
    "kicp_pre_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "kicp_pre_get_option": (C.c_double, [C.c_void_p, C.c_char_p]),
    "kicp_pre_preprocess_ingested": (C.c_int, [C.c_void_p, _dp, _dp, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "kicp_pre_ingested": (C.c_int, [C.c_void_p, _dp, _dp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "kicp_pre_frame": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp, C.c_size_t, _dp, _dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, _dp, C.c_size_t,
                                 C.POINTER(C.c_size_t)]),
    "kicp_pre_frame_ingested": (C.c_int, [C.c_void_p, _dp, _dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_pre_frame_f32": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp, C.c_size_t, _dp, _dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                     C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_pre_frame_ingested_f32": (C.c_int, [C.c_void_p, _dp, _dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_size_t,
                                              C.POINTER(C.c_size_t)]),
    "kicp_pre_ingested_count": (C.c_size_t, [C.c_void_p]),
    "kicp_pre_voxel_downsample": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_size_t)]),
    "kicp_pre_last_max_probe": (C.c_uint, [C.c_void_p]),
    "kicp_pre_set_probe_limit": (C.c_int, [C.c_void_p, C.c_uint]),
    "kicp_pre_upload": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t]),
    "kicp_pre_download": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_pre_download_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_pre_download_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "kicp_pre_download_begin_into": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t]),
    "kicp_pre_download_finish": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kicp_pre_device_ptr": (C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "kicp_device_malloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]),
    "kicp_device_free": (C.c_int, [C.c_int, C.c_void_p]),
    "kicp_device_upload": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "kicp_device_synchronize": (C.c_int, [C.c_int]),
    "kicp_comm_unique_id": (C.c_int, [C.c_char_p]),
    "kicp_reg_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p]),
    "kicp_reg_comm_destroy": (C.c_int, [C.c_void_p]),
    "kicp_reg_shm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p]),
    "kicp_reg_shm_destroy": (C.c_int, [C.c_void_p]),
    "kicp_reg_p2p_export": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p]),
    "kicp_reg_p2p_connect": (C.c_int, [C.c_void_p, C.c_char_p]),
    "kicp_reg_p2p_destroy": (C.c_int, [C.c_void_p]),
    "kicp_reg_set_allreduce": (C.c_int, [C.c_void_p, ALLREDUCE_FN, C.c_void_p]),
    "kicp_aql_kernel_names": (C.c_size_t, [C.c_char_p, C.c_size_t]),
    "kicp_probe_dependent_load": (C.c_int, [C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "kicp_map_device_bytes": (C.c_size_t, [C.c_void_p]),
}


def lib():
    """Load libkicp_amd.so (once).  Fails loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KicpError(KICP_ERR_HIP, "HIP extension %s not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                                          "or `make -C kinematic_icp_amd/csrc`); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise KicpError(rc, lib().kicp_last_error().decode(errors="replace"))
    return rc


def _d(a):
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
        a = np.ascontiguousarray(a, dtype=np.float64)
    return a, C.cast(a.ctypes.data, _dp)


# Small arrays that come back call after call (poses): their ctypes pointer is built once.  The cache holds a reference
# to the array, so its address - and the id() used as the key - stays valid; it is only used for arrays of at most 16
# doubles and is bounded.
_PTR_CACHE = {}


def _pose_ptr(a):
    hit = _PTR_CACHE.get(id(a))
    if hit is not None and hit[0] is a:
        return hit[1]
    arr, ptr = _d(a)
    if arr is a and arr.size <= 16:
        if len(_PTR_CACHE) >= 256:
            _PTR_CACHE.clear()
        _PTR_CACHE[id(a)] = (a, ptr)
    elif arr is not a:
        ptr._keep = arr  # a converted temporary must outlive the call
    return ptr


def probe_dependent_load(working_set_bytes, workgroups=512, block=256, steps=64, device=0):
    """ns per dependent load step of `workgroups` x `block` lanes walking a random chain through `working_set_bytes` (kicp.h)"""
    out = C.c_double(0.0)
    _check(lib().kicp_probe_dependent_load(device, int(working_set_bytes), workgroups, block, steps, C.byref(out)))
    return out.value


def device_count():
    return lib().kicp_device_count()


def device_locality(device=0):
    """(NUMA node the GPU is attached to | -1, its CPUs as a set | empty) - kicp_device_locality"""
    node, buf = C.c_int(-1), C.create_string_buffer(4096)
    _check(lib().kicp_device_locality(device, C.byref(node), buf, len(buf)))
    cpus = set()
    for part in buf.value.decode().split(","):
        if part.strip():
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
    return node.value, cpus


def cpus_near_gpu(device=0, one_l3_domain=True):
    """CPUs to bind a process that drives `device` to: the GPU's NUMA node, narrowed to what the process may use and (by default) to
    ONE L3 domain of it - the calling thread and the library's helper threads then share a last-level cache.  Empty: unknown."""
    import os
    _, cpus = device_locality(device)
    cpus &= os.sched_getaffinity(0)
    if not cpus or not one_l3_domain:
        return cpus
    try:
        with open("/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list" % min(cpus)) as f:
            l3 = set()
            for part in f.read().strip().split(","):
                lo, _, hi = part.partition("-")
                l3.update(range(int(lo), int(hi or lo) + 1))
        return (cpus & l3) or cpus
    except OSError:
        return cpus


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


def search_yaws(window):
    """kicp_search_yaws: the (nyaw, 2) table of (cos, sin) the node scores are computed from - the very doubles the device uses"""
    out = np.zeros((window.nyaw, 2), dtype=np.float64)
    _check(lib().kicp_search_yaws(C.byref(window), out.ctypes.data_as(_dp)))
    return out


def search_window_around(occ, center_xy, half_x, half_y, z, yaw_step):
    """kicp_search_window_around: the window of nodes within the half extents of center_xy (rounded down to whole cells of the pyramid)
    over the full circle of yaws; half extents <= 0 (center_xy may be None): the pyramid's whole x-y footprint -> SearchWindow"""
    w = SearchWindow()
    center, c = (None, None) if center_xy is None else _d(np.asarray(center_xy, dtype=np.float64).reshape(2))  # (`center` keeps the array alive)
    _check(lib().kicp_search_window_around(occ._h, c, float(half_x), float(half_y), float(z), float(yaw_step), C.byref(w)))
    return w


class OccupancyPyramid:
    """kicp_occ: a SNAPSHOT of a map as an occupancy grid of `cell` metres (every point's cell and those within `dilate` of it) and
    `levels` max-pooled levels above it (include/kicp.h).  It owns its device memory and does not follow later updates of the map."""

    def __init__(self, voxel_map, cell, dilate=1, levels=4, device=0):
        h = C.c_void_p()
        self._h = None
        _check(lib().kicp_occ_build(voxel_map._h, int(device), float(cell), int(dilate), int(levels), C.byref(h)))
        self._h, self.device = h, device

    @classmethod
    def build(cls, voxel_map, cell, dilate=1, levels=4, device=0):
        """kicp_occ_build, spelled as the C-ABI spells it: the same as calling the class"""
        return cls(voxel_map, cell, dilate, levels, device)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.kicp_occ_destroy(self._h)
            self._h = None

    def info(self):
        """-> dict: min[3], dims[3], cell, dilate, levels, set_cells (level 0)"""
        mn, dims = np.zeros(3, dtype=np.float64), (C.c_int * 3)()
        cell, dilate, levels, set_cells = C.c_double(), C.c_int(), C.c_int(), C.c_ulonglong()
        _check(lib().kicp_occ_info(self._h, mn.ctypes.data_as(_dp), dims, C.byref(cell), C.byref(dilate), C.byref(levels), C.byref(set_cells)))
        return {"min": mn, "dims": np.array(list(dims), dtype=np.int64), "cell": cell.value, "dilate": dilate.value, "levels": levels.value,
                "set_cells": set_cells.value}

    def level(self, level):
        """one level as uint32 words shaped (dims z, dims y, words per row): cell (x, y, z) is bit x & 31 of [z, y, x >> 5]"""
        total = C.c_size_t()
        _check(lib().kicp_occ_level(self._h, int(level), None, 0, C.byref(total)))
        words = np.zeros(total.value, dtype=np.uint32)
        _check(lib().kicp_occ_level(self._h, int(level), words.ctypes.data_as(C.POINTER(C.c_uint)), total.value, None))
        dims = self.info()["dims"]
        return words.reshape(int(dims[2]), int(dims[1]), -1)


def occupancy_from_counts(counts, min_observations=1):
    """kicp_grid_occupancy_from_counts: the readout of counters shaped (..., 2) = (hits, misses) on the host -> int8 of the leading shape:
    -1 below min_observations, else (100 hits + (hits + misses) / 2) / (hits + misses) in integers.  Needs no GPU."""
    c = np.ascontiguousarray(counts, dtype=np.uint16)
    if c.ndim < 1 or c.shape[-1] != 2:
        raise KicpError(KICP_ERR_ARG, "counts must be shaped (..., 2): hits, misses")
    out = np.empty(c.shape[:-1], dtype=np.int8)
    _check(lib().kicp_grid_occupancy_from_counts(c.ctypes.data_as(C.POINTER(C.c_ushort)), out.size, int(min_observations),
                                                 out.ctypes.data_as(C.POINTER(C.c_byte))))
    return out


def write_map(prefix, occupancy, cell, origin_x, origin_y, occupied_thresh=0.65, free_thresh=0.25):
    """kicp_grid_write_map: `occupancy` (int8, shaped (height, width), row 0 at the origin) as <prefix>.pgm + <prefix>.yaml, the pair
    map_server and Nav2 read.  Needs no GPU."""
    occ = np.ascontiguousarray(occupancy, dtype=np.int8)
    if occ.ndim != 2:
        raise KicpError(KICP_ERR_ARG, "occupancy must be shaped (height, width)")
    _check(lib().kicp_grid_write_map(os.fsencode(prefix), occ.ctypes.data_as(C.POINTER(C.c_byte)), occ.shape[1], occ.shape[0], float(cell), float(origin_x),
                                     float(origin_y), float(occupied_thresh), float(free_thresh)))


def _clearance_config(radius_cells, min_observations, occupied_thresh, unknown_is_obstacle):
    return GridClearanceConfig(int(min_observations), float(occupied_thresh), 1 if unknown_is_obstacle else 0, int(radius_cells))


def _rect(rect, width, height):
    """(x0, y0, w, h) of `rect`, the full grid for None; negative numbers are passed as something the library refuses"""
    x0, y0, w, h = (0, 0, width, height) if rect is None else (int(v) for v in rect)
    if min(x0, y0, w, h) < 0:
        raise KicpError(KICP_ERR_ARG, "the rectangle (x0, y0, w, h) must not be negative")
    return x0, y0, w, h


def _cost_table(table):
    t = np.ascontiguousarray(table, dtype=np.uint8)
    if t.ndim != 1:
        raise KicpError(KICP_ERR_ARG, "the cost table must be one-dimensional: table[0 .. R^2 + 1]")
    return t


def _occupancy_2d(occupancy):
    occ = np.ascontiguousarray(occupancy, dtype=np.int8)
    if occ.ndim != 2 or occ.size == 0:
        raise KicpError(KICP_ERR_ARG, "occupancy must be shaped (height, width), both at least 1")
    return occ


def clearance_from_occupancy(occupancy, radius_cells, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, rect=None):
    """kicp_grid_clearance_from_occupancy: the squared distance in cells from every cell of `rect` = (x0, y0, w, h) (None: the full grid)
    to the nearest source within radius_cells of it, radius_cells^2 + 1 where there is none, over a readout shaped (height, width) ->
    uint16 (h, w).  Pure host code: needs no GPU."""
    occ = _occupancy_2d(occupancy)
    x0, y0, w, h = _rect(rect, occ.shape[1], occ.shape[0])
    cfg = _clearance_config(radius_cells, min_observations, occupied_thresh, unknown_is_obstacle)
    out = np.empty((h, w), dtype=np.uint16)
    _check(lib().kicp_grid_clearance_from_occupancy(occ.ctypes.data_as(C.POINTER(C.c_byte)), occ.shape[1], occ.shape[0], C.byref(cfg), x0, y0, w, h,
                                                    out.ctypes.data_as(C.POINTER(C.c_ushort)), out.size))
    return out


def costmap_from_occupancy(occupancy, table, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=False, rect=None):
    """kicp_grid_costmap_from_occupancy: Nav2's costs (254 lethal, 253 inscribed, 255 no information, 0 free) of the cells of `rect` from
    `table`[clearance] (length R^2 + 2, which gives R) over a readout shaped (height, width) -> uint8 (h, w).  Pure host code."""
    occ, t = _occupancy_2d(occupancy), _cost_table(table)
    x0, y0, w, h = _rect(rect, occ.shape[1], occ.shape[0])
    cfg = _clearance_config(_table_radius(t), min_observations, occupied_thresh, unknown_is_obstacle)
    out = np.empty((h, w), dtype=np.uint8)
    _check(lib().kicp_grid_costmap_from_occupancy(occ.ctypes.data_as(C.POINTER(C.c_byte)), occ.shape[1], occ.shape[0], C.byref(cfg),
                                                  t.ctypes.data_as(C.POINTER(C.c_ubyte)), t.size, 1 if inflate_unknown else 0, x0, y0, w, h,
                                                  out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size))
    return out


def _table_radius(table):
    """R of a table of R^2 + 2 entries (any other length: KICP_ERR_ARG)"""
    r = math.isqrt(max(int(table.size) - 2, 0))
    if r * r + 2 != table.size:
        raise KicpError(KICP_ERR_ARG, "the cost table must have R^2 + 2 entries, table[0 .. R^2 + 1]")
    return r


def nav2_cost_table(cell, radius_cells, inscribed_radius, cost_scaling_factor):
    """kicp_grid_cost_table_nav2: the table of Nav2's inflation layer for a radius of radius_cells cells of `cell` metres -> uint8
    [radius_cells^2 + 2]: 254 at 0, 253 up to inscribed_radius, 252 exp(-cost_scaling_factor (d - inscribed_radius)) beyond, 0 for far"""
    r = int(radius_cells)
    out = np.empty(r * r + 2 if 1 <= r <= 254 else 2, dtype=np.uint8)
    _check(lib().kicp_grid_cost_table_nav2(float(cell), r, float(inscribed_radius), float(cost_scaling_factor), out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size))
    return out


MAX_POTENTIAL = 0xFFFFFFFE
UNREACHED = 0xFFFFFFFF


def plan_weights(neutral=50, factor_num=4, factor_den=5, lethal_from=253, unknown_weight=0):
    """kicp_plan_weights: weight[256] for the potential, uint8: min(255, neutral + b * factor_num / factor_den) for a cost b < lethal_from,
    0 (impassable) from lethal_from to 254, unknown_weight for 255 (0 keeps the planner out of unknown space).  The defaults are NavFn's."""
    args = [int(v) for v in (neutral, factor_num, factor_den, lethal_from, unknown_weight)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "the arguments of plan_weights are unsigned 32-bit integers")
    out = np.empty(256, dtype=np.uint8)
    _check(lib().kicp_plan_weights(*args, out.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return out


def _plan_args(costmap, weight, goals, max_potential):
    """-> (costmap uint8 (H, W), weight uint8 [256], goals uint32 (n, 2), PlanConfig); what the library cannot be handed is refused here"""
    cm, wt = np.ascontiguousarray(costmap, dtype=np.uint8), np.ascontiguousarray(weight, dtype=np.uint8)
    if cm.ndim != 2 or cm.size == 0:
        raise KicpError(KICP_ERR_ARG, "the costmap must be shaped (height, width), both at least 1")
    if wt.shape != (256,):
        raise KicpError(KICP_ERR_ARG, "the weight table must have 256 entries")
    g = np.asarray(goals, dtype=np.int64).reshape(-1, 2)
    if g.size and (g.min() < 0 or g.max() > 0xFFFFFFFF):
        raise KicpError(KICP_ERR_ARG, "a goal (x, y) must not be negative")
    if not 0 <= int(max_potential) <= 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "max_potential must lie in 1 .. 0xFFFFFFFE")
    return cm, wt, np.ascontiguousarray(g, dtype=np.uint32), PlanConfig(int(max_potential))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_ubyte))


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint))


def _potential_out(out, shape):
    """the array a potential is written into: `out` (uint32, C-contiguous, of `shape`) or a new one"""
    return _out_array(out, shape, np.uint32, "(height, width)")


def _potential_result(out, stats, return_stats):
    return (out, tuple(int(v) for v in stats)) if return_stats else out


def potential_from_costmap(costmap, weight, goals, max_potential=MAX_POTENTIAL, return_stats=False, out=None):
    """kicp_potential_from_costmap: the cost-to-go field over a costmap shaped (height, width) with q = weight[costmap] (0: impassable)
    from `goals` = [(x, y), ...] -> uint32 (height, width): 0 on a passable goal, min(least sum of edge weights, max_potential) on every
    cell a path reaches, 0xFFFFFFFF elsewhere.  return_stats: also (goals used, cells below max_potential, cells at it, 0).  out: a uint32
    array of that shape to write into instead of a new one.  Pure host code: needs no GPU."""
    cm, wt, g, cfg = _plan_args(costmap, weight, goals, max_potential)
    out, stats = _potential_out(out, cm.shape), np.zeros(4, dtype=np.uint64)
    _check(lib().kicp_potential_from_costmap(_u8(cm), cm.shape[1], cm.shape[0], _u8(wt), C.byref(cfg), _u32(g), len(g), _u32(out), out.size,
                                             stats.ctypes.data_as(C.POINTER(C.c_ulonglong))))
    return _potential_result(out, stats, return_stats)


def potential_path(potential, costmap, weight, start):
    """kicp_potential_path: the path from `start` = (x, y) down `potential` (made from this costmap and these weights) -> uint32 (n, 2):
    the cells as (x, y), start and goal included.  Each step takes the first neighbour - +x, -x, +y, -y, then the diagonals - whose
    potential plus the edge's weight is the current cell's.  KICP_ERR_ARG for an unreachable start, KICP_ERR_CAPACITY for one at or
    inside the zone max_potential clamped.  Needs no GPU."""
    cm, wt, _, _ = _plan_args(costmap, weight, np.zeros((0, 2)), 1)
    pot = np.ascontiguousarray(potential, dtype=np.uint32)
    if pot.shape != cm.shape:
        raise KicpError(KICP_ERR_ARG, "the potential must have the costmap's shape")
    x, y = (int(v) for v in start)
    if min(x, y) < 0 or max(x, y) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "the start (x, y) must not be negative")
    cap, n = cm.shape[0] + cm.shape[1], C.c_size_t()
    while True:
        out = np.empty((cap, 2), dtype=np.uint32)
        rc = lib().kicp_potential_path(_u32(pot), _u8(cm), cm.shape[1], cm.shape[0], _u8(wt), x, y, _u32(out), cap, C.byref(n))
        if rc == KICP_ERR_CAPACITY and n.value > cap:  # the path is longer: its length came back
            cap = n.value
            continue
        _check(rc)
        return out[:n.value].copy()


ARCS_MAX_K, ARCS_MAX_T, ARCS_MAX_P = 1 << 20, 1024, 4096


def _out_array(out, shape, dtype, what):
    """the array a result is written into: `out` (of `dtype`, C-contiguous, of `shape`) or a new one"""
    if out is None:
        return np.empty(shape, dtype=dtype)
    if not isinstance(out, np.ndarray) or out.dtype != dtype or out.shape != tuple(shape) or not out.flags.c_contiguous or not out.flags.writeable:
        raise KicpError(KICP_ERR_ARG, "out must be a writeable C-contiguous %s array shaped %s" % (np.dtype(dtype).name, what))
    return out


def plan_q(costmap, weight, out=None):
    """kicp_plan_q: q = weight[costmap], uint8 of the costmap's shape (0: impassable) - half of the plan score_arcs_from_plan takes.
    Pure host code."""
    cm, wt = np.ascontiguousarray(costmap, dtype=np.uint8), np.ascontiguousarray(weight, dtype=np.uint8)
    if wt.shape != (256,):
        raise KicpError(KICP_ERR_ARG, "the weight table must have 256 entries")
    out = _out_array(out, cm.shape, np.uint8, "like the costmap")
    _check(lib().kicp_plan_q(_u8(cm), cm.size, _u8(wt), _u8(out)))
    return out


def arc_start(x, y, yaw):
    """the start of score_arcs from a planar pose: (x, y, cos(yaw), sin(yaw))"""
    return np.array([float(x), float(y), math.cos(yaw), math.sin(yaw)], dtype=np.float64)


def arc_steps(v, omega, dt, out=None):
    """kicp_arc_steps: one step (dx, dy, dc, ds) of the arc each command (v[k], omega[k]) drives in dt, the reference's motion model
    -> float64 (K, 4).  Pure host code."""
    va, vp = _d(np.asarray(v, dtype=np.float64).reshape(-1))
    wa, wp = _d(np.asarray(omega, dtype=np.float64).reshape(-1))
    if va.size != wa.size:
        raise KicpError(KICP_ERR_ARG, "v and omega must have the same length")
    out = _out_array(out, (va.size, 4), np.float64, "(K, 4)")
    _check(lib().kicp_arc_steps(vp, wp, float(dt), va.size, C.cast(out.ctypes.data, _dp)))
    return out


def footprint_box(x_min, x_max, y_min, y_max, spacing, out=None):
    """kicp_footprint_box: a lattice over the box [x_min, x_max] x [y_min, y_max] (base frame) that includes its boundary, at most
    `spacing` apart -> float64 (nx * ny, 2), x running fastest.  out: a float64 array of exactly that shape.  Pure host code."""
    box = [float(v) for v in (x_min, x_max, y_min, y_max, spacing)]
    n = C.c_size_t()
    rc = lib().kicp_footprint_box(*box, None, 0, C.byref(n))
    if rc != KICP_ERR_CAPACITY or n.value == 0:  # the count came back with KICP_ERR_CAPACITY; anything else is the error itself
        _check(rc)
    out = _out_array(out, (n.value, 2), np.float64, "(nx * ny, 2) = (%d, 2)" % n.value)
    _check(lib().kicp_footprint_box(*box, C.cast(out.ctypes.data, _dp), n.value, C.byref(n)))
    return out


def _arcs_args(start, arcs, n_steps, footprint):
    """-> (start [4], arcs (K, 4), footprint (P, 2), all float64, and n_steps); what the library cannot be handed is refused here"""
    s = np.ascontiguousarray(start, dtype=np.float64).reshape(-1)
    a, f = np.ascontiguousarray(arcs, dtype=np.float64), np.ascontiguousarray(footprint, dtype=np.float64)
    if s.size != 4:
        raise KicpError(KICP_ERR_ARG, "the start must be (x, y, cosine, sine)")
    if a.ndim != 2 or a.shape[1] != 4:
        raise KicpError(KICP_ERR_ARG, "the arcs must be shaped (K, 4): dx, dy, dc, ds")
    if f.ndim != 2 or f.shape[1] != 2:
        raise KicpError(KICP_ERR_ARG, "the footprint must be shaped (P, 2)")
    if not 0 <= int(n_steps) <= 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "n_steps must lie in 1 .. %d" % ARCS_MAX_T)
    return s, a, f, int(n_steps)


def score_arcs_from_plan(q, potential, cell, origin_x, origin_y, start, arcs, n_steps, footprint, out=None):
    """kicp_score_arcs_from_plan: every arc of `arcs` (K, 4) rolled n_steps poses forward from `start` = (x, y, cosine, sine) with the
    footprint's samples (P, 2) laid on q (uint8 (height, width), 0 impassable: plan_q makes it) at every pose -> uint32 (K, 4):
    free_steps, cost_sum, cost_max, end_potential (the potential at the last free pose; 0xFFFFFFFF outside the grid).  out: a uint32
    (K, 4) array to write into.  Pure host code: needs no GPU."""
    qa, pot = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(potential, dtype=np.uint32)
    if qa.ndim != 2 or qa.size == 0 or pot.shape != qa.shape:
        raise KicpError(KICP_ERR_ARG, "q and the potential must be shaped (height, width), both at least 1")
    s, a, f, n_steps = _arcs_args(start, arcs, n_steps, footprint)
    out = _out_array(out, (len(a), 4), np.uint32, "(K, 4)")
    _check(lib().kicp_score_arcs_from_plan(_u8(qa), _u32(pot), float(cell), float(origin_x), float(origin_y), qa.shape[1], qa.shape[0], C.cast(s.ctypes.data, _dp),
                                           C.cast(a.ctypes.data, _dp), len(a), n_steps, C.cast(f.ctypes.data, _dp), len(f), _u32(out), out.size))
    return out


def arcs_best(results, n_steps, w_potential=1, w_cost=0, w_blocked=0, min_free_steps=1):
    """kicp_arcs_best: the index of the admissible arc (free_steps >= min_free_steps, end_potential != 0xFFFFFFFF) of least
    w_potential * end_potential + w_cost * cost_sum + w_blocked * (n_steps - free_steps), the lowest on a tie; None when no arc is
    admissible.  Pure host code."""
    r = np.ascontiguousarray(results, dtype=np.uint32)
    if r.ndim != 2 or r.shape[1] != 4:
        raise KicpError(KICP_ERR_ARG, "the results must be shaped (K, 4)")
    args = [int(v) for v in (w_potential, w_cost, w_blocked, n_steps, min_free_steps)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "the weights, n_steps and min_free_steps are unsigned 32-bit integers")
    index = C.c_size_t()
    _check(lib().kicp_arcs_best(_u32(r), len(r), *args, C.byref(index)))
    return None if index.value == len(r) else int(index.value)


ARC_TREE_MAX_DEPTH, ARC_TREE_MAX_NODES, ARC_TREE_MAX_T = 8, 1 << 20, 1024


def _arc_tree_levels(branch, steps):
    """-> (branch, steps) as uint32 arrays with one entry per level; what the library cannot be handed is refused here"""
    b, s = np.asarray(branch).reshape(-1), np.asarray(steps).reshape(-1)
    if b.size != s.size:
        raise KicpError(KICP_ERR_ARG, "branch and steps must have the same length: one entry per level")
    for a in (b, s):
        if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise KicpError(KICP_ERR_ARG, "branch and steps hold unsigned 32-bit integers, at least 1")
    return np.ascontiguousarray(b, dtype=np.uint32), np.ascontiguousarray(s, dtype=np.uint32)


def arc_tree_nodes(branch, steps):
    """kicp_arc_tree_nodes: the counts of the tree with branch[d] primitives and steps[d] steps at level d + 1 ->
    (n_nodes, n_leaves, total_steps, level_offset): the rows of all levels, the nodes of the last one, the steps along a path and the row
    each level begins at.  Raises on a tree the scoring entries refuse (depth above 8, more than 2^20 nodes, more than 1 024 steps along
    a path: KICP_ERR_CAPACITY; no level, a zero: KICP_ERR_ARG).  Pure host code."""
    b, s = _arc_tree_levels(branch, steps)
    n_nodes, n_leaves, total = C.c_size_t(), C.c_size_t(), C.c_uint()
    offsets = (C.c_size_t * max(b.size, 1))()
    _check(lib().kicp_arc_tree_nodes(b.size, _u32(b), _u32(s), C.byref(n_nodes), C.byref(n_leaves), C.byref(total), offsets))
    return int(n_nodes.value), int(n_leaves.value), int(total.value), tuple(int(v) for v in offsets[:b.size])


def _arc_tree_args(start, branch, steps, primitives, footprint):
    """-> (start [4], branch [D], steps [D], primitives (sum of branch, 4), footprint (P, 2), n_nodes)"""
    b, st = _arc_tree_levels(branch, steps)
    n_nodes = arc_tree_nodes(b, st)[0]
    s = np.ascontiguousarray(start, dtype=np.float64).reshape(-1)
    p, f = np.ascontiguousarray(primitives, dtype=np.float64), np.ascontiguousarray(footprint, dtype=np.float64)
    if s.size != 4:
        raise KicpError(KICP_ERR_ARG, "the start must be (x, y, cosine, sine)")
    if p.ndim != 2 or p.shape != (int(b.sum(dtype=np.uint64)), 4):
        raise KicpError(KICP_ERR_ARG, "the primitives must be shaped (sum of branch, 4) = (%d, 4): dx, dy, dc, ds, level 1's rows first" % int(b.sum(dtype=np.uint64)))
    if f.ndim != 2 or f.shape[1] != 2:
        raise KicpError(KICP_ERR_ARG, "the footprint must be shaped (P, 2)")
    return s, b, st, p, f, n_nodes


def score_arc_tree_from_plan(q, potential, cell, origin_x, origin_y, start, branch, steps, primitives, footprint, out=None):
    """kicp_score_arc_tree_from_plan: a tree of arc segments on the plan score_arcs_from_plan takes.  Level d + 1 has branch[d]
    primitives - rows (dx, dy, dc, ds) of `primitives`, level 1's first - each held for steps[d] steps; a node's trajectory runs from
    `start` through the primitives of its path -> uint32 (N, 4), the rows level-major (arc_tree_nodes gives N and where each level
    begins; the child with primitive b of the node j of a level is the node j * branch + b of the next): free_steps along the whole
    path, cost_sum, cost_max, end_potential.  A node under one that collided repeats its four words.  out: a uint32 (N, 4) array to
    write into.  Pure host code: needs no GPU."""
    qa, pot = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(potential, dtype=np.uint32)
    if qa.ndim != 2 or qa.size == 0 or pot.shape != qa.shape:
        raise KicpError(KICP_ERR_ARG, "q and the potential must be shaped (height, width), both at least 1")
    s, b, st, p, f, n_nodes = _arc_tree_args(start, branch, steps, primitives, footprint)
    out = _out_array(out, (n_nodes, 4), np.uint32, "(N, 4) = (%d, 4)" % n_nodes)
    _check(lib().kicp_score_arc_tree_from_plan(_u8(qa), _u32(pot), float(cell), float(origin_x), float(origin_y), qa.shape[1], qa.shape[0], C.cast(s.ctypes.data, _dp),
                                               b.size, _u32(b), _u32(st), C.cast(p.ctypes.data, _dp), C.cast(f.ctypes.data, _dp), len(f), _u32(out), out.size))
    return out


def arc_tree_best(results, branch, steps, w_potential=1, w_cost=0, w_blocked=0, min_free_steps=1):
    """kicp_arc_tree_best: among the LEAVES of a scored tree (results: uint32 (N, 4) as the scoring entries write them) the admissible
    one of least score, by arcs_best's rule with n_steps = the steps along a path, the lowest in-level index on a tie ->
    (leaf, path): the leaf's in-level index and the primitive its path takes at every level - path[0] is the command to execute
    now; None when no leaf is admissible.  Pure host code."""
    b, st = _arc_tree_levels(branch, steps)
    n_nodes, n_leaves = arc_tree_nodes(b, st)[:2]
    r = np.ascontiguousarray(results, dtype=np.uint32)
    if r.shape != (n_nodes, 4):
        raise KicpError(KICP_ERR_ARG, "the results must be shaped (N, 4) = (%d, 4)" % n_nodes)
    args = [int(v) for v in (w_potential, w_cost, w_blocked, min_free_steps)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "the weights and min_free_steps are unsigned 32-bit integers")
    leaf, path = C.c_size_t(), np.zeros(b.size, dtype=np.uint32)
    _check(lib().kicp_arc_tree_best(_u32(r), b.size, _u32(b), _u32(st), *args, C.byref(leaf), _u32(path)))
    return None if leaf.value == n_leaves else (int(leaf.value), tuple(int(v) for v in path))


FRONTIER_WORDS = 10


def _frontier_config(min_observations, occupied_thresh, min_size):
    args = [int(min_observations), int(min_size)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "min_observations and min_size are unsigned 32-bit integers, at least 1")
    return FrontierConfig(args[0], float(occupied_thresh), args[1])


def _frontier_call(call, shape, return_labels):
    """call(rows pointer, cap, byref(n), labels pointer, cap_labels) -> rc, with a modest capacity first and, when more frontiers pass the
    filter than that, once more with the number that came back -> uint64 (F, 10), or that and uint32 labels of `shape`"""
    labels = np.empty(shape, dtype=np.uint32) if return_labels else None
    lp, lcap = (_u32(labels), labels.size) if return_labels else (None, 0)
    cap, n = 256, C.c_size_t()
    rows = np.empty((cap, FRONTIER_WORDS), dtype=np.uint64)
    rc = call(rows.ctypes.data_as(C.POINTER(C.c_ulonglong)), cap, C.byref(n), lp, lcap)
    if rc == KICP_ERR_CAPACITY and n.value > cap:  # more frontiers than that: their number came back
        cap = n.value
        rows = np.empty((cap, FRONTIER_WORDS), dtype=np.uint64)
        rc = call(rows.ctypes.data_as(C.POINTER(C.c_ulonglong)), cap, C.byref(n), lp, lcap)
    _check(rc)
    rows = rows[:n.value].copy()
    return (rows, labels) if return_labels else rows


def frontiers_from_occupancy(occupancy, min_observations=1, occupied_thresh=0.65, min_size=1, potential=None, return_labels=False):
    """kicp_frontiers_from_occupancy: the exploration frontiers of a readout shaped (height, width) - the clear cells with an unknown edge
    neighbour, joined over their eight neighbours - of at least min_size cells, in ascending label order -> uint64 (F, 10): label (the
    least cell index y * width + x), size, sum of x, sum of y, min x, max x, min y, max y, best_potential (the least of `potential`,
    uint32 (height, width), over the cells; 0xFFFFFFFF without one) and best_cell (the least index that attains it).  return_labels:
    also uint32 (height, width), the label on every frontier cell - of the small frontiers too - and 0xFFFFFFFF elsewhere.  Pure host
    code: needs no GPU."""
    occ = _occupancy_2d(occupancy)
    cfg = _frontier_config(min_observations, occupied_thresh, min_size)
    pot = None
    if potential is not None:
        pot = np.ascontiguousarray(potential, dtype=np.uint32)
        if pot.shape != occ.shape:
            raise KicpError(KICP_ERR_ARG, "the potential must have the occupancy's shape")
    return _frontier_call(lambda rp, cap, n, lp, lcap: lib().kicp_frontiers_from_occupancy(occ.ctypes.data_as(C.POINTER(C.c_byte)), occ.shape[1], occ.shape[0], C.byref(cfg),
                                                                                           None if pot is None else _u32(pot), rp, cap, n, lp, lcap),
                          occ.shape, return_labels)


GAIN_WORDS = 4


def _gain_config(range_cells, min_observations, occupied_thresh):
    args = [int(min_observations), int(range_cells)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "min_observations and range_cells are unsigned 32-bit integers, at least 1")
    return GainConfig(args[0], float(occupied_thresh), args[1])


def _gain_views(views, width, height):
    """viewpoints as cell indices y * width + x (any shape but (N, 2): flattened) or as an (N, 2) array of (x, y) -> uint32 (N,)"""
    v = np.asarray(views)
    if v.size and v.dtype.kind not in "iu":
        raise KicpError(KICP_ERR_ARG, "viewpoints are integers: cell indices, or an (N, 2) array of (x, y)")
    v = v.astype(np.int64)
    if v.ndim == 2 and v.shape[1] == 2:
        if v.size and not ((v >= 0).all() and (v[:, 0] < width).all() and (v[:, 1] < height).all()):
            bad = int(np.flatnonzero((v < 0).any(axis=1) | (v[:, 0] >= width) | (v[:, 1] >= height))[0])
            raise KicpError(KICP_ERR_ARG, "viewpoint %d is (%d, %d), outside the grid of %d x %d cells" % (bad, v[bad, 0], v[bad, 1], width, height))
        v = v[:, 1] * width + v[:, 0]
    v = v.reshape(-1)
    if v.size and (v.min() < 0 or v.max() > 0xFFFFFFFF):
        raise KicpError(KICP_ERR_ARG, "viewpoints are cell indices, unsigned 32-bit integers")
    return np.ascontiguousarray(v, dtype=np.uint32)


def gain_from_occupancy(occupancy, views, range_cells, min_observations=1, occupied_thresh=0.65):
    """kicp_gain_from_occupancy: what a sensor of range_cells' range (1 .. 361) would see from each viewpoint of a readout shaped
    (height, width): from a clear viewpoint 8 R rays are walked to the cells at Chebyshev distance R, cut to the disc of radius R; a ray
    ends where it leaves the grid or at an occupied cell and passes through unknown cells, which it thereby sees (include/kicp.h states
    the walk).  views: cell indices y * width + x - word 9 of a frontier's row - or an (N, 2) array of (x, y) -> uint32 (N, 4): the
    distinct unknown cells seen, the rays blocked, the rays that left the grid, and the class of the viewpoint's own cell (0 clear,
    1 unknown, 2 occupied: then the other three are 0).  Pure host code: needs no GPU."""
    occ = _occupancy_2d(occupancy)
    cfg = _gain_config(range_cells, min_observations, occupied_thresh)
    v = _gain_views(views, occ.shape[1], occ.shape[0])
    out = np.empty((len(v), GAIN_WORDS), dtype=np.uint32)
    _check(lib().kicp_gain_from_occupancy(occ.ctypes.data_as(C.POINTER(C.c_byte)), occ.shape[1], occ.shape[0], C.byref(cfg), _u32(v), len(v), _u32(out), out.size))
    return out


def _struct(cls, value):
    """a ctypes struct of integers: an instance of cls, or its fields as a tuple or a dict"""
    if isinstance(value, cls):
        return value
    if isinstance(value, dict):
        value = [value[name] for name, _ in cls._fields_]
    return cls(*[int(v) for v in value])


def _traversability_call(call, w, h, return_ground, return_fit, return_counts, fit_values, count_words):
    """what the traversability entries share: the outputs, the call, and what is returned - the classes alone, or a tuple with the
    ground bytes, the fit and / or the counts behind them.  fit_values = 0: the entry has no fit argument; 3: the fit is int64 (h, w, 3)
    - D, Da, Db - and the counts are five; 5: with ROUGH (h, w, 5) - D, Da, Db, Q, n - and six"""
    out = np.empty((h, w), dtype=np.int8)
    ground = np.empty((h, w), dtype=np.uint8) if return_ground else None
    fit = np.empty((h, w, fit_values), dtype=np.int64) if return_fit else None
    counts = np.zeros(count_words, dtype=np.uint64)
    fit_arg = [fit.ctypes.data_as(C.POINTER(C.c_longlong)) if return_fit else None] if fit_values else []
    _check(call(out.ctypes.data_as(C.POINTER(C.c_byte)), ground.ctypes.data_as(C.POINTER(C.c_ubyte)) if return_ground else None, *fit_arg,
                counts.ctypes.data_as(C.POINTER(C.c_ulonglong)) if return_counts else None, out.size))
    if not (return_ground or return_fit or return_counts):
        return out
    return (out,) + ((ground,) if return_ground else ()) + ((fit,) if return_fit else ()) + ((tuple(int(v) for v in counts),) if return_counts else ())


def _elev_classes(step_slabs, robot_slabs, *fit):
    """a classification - plain, with a slope config, or with a slope and a rough config (each a struct, a tuple or a dict) -> the suffix
    of its entries' names, its configs by reference, fit_values and count_words (_traversability_call)"""
    cfgs = [ElevationTraversabilityConfig(int(step_slabs), int(robot_slabs))] + [_struct(cls, v) for cls, v in zip((ElevationSlopeConfig, ElevationRoughConfig), fit)]
    return ("", "_slope", "_rough")[len(fit)], [C.byref(v) for v in cfgs], (0, 3, 5)[len(fit)], 4 + len(fit)


def _traversability_from_columns(columns, rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, *fit):
    """what the three *_from_columns functions share"""
    c = np.ascontiguousarray(columns, dtype=np.uint64)
    if c.ndim != 2 or c.size == 0:
        raise KicpError(KICP_ERR_ARG, "columns must be shaped (height, width), both at least 1")
    x0, y0, w, h = _rect(rect, c.shape[1], c.shape[0])
    suffix, cfgs, fit_values, count_words = _elev_classes(step_slabs, robot_slabs, *fit)
    entry = getattr(lib(), "kicp_elev_traversability" + suffix + "_from_columns")
    return _traversability_call(lambda *outs: entry(c.ctypes.data_as(C.POINTER(C.c_ulonglong)), c.shape[1], c.shape[0], *cfgs, x0, y0, w, h, *outs), w, h, return_ground,
                                return_fit, return_counts, fit_values, count_words)


def traversability_from_columns(columns, step_slabs, robot_slabs, rect=None, return_ground=False, return_counts=False):
    """kicp_elev_traversability_from_columns: the classes of the cells of `rect` = (x0, y0, w, h) (None: the full layer) from columns
    shaped (height, width), uint64 -> int8 (h, w): -1 unknown, 0 traversable, 100 obstacle (BODY: something between step_slabs and
    robot_slabs over the cell's ground; STEP: an 8-neighbour's ground more than step_slabs below).  return_ground adds uint8 (h, w), the
    ground's slab, 255 unknown; return_counts adds (unknown, traversable, BODY, STEP only).  Pure host code: needs no GPU."""
    return _traversability_from_columns(columns, rect, return_ground, False, return_counts, step_slabs, robot_slabs)


def traversability_slope_from_columns(columns, step_slabs, robot_slabs, slope, rect=None, return_ground=False, return_fit=False, return_counts=False):
    """kicp_elev_traversability_slope_from_columns: traversability_from_columns with the slope limit - a cell is also an obstacle when a
    least-squares plane through the known grounds of its window (include/kicp.h states the fit) is steeper than slope.rise_slabs slabs
    per slope.run_cells cells.  slope: an ElevationSlopeConfig, or its five fields as a tuple or a dict.  return_fit adds int64
    (h, w, 3): the determinants D, Da, Db of the fit - the gradient is (Da / D, Db / D) slabs per cell -, zeros where a cell has no fit;
    return_counts adds (unknown, traversable, BODY, STEP only, SLOPE only).  Pure host code: needs no GPU."""
    return _traversability_from_columns(columns, rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, slope)


def traversability_rough_from_columns(columns, step_slabs, robot_slabs, slope, rough, rect=None, return_ground=False, return_fit=False, return_counts=False):
    """kicp_elev_traversability_rough_from_columns: traversability_slope_from_columns with the class ROUGH - a cell with a fit is also an
    obstacle when the mean squared residual of its fit set to the fitted plane exceeds rough.num / rough.den slabs^2 (include/kicp.h
    states Q).  rough: an ElevationRoughConfig, or (num, den), or a dict.  return_fit adds int64 (h, w, 5): D, Da, Db, Q, n - the mean
    squared residual is Q / (n D) -, zeros where a cell has no fit; return_counts adds (unknown, traversable, BODY, STEP only, SLOPE
    only, ROUGH only).  Pure host code: needs no GPU."""
    return _traversability_from_columns(columns, rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, slope, rough)


def elev_slope_limit(cell, slab, max_tangent):
    """kicp_elev_slope_limit: -> (rise_slabs, run_cells) of the slope limit whose tangent is max_tangent on cells of side `cell` and
    slabs of `slab` metres: run_cells = 1024, rise_slabs = floor(max_tangent * cell / slab * 1024)"""
    cfg, rise, run = ElevationConfig(float(cell), 0.0, 0.0, 0, 0, 0.0, float(slab), 0.0), C.c_uint(), C.c_uint()
    _check(lib().kicp_elev_slope_limit(C.byref(cfg), float(max_tangent), C.byref(rise), C.byref(run)))
    return rise.value, run.value


def elev_rough_limit(slab, rms_metres):
    """kicp_elev_rough_limit: -> (num, den) of the ROUGH limit whose r.m.s. residual is rms_metres on slabs of `slab` metres: den = 1024,
    num = floor((rms_metres / slab)^2 * 1024)"""
    cfg, num, den = ElevationConfig(0.0, 0.0, 0.0, 0, 0, 0.0, float(slab), 0.0), C.c_uint(), C.c_uint()
    _check(lib().kicp_elev_rough_limit(C.byref(cfg), float(rms_metres), C.byref(num), C.byref(den)))
    return num.value, den.value


def fill_unknown_counts(dst_counts, src_counts, min_observations=1, free_max=25, occupied_min=101, return_counts=False):
    """kicp_grid_fill_unknown_counts: OccupancyGrid.fill_unknown as pure host code over counters in counts()' layout - uint16 (..., 2),
    the same shape - -> the destination's counters after the fill, a new array (the arguments are not changed); return_counts adds
    the seven counts.  Needs no GPU."""
    d, s = np.array(dst_counts, dtype=np.uint16, order="C"), np.ascontiguousarray(src_counts, dtype=np.uint16)
    if d.shape != s.shape or d.size % 2:
        raise KicpError(KICP_ERR_ARG, "the two arrays must have one shape and hold (hits, misses) pairs")
    cfg, counts = GridFillConfig(int(min_observations), int(free_max), int(occupied_min)), np.zeros(7, dtype=np.uint64)
    _check(lib().kicp_grid_fill_unknown_counts(d.ctypes.data_as(C.POINTER(C.c_ushort)), s.ctypes.data_as(C.POINTER(C.c_ushort)), d.size // 2, C.byref(cfg),
                                               counts.ctypes.data_as(C.POINTER(C.c_ulonglong)) if return_counts else None))
    return (d, tuple(int(v) for v in counts)) if return_counts else d


def elev_update_columns(config, columns, frame, pose, sensor_xyz=(0.0, 0.0, 0.0), margin_steps=2, widen_slabs=1, keep_ground=1):
    """kicp_elev_update_columns: ElevationLayer.update as pure host code.  config: an ElevationConfig, or a dict with its fields;
    columns: uint64 (height, width), contiguous, CHANGED IN PLACE -> the nine words of the update.  Needs no GPU."""
    cfg = config if isinstance(config, ElevationConfig) else ElevationConfig(*[config[name] for name, _ in ElevationConfig._fields_])
    if not (isinstance(columns, np.ndarray) and columns.dtype == np.uint64 and columns.flags.c_contiguous and columns.flags.writeable):
        raise KicpError(KICP_ERR_ARG, "columns must be a writeable contiguous uint64 array")
    a, p = _d(np.asarray(frame, dtype=np.float64).reshape(-1, 3))
    s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
    carve, out = ElevationCarveConfig(int(margin_steps), int(widen_slabs), int(keep_ground)), np.zeros(9, dtype=np.uint64)
    _check(lib().kicp_elev_update_columns(C.byref(cfg), columns.ctypes.data_as(C.POINTER(C.c_ulonglong)), columns.size, p if a.size else None, a.size // 3, _pose_ptr(pose), sp,
                                          C.byref(carve), out.ctypes.data_as(C.POINTER(C.c_ulonglong))))
    return tuple(int(v) for v in out)


class OccupancyGrid:
    """kicp_grid: a world-aligned 2-D grid of (hits, misses) counters a mapping run draws frame by frame - every used point's cell is
    hit, the cells its ray from the sensor crosses are missed, once per cell per frame (include/kicp.h states the exact semantics).
    It owns its device memory; the counters stay in HBM until they are asked for."""

    def __init__(self, cell, origin_x, origin_y, width, height, z_min, z_max, max_ray, device=0):
        self._h = None
        cfg = GridConfig(float(cell), float(origin_x), float(origin_y), int(width), int(height), float(z_min), float(z_max), float(max_ray))
        h = C.c_void_p()
        _check(lib().kicp_grid_create(C.byref(cfg), int(device), C.byref(h)))
        self._h, self.device, self.width, self.height = h, device, int(width), int(height)
        self._last = np.zeros(4, dtype=np.uint64)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.kicp_grid_destroy(self._h)
            self._h = None

    def info(self):
        """-> dict: the configuration's fields, reach (cells) and frames (integrated since creation or clear)"""
        cfg, reach, frames = GridConfig(), C.c_int(), C.c_ulonglong()
        _check(lib().kicp_grid_info(self._h, C.byref(cfg), C.byref(reach), C.byref(frames)))
        out = {name: getattr(cfg, name) for name, _ in GridConfig._fields_}
        out.update(reach=reach.value, frames=frames.value)
        return out

    def clear(self):
        _check(lib().kicp_grid_clear(self._h))

    def integrate(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0)):
        """kicp_grid_integrate: one frame of points in the base frame (host memory) at `pose`, the sensor at `sensor_xyz` in the base frame
        -> (points used, points skipped, cells HIT, cells MISS)"""
        a, p = _d(np.asarray(frame, dtype=np.float64).reshape(-1, 3))
        s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
        _check(lib().kicp_grid_integrate(self._h, p if a.size else None, a.size // 3, _pose_ptr(pose), sp, self._last.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return self.last_frame()

    def integrate_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), n=None):
        """kicp_grid_integrate_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
        count = device_frame.n if n is None else int(n)
        _check(lib().kicp_grid_integrate_device(self._h, device_frame.ptr if count else None, count, _pose_ptr(pose), sp,
                                                self._last.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return self.last_frame()

    def last_frame(self):
        """(points used, points skipped, cells HIT, cells MISS) of the last integrated frame"""
        return tuple(int(v) for v in self._last)

    def counts(self):
        """-> uint16 (height, width, 2): hits, misses"""
        out = np.empty((self.height, self.width, 2), dtype=np.uint16)
        _check(lib().kicp_grid_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_ushort)), self.width * self.height))
        return out

    def set_counts(self, counts):
        c = np.ascontiguousarray(counts, dtype=np.uint16)
        if c.size % 2:
            raise KicpError(KICP_ERR_ARG, "counts must hold (hits, misses) pairs")
        _check(lib().kicp_grid_set_counts(self._h, c.ctypes.data_as(C.POINTER(C.c_ushort)), c.size // 2))

    def fill_unknown(self, src, min_observations=1, free_max=25, occupied_min=101, return_counts=False):
        """kicp_grid_fill_unknown: on the GPU, the unknown cells of this grid - both counters 0 - become traversable (0, 1) where `src`,
        an OccupancyGrid of the same geometry, reads 0 .. free_max at min_observations, and obstacles (1, 0) where it reads occupied_min
        or more (101: never); every other counter keeps its bits, `src` is not changed, and the plan of this grid is invalidated.
        return_counts -> (kept obstacle, kept traversable, filled free, filled occupied, left unknown, traversable over a source
        OCCUPIED, obstacle over a source FREE)"""
        cfg, counts = GridFillConfig(int(min_observations), int(free_max), int(occupied_min)), np.zeros(7, dtype=np.uint64)
        _check(lib().kicp_grid_fill_unknown(self._h, src._h if src is not None else None, C.byref(cfg),
                                            counts.ctypes.data_as(C.POINTER(C.c_ulonglong)) if return_counts else None))
        return tuple(int(v) for v in counts) if return_counts else None

    def occupancy(self, min_observations=1):
        """kicp_grid_occupancy: the readout on the GPU -> int8 (height, width): -1 unknown, else 0 .. 100 - a nav_msgs/OccupancyGrid's data"""
        out = np.empty((self.height, self.width), dtype=np.int8)
        _check(lib().kicp_grid_occupancy(self._h, int(min_observations), out.ctypes.data_as(C.POINTER(C.c_byte)), out.size))
        return out

    def clearance(self, radius_cells, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, rect=None):
        """kicp_grid_clearance: on the GPU, the squared distance in cells from every cell of `rect` = (x0, y0, w, h) (None: the full grid)
        to the nearest source within radius_cells of it - inside the rectangle or not - radius_cells^2 + 1 where there is none
        -> uint16 (h, w)"""
        x0, y0, w, h = _rect(rect, self.width, self.height)
        cfg = _clearance_config(radius_cells, min_observations, occupied_thresh, unknown_is_obstacle)
        out = np.empty((h, w), dtype=np.uint16)
        _check(lib().kicp_grid_clearance(self._h, C.byref(cfg), x0, y0, w, h, out.ctypes.data_as(C.POINTER(C.c_ushort)), out.size))
        return out

    def costmap(self, table, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=False, rect=None):
        """kicp_grid_costmap: on the GPU, Nav2's costs of the cells of `rect` from `table`[clearance] (nav2_cost_table builds one; its
        length R^2 + 2 gives R) -> uint8 (h, w): a nav2_msgs/Costmap's data"""
        t = _cost_table(table)
        x0, y0, w, h = _rect(rect, self.width, self.height)
        cfg = _clearance_config(_table_radius(t), min_observations, occupied_thresh, unknown_is_obstacle)
        out = np.empty((h, w), dtype=np.uint8)
        _check(lib().kicp_grid_costmap(self._h, C.byref(cfg), t.ctypes.data_as(C.POINTER(C.c_ubyte)), t.size, 1 if inflate_unknown else 0, x0, y0, w, h,
                                       out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size))
        return out

    def potential_of_costmap(self, costmap, weight, goals, max_potential=MAX_POTENTIAL, return_stats=False, out=None):
        """kicp_grid_potential_of_costmap: on the GPU, the cost-to-go field of potential_from_costmap over `costmap` (uint8, the grid's
        (height, width)) -> uint32 (height, width).  return_stats: also (goals used, cells below max_potential, cells at it, relaxation
        rounds - the last depends on the implementation); out: as potential_from_costmap's."""
        cm, wt, g, cfg = _plan_args(costmap, weight, goals, max_potential)
        if cm.shape != (self.height, self.width):
            raise KicpError(KICP_ERR_ARG, "the costmap must have the grid's shape (height, width)")
        out, stats = _potential_out(out, cm.shape), np.zeros(4, dtype=np.uint64)
        _check(lib().kicp_grid_potential_of_costmap(self._h, _u8(cm), _u8(wt), C.byref(cfg), _u32(g), len(g), _u32(out), out.size,
                                                    stats.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return _potential_result(out, stats, return_stats)

    def potential(self, table, weight, goals, max_potential=MAX_POTENTIAL, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=False,
                  return_stats=False, out=None):
        """kicp_grid_potential: on the GPU, the full grid's costmap (the arguments and bytes of costmap()) and the cost-to-go field over
        it from `goals` = [(x, y), ...] - the costmap never leaves HBM -> uint32 (height, width); return_stats and out as
        potential_of_costmap's"""
        t = _cost_table(table)
        cfg = _clearance_config(_table_radius(t), min_observations, occupied_thresh, unknown_is_obstacle)
        _, wt, g, plan = _plan_args(np.zeros((1, 1), dtype=np.uint8), weight, goals, max_potential)
        out, stats = _potential_out(out, (self.height, self.width)), np.zeros(4, dtype=np.uint64)
        _check(lib().kicp_grid_potential(self._h, C.byref(cfg), _u8(t), t.size, 1 if inflate_unknown else 0, _u8(wt), C.byref(plan), _u32(g), len(g), _u32(out), out.size,
                                         stats.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return _potential_result(out, stats, return_stats)

    def has_plan(self):
        """kicp_grid_has_plan: does the handle hold the plan of a potential call that succeeded?"""
        return bool(lib().kicp_grid_has_plan(self._h))

    def score_arcs(self, start, arcs, n_steps, footprint, out=None):
        """kicp_grid_score_arcs: on the GPU, score_arcs_from_plan's result on the plan the last potential() or potential_of_costmap()
        left in the handle (KICP_ERR_ARG when there is none) -> uint32 (K, 4); the plan never leaves HBM.  out: as
        score_arcs_from_plan's."""
        s, a, f, n_steps = _arcs_args(start, arcs, n_steps, footprint)
        out = _out_array(out, (len(a), 4), np.uint32, "(K, 4)")
        _check(lib().kicp_grid_score_arcs(self._h, C.cast(s.ctypes.data, _dp), C.cast(a.ctypes.data, _dp), len(a), n_steps, C.cast(f.ctypes.data, _dp), len(f), _u32(out),
                                          out.size))
        return out

    def score_arc_tree(self, start, branch, steps, primitives, footprint, out=None):
        """kicp_grid_score_arc_tree: on the GPU, score_arc_tree_from_plan's result on the plan the last potential() or
        potential_of_costmap() left in the handle (KICP_ERR_ARG when there is none) -> uint32 (N, 4), one launch per level; the plan
        never leaves HBM.  out: as score_arc_tree_from_plan's."""
        s, b, st, p, f, n_nodes = _arc_tree_args(start, branch, steps, primitives, footprint)
        out = _out_array(out, (n_nodes, 4), np.uint32, "(N, 4) = (%d, 4)" % n_nodes)
        _check(lib().kicp_grid_score_arc_tree(self._h, C.cast(s.ctypes.data, _dp), b.size, _u32(b), _u32(st), C.cast(p.ctypes.data, _dp), C.cast(f.ctypes.data, _dp), len(f),
                                              _u32(out), out.size))
        return out

    def frontiers(self, min_observations=1, occupied_thresh=0.65, min_size=1, use_plan=False, return_labels=False):
        """kicp_grid_frontiers: on the GPU, frontiers_from_occupancy's result on the counters where they are -> uint64 (F, 10), and uint32
        (height, width) labels with return_labels.  use_plan: best_potential and best_cell come from the plan the last potential() or
        potential_of_costmap() left in the handle (KICP_ERR_ARG when there is none) - with the robot's cell as that call's one goal,
        the cost of driving to each frontier and the cell to drive to.  The plan is a snapshot, the frontiers are the current counters';
        neither is changed."""
        cfg = _frontier_config(min_observations, occupied_thresh, min_size)
        return _frontier_call(lambda rp, cap, n, lp, lcap: lib().kicp_grid_frontiers(self._h, C.byref(cfg), 1 if use_plan else 0, rp, cap, n, lp, lcap),
                              (self.height, self.width), return_labels)

    def gain(self, views, range_cells, min_observations=1, occupied_thresh=0.65):
        """kicp_grid_gain: on the GPU, gain_from_occupancy's result on the counters where they are -> uint32 (N, 4): per viewpoint (a cell
        index, such as frontiers(use_plan=True)[:, 9], or (x, y)) the distinct unknown cells a sensor of range_cells' range would see, the
        rays blocked, the rays that left the grid and the class of the viewpoint's cell.  Neither the counters nor the plan are changed."""
        cfg = _gain_config(range_cells, min_observations, occupied_thresh)
        v = _gain_views(views, self.width, self.height)
        out = np.empty((len(v), GAIN_WORDS), dtype=np.uint32)
        _check(lib().kicp_grid_gain(self._h, C.byref(cfg), _u32(v), len(v), _u32(out), out.size))
        return out

    def last_window(self):
        """kicp_grid_last_window: (x0, y0, w, h) of the last integrated frame's window clipped to the grid; w = h = 0 when it lies
        outside and before any frame.  Grown by R and clipped it is all a costmap has to refresh after that frame."""
        v = [C.c_uint() for _ in range(4)]
        _check(lib().kicp_grid_last_window(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def save_map(self, prefix, min_observations=1, occupied_thresh=0.65, free_thresh=0.25):
        """kicp_grid_save_map: <prefix>.pgm + <prefix>.yaml of the readout"""
        _check(lib().kicp_grid_save_map(self._h, os.fsencode(prefix), int(min_observations), float(occupied_thresh), float(free_thresh)))


class ElevationLayer:
    """kicp_elev: a world-aligned layer over a grid's geometry that keeps, per cell, one 64-bit column of the world heights that ever
    returned there, and reads traversability off it by height over the local ground (include/kicp.h states the exact semantics and the
    known limitations).  integrate only ever sets bits; update also clears the bits a frame's rays pass through, so what has left is
    forgotten.  It owns its device memory; the columns stay in HBM until they are asked for."""

    def __init__(self, cell, origin_x, origin_y, width, height, z_origin, slab, max_ray, device=0):
        self._h = None
        cfg = ElevationConfig(float(cell), float(origin_x), float(origin_y), int(width), int(height), float(z_origin), float(slab), float(max_ray))
        h = C.c_void_p()
        _check(lib().kicp_elev_create(C.byref(cfg), int(device), C.byref(h)))
        self._h, self.device, self.width, self.height = h, device, int(width), int(height)
        self._last, self._last_update = np.zeros(6, dtype=np.uint64), np.zeros(9, dtype=np.uint64)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.kicp_elev_destroy(self._h)
            self._h = None

    def info(self):
        """-> dict: the configuration's fields, reach (cells) and frames (integrated since creation or clear)"""
        cfg, reach, frames = ElevationConfig(), C.c_int(), C.c_ulonglong()
        _check(lib().kicp_elev_info(self._h, C.byref(cfg), C.byref(reach), C.byref(frames)))
        out = {name: getattr(cfg, name) for name, _ in ElevationConfig._fields_}
        out.update(reach=reach.value, frames=frames.value)
        return out

    def clear(self):
        _check(lib().kicp_elev_clear(self._h))

    def integrate(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0)):
        """kicp_elev_integrate: one frame of points in the base frame (host memory) at `pose`, the sensor at `sensor_xyz` in the base frame
        -> (used, skipped, outside_grid, outside_column, new_bits, new_cells)"""
        a, p = _d(np.asarray(frame, dtype=np.float64).reshape(-1, 3))
        s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
        _check(lib().kicp_elev_integrate(self._h, p if a.size else None, a.size // 3, _pose_ptr(pose), sp, self._last.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return self.last_frame()

    def integrate_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), n=None):
        """kicp_elev_integrate_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
        count = device_frame.n if n is None else int(n)
        _check(lib().kicp_elev_integrate_device(self._h, device_frame.ptr if count else None, count, _pose_ptr(pose), sp,
                                                self._last.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return self.last_frame()

    def update(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0), margin_steps=2, widen_slabs=1, keep_ground=1):
        """kicp_elev_update: the frame as an UPDATE - the bits its rays pass through are cleared (the last margin_steps steps of a ray
        left alone, each step's slabs widened by widen_slabs, a column's lowest bit kept with keep_ground), then the frame is marked as
        integrate marks it -> integrate's six words, counted on the carved columns, then (carve_points, bits_cleared, cells_emptied)"""
        a, p = _d(np.asarray(frame, dtype=np.float64).reshape(-1, 3))
        s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
        cfg, out = ElevationCarveConfig(int(margin_steps), int(widen_slabs), int(keep_ground)), np.zeros(9, dtype=np.uint64)
        _check(lib().kicp_elev_update(self._h, p if a.size else None, a.size // 3, _pose_ptr(pose), sp, C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        self._last[:], self._last_update = out[:6], out
        return self.last_update()

    def update_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), margin_steps=2, widen_slabs=1, keep_ground=1, n=None):
        """kicp_elev_update_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
        count = device_frame.n if n is None else int(n)
        cfg, out = ElevationCarveConfig(int(margin_steps), int(widen_slabs), int(keep_ground)), np.zeros(9, dtype=np.uint64)
        _check(lib().kicp_elev_update_device(self._h, device_frame.ptr if count else None, count, _pose_ptr(pose), sp, C.byref(cfg),
                                             out.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        self._last[:], self._last_update = out[:6], out
        return self.last_update()

    def last_frame(self):
        """(used, skipped, outside_grid, outside_column, new_bits, new_cells) of the last integrated or updated frame"""
        return tuple(int(v) for v in self._last)

    def last_update(self):
        """the nine words of the last update (zeros before the first one): last_frame()'s six, then carve_points, bits_cleared,
        cells_emptied"""
        return tuple(int(v) for v in self._last_update)

    def columns(self):
        """-> uint64 (height, width): bit b of a column is set when a return ever had a world height in slab b"""
        out = np.empty((self.height, self.width), dtype=np.uint64)
        _check(lib().kicp_elev_columns(self._h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.size))
        return out

    def set_columns(self, columns):
        c = np.ascontiguousarray(columns, dtype=np.uint64)
        _check(lib().kicp_elev_set_columns(self._h, c.ctypes.data_as(C.POINTER(C.c_ulonglong)), c.size))

    def last_window(self):
        """kicp_elev_last_window: (x0, y0, w, h) of the last integrated frame's window clipped to the layer, by OccupancyGrid.last_window's
        rules; that rectangle grown by one cell is all a frame can change of the traversability"""
        v = [C.c_uint() for _ in range(4)]
        _check(lib().kicp_elev_last_window(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _traversability(self, rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, *fit):
        """what the three traversability* methods share"""
        x0, y0, w, h = _rect(rect, self.width, self.height)
        suffix, cfgs, fit_values, count_words = _elev_classes(step_slabs, robot_slabs, *fit)
        entry = getattr(lib(), "kicp_elev_traversability" + suffix)
        return _traversability_call(lambda *outs: entry(self._h, *cfgs, x0, y0, w, h, *outs), w, h, return_ground, return_fit, return_counts, fit_values, count_words)

    def _to_grid(self, grid, step_slabs, robot_slabs, *fit):
        """what the three to_grid* methods share"""
        suffix, cfgs, _, _ = _elev_classes(step_slabs, robot_slabs, *fit)
        _check(getattr(lib(), "kicp_elev_to_grid" + suffix)(self._h, *cfgs, grid._h))

    def traversability(self, step_slabs, robot_slabs, rect=None, return_ground=False, return_counts=False):
        """kicp_elev_traversability: on the GPU, traversability_from_columns' result on the columns where they are"""
        return self._traversability(rect, return_ground, False, return_counts, step_slabs, robot_slabs)

    def to_grid(self, grid, step_slabs, robot_slabs):
        """kicp_elev_to_grid: on the GPU, the classes of every cell into the counters of `grid`, an OccupancyGrid of equal cell, origin,
        width and height on the same device that the caller dedicates to it: obstacle (1, 0), traversable (0, 1), unknown (0, 0).  At
        min_observations = 1 grid.costmap, .potential, .score_arcs, .frontiers and .gain then run on traversability."""
        self._to_grid(grid, step_slabs, robot_slabs)

    def traversability_slope(self, step_slabs, robot_slabs, slope, rect=None, return_ground=False, return_fit=False, return_counts=False):
        """kicp_elev_traversability_slope: on the GPU, traversability_slope_from_columns' result on the columns where they are; a frame
        changes it only inside last_window() grown by max(1, slope.radius_cells) cells"""
        return self._traversability(rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, slope)

    def to_grid_slope(self, grid, step_slabs, robot_slabs, slope):
        """kicp_elev_to_grid_slope: to_grid with the slope limit - a SLOPE cell is an obstacle (1, 0) like a BODY or STEP one"""
        self._to_grid(grid, step_slabs, robot_slabs, slope)

    def traversability_rough(self, step_slabs, robot_slabs, slope, rough, rect=None, return_ground=False, return_fit=False, return_counts=False):
        """kicp_elev_traversability_rough: on the GPU, traversability_rough_from_columns' result on the columns where they are; a frame
        changes it only inside last_window() grown by max(1, slope.radius_cells) cells"""
        return self._traversability(rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, slope, rough)

    def to_grid_rough(self, grid, step_slabs, robot_slabs, slope, rough):
        """kicp_elev_to_grid_rough: to_grid_slope with the class ROUGH - a ROUGH cell is an obstacle (1, 0) too"""
        self._to_grid(grid, step_slabs, robot_slabs, slope, rough)

    def rough_limit(self, rms_metres):
        """elev_rough_limit for this layer's slab -> (num, den)"""
        return elev_rough_limit(self.info()["slab"], rms_metres)

    def slope_limit(self, max_tangent):
        """elev_slope_limit for this layer's cell and slab -> (rise_slabs, run_cells)"""
        info = self.info()
        return elev_slope_limit(info["cell"], info["slab"], max_tangent)


class DepthView:
    """kicp_view: a cube map of depths around the sensor, rendered from ONE frame, that tells which world points that frame sees
    through (include/kicp.h states the exact semantics); VoxelHashMap.RemoveSeenThrough(view) removes them from a map.  It owns its
    device memory; the image stays in HBM until it is asked for."""

    SEEN_THROUGH, IN_RANGE = 1, 2  # bits of a verdict

    def __init__(self, res, window, min_rays, max_ray, margin, margin_per_metre, device=0):
        self._h = None
        cfg = ViewConfig(int(res), int(window), int(min_rays), float(max_ray), float(margin), float(margin_per_metre))
        h = C.c_void_p()
        _check(lib().kicp_view_create(C.byref(cfg), int(device), C.byref(h)))
        self._h, self.device, self.res = h, device, int(res)
        self._last = np.zeros(2, dtype=np.uint64)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.kicp_view_destroy(self._h)
            self._h = None

    def info(self):
        """-> dict: the configuration's fields, sensor_world (c of the last frame, NaN before the first) and frames (rendered so far)"""
        cfg, c, frames = ViewConfig(), np.zeros(3), C.c_ulonglong()
        _check(lib().kicp_view_info(self._h, C.byref(cfg), c.ctypes.data_as(_dp), C.byref(frames)))
        out = {name: getattr(cfg, name) for name, _ in ViewConfig._fields_}
        out.update(sensor_world=c, frames=frames.value)
        return out

    def render(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0)):
        """kicp_view_render: the image of one frame of points in the base frame (host memory) at `pose`, the sensor at `sensor_xyz` in the
        base frame -> (points used, points skipped)"""
        a, p = _d(np.asarray(frame, dtype=np.float64).reshape(-1, 3))
        s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
        _check(lib().kicp_view_render(self._h, p if a.size else None, a.size // 3, _pose_ptr(pose), sp, self._last.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return self.last_frame()

    def render_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), n=None):
        """kicp_view_render_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
        count = device_frame.n if n is None else int(n)
        _check(lib().kicp_view_render_device(self._h, device_frame.ptr if count else None, count, _pose_ptr(pose), sp,
                                             self._last.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return self.last_frame()

    def last_frame(self):
        """(points used, points skipped) of the last rendered frame"""
        return tuple(int(v) for v in self._last)

    def depth(self):
        """kicp_view_depth -> float32 (6, res, res): [face, w_, u], +inf where no used point fell"""
        out = np.empty((6, self.res, self.res), dtype=np.float32)
        _check(lib().kicp_view_depth(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def classify(self, points):
        """kicp_view_classify: the verdict for world points -> uint8 per point: bit 0 (SEEN_THROUGH), bit 1 (IN_RANGE)"""
        a, p = _d(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        out = np.zeros(a.size // 3, dtype=np.uint8)
        _check(lib().kicp_view_classify(self._h, p if a.size else None, a.size // 3, out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out


class VoxelHashMap:
    """kiss_icp::VoxelHashMap: host-authoritative voxel map with an HBM mirror."""

    def __init__(self, voxel_size, max_distance, max_points_per_voxel, device=None):
        """device: preferred GPU for bulk insertions (AddPoints / Update with >= 4096 points run there); None = on the host."""
        self.voxel_size_, self.max_distance_, self.max_points_per_voxel_ = voxel_size, max_distance, max_points_per_voxel
        h = C.c_void_p()
        _check(lib().kicp_map_create(voxel_size, max_distance, max_points_per_voxel, C.byref(h)))
        self._h = h
        if device is not None:
            self.set_device(device)

    def set_device(self, device):
        _check(lib().kicp_map_set_device(self._h, -1 if device is None else int(device)))

    def copy(self):
        """VoxelHashMap(const VoxelHashMap&): a deep copy of the newest state."""
        c = VoxelHashMap.__new__(VoxelHashMap)
        c.voxel_size_, c.max_distance_, c.max_points_per_voxel_ = self.voxel_size_, self.max_distance_, self.max_points_per_voxel_
        h = C.c_void_p()
        _check(lib().kicp_map_clone(self._h, C.byref(h)))
        c._h = h
        return c

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.kicp_map_destroy(self._h)
            self._h = None

    def save_pcd(self, path):
        """The map as a PCD v0.7 file, DATA binary (kicp_map_save_pcd): Pointcloud() in its order plus a comment line with the three
        parameters.  A pending map update's error is raised here."""
        _check(lib().kicp_map_save_pcd(self._h, os.fsencode(path)))

    @staticmethod
    def load_pcd(path, voxel_size=0.0, max_distance=0.0, max_points_per_voxel=0, device=None):
        """A new map from a PCD file (kicp_map_load_pcd), its points inserted in file order - on `device` (bulk insertion) or, with None,
        on the host.  voxel_size <= 0: the parameters come from the file's `# kicp_map` line.  The new map's `points_read` and
        `points_dropped` tell how many rows the file held and how many of them were not finite."""
        m = VoxelHashMap.__new__(VoxelHashMap)
        h, read, dropped = C.c_void_p(), C.c_size_t(), C.c_size_t()
        m._h = None
        _check(lib().kicp_map_load_pcd(os.fsencode(path), float(voxel_size), float(max_distance), int(max_points_per_voxel),
                                       -1 if device is None else int(device), C.byref(h), C.byref(read), C.byref(dropped)))
        m._h = h
        vs, md, cap = C.c_double(), C.c_double(), C.c_uint()
        _check(lib().kicp_map_params(h, C.byref(vs), C.byref(md), C.byref(cap)))
        m.voxel_size_, m.max_distance_, m.max_points_per_voxel_ = vs.value, md.value, cap.value
        m.points_read, m.points_dropped = read.value, dropped.value
        return m

    def Clear(self):
        _check(lib().kicp_map_clear(self._h))

    def Empty(self):
        return bool(lib().kicp_map_empty(self._h))

    def AddPoints(self, points):
        a, p = _d(points)
        _check(lib().kicp_map_add_points(self._h, p, a.size // 3))

    def RemovePointsFarFromLocation(self, origin):
        _, p = _d(origin)
        _check(lib().kicp_map_remove_far(self._h, p))

    def Update(self, points, pose_or_origin):
        a, p = _d(points)
        b, q = _d(pose_or_origin)
        if b.size == 7:
            _check(lib().kicp_map_update_pose(self._h, p, a.size // 3, q))
        elif b.size == 3:
            _check(lib().kicp_map_update_origin(self._h, p, a.size // 3, q))
        else:
            raise ValueError("Update expects a 7-vector pose or a 3-vector origin")

    def UpdateDevice(self, device_frame, pose):
        """Update(points, pose) with the points already in HBM (DeviceFrame / PreSteps.frame); returns True if it ran on
        the GPU (table and pool growth included), False if the host map took it over: no points, or a map that holds or
        meets a voxel beyond +-2^20 voxels from the origin."""
        _, q = _d(pose)
        _check(lib().kicp_map_update_pose_device(self._h, device_frame.device, device_frame.ptr, device_frame.n, q))
        return bool(lib().kicp_map_last_update_on_device(self._h))

    def UpdateDeviceBegin(self, device_frame, pose):
        """kicp_map_update_pose_device_begin: the update's kernels are queued, nothing is waited for (UpdateFinish, or any other
        call on the map, collects it); the frame must stay alive and unchanged until then"""
        _, q = _d(pose)
        _check(lib().kicp_map_update_pose_device_begin(self._h, device_frame.device, device_frame.ptr, device_frame.n, q))

    def UpdateFinish(self):
        _check(lib().kicp_map_update_finish(self._h))
        return bool(lib().kicp_map_last_update_on_device(self._h))

    def RemoveSeenThrough(self, view):
        """kicp_map_remove_seen_through: remove every map point the frame in `view` (a DepthView) sees through -> (points in range, points
        removed, voxels that lost at least one point, voxels erased).  A pending map update is collected first."""
        out = (C.c_ulonglong * 4)()
        _check(lib().kicp_map_remove_seen_through(self._h, view._h, out))
        return tuple(int(v) for v in out)

    def device_updates(self):
        """Updates that ran on the GPU and have been collected (kicp_map_device_updates); a pending one stays pending."""
        return lib().kicp_map_device_updates(self._h)

    UPDATE_COUNTS = ("one_queue", "staged", "second_claims", "rehashes", "pool_growths", "apply_wave", "apply_thread", "wide_scans",
                     "host_updates", "deferred", "touched", "record_pieces")

    def update_counts(self):
        """Which way this map's updates went so far (kicp_map_update_counts, include/kicp.h): a dict of the twelve host-side
        counters; reads no device state and does not collect a pending update.  "record_pieces": pieces of PointcloudF32 /
        kicp_map_pointcloud_f32 calls that the device announced and the host copied (the host path and the fallback leave it alone)."""
        out = (C.c_ulonglong * 12)()
        _check(lib().kicp_map_update_counts(self._h, out))
        return dict(zip(self.UPDATE_COUNTS, out))

    def num_points(self):
        return lib().kicp_map_num_points(self._h)

    def num_voxels(self):
        return lib().kicp_map_num_voxels(self._h)

    def Pointcloud(self):
        n = self.num_points()
        out = np.empty((n, 3), dtype=np.float64)
        lib().kicp_map_pointcloud(self._h, out.ctypes.data_as(_dp), n)
        return out

    def PointcloudF32(self):
        """Pointcloud() as the published map's PointCloud2 records (kicp_map_pointcloud_f32): (n, 3) float32, static_cast<float> of
        Pointcloud(), narrowed on the GPU where the map lives there.  A pending map update's error is raised here."""
        n = C.c_size_t()
        _check(lib().kicp_map_pointcloud_f32(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.float32)
        _check(lib().kicp_map_pointcloud_f32(self._h, out.ctypes.data if n.value else None, n.value, C.byref(n)))
        return out

    def GetClosestNeighbor(self, queries, device=0):
        """Batch form of GetClosestNeighbor: (N,3) queries -> ((N,3) neighbours, (N,) distances)."""
        a, p = _d(queries)
        n = a.size // 3
        nn = np.empty((n, 3), dtype=np.float64)
        d = np.empty(n, dtype=np.float64)
        _check(lib().kicp_map_closest(self._h, device, p, n, nn.ctypes.data_as(_dp), d.ctypes.data_as(_dp)))
        return nn, d

    def check(self):
        """Number of violated table invariants on the host copy (0 = consistent); debug aid."""
        return lib().kicp_map_check(self._h)

    def sync(self, device=0):
        _check(lib().kicp_map_sync(self._h, device))

    def device_bytes(self):
        return lib().kicp_map_device_bytes(self._h)

    def last_upload(self):
        """(bytes sent by the last mirror upload, True if it was a full re-send rather than a delta)."""
        b, f = C.c_size_t(), C.c_int()
        _check(lib().kicp_map_last_upload(self._h, C.byref(b), C.byref(f)))
        return b.value, bool(f.value)


class DeviceFrame:
    """A scan resident in HBM (what an on-device pre-step would hand to the registration)."""

    def __init__(self, points, device=0):
        a, _ = _d(points)
        self.n, self.device = a.size // 3, device
        self.ptr = C.c_void_p()
        _check(lib().kicp_device_malloc(device, max(a.nbytes, 8), C.byref(self.ptr)))
        if a.nbytes:
            _check(lib().kicp_device_upload(device, self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None and not getattr(self, "_borrowed", False):
            _lib.kicp_device_free(self.device, self.ptr)
            self.ptr = None


class _Batch:
    pass


class KinematicRegistration:
    """kinematic_icp::KinematicRegistration (registration/Registration.hpp:32-50) on one MI355X."""

    def __init__(self, max_num_iteration=10, convergence_criterion=1e-3, max_num_threads=1,
                 use_adaptive_odometry_regularization=True, fixed_regularization=0.0, device=0):
        cfg = RegConfig(max_num_iteration, convergence_criterion, max_num_threads, int(use_adaptive_odometry_regularization),
                        fixed_regularization)
        h = C.c_void_p()
        _check(lib().kicp_reg_create(C.byref(cfg), device, C.byref(h)))
        self._h, self.device = h, device
        self.last_stats, self.last_status = Stats(), 0
        self._stats_ref = C.byref(self.last_stats)
        self._out = np.zeros(7, dtype=np.float64)
        self._out_p = C.cast(self._out.ctypes.data, _dp)
        self._cb = None

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.kicp_reg_destroy(self._h)
            self._h = None

    def copy(self):
        """KinematicRegistration(const KinematicRegistration &): the reference's struct is copyable (Registration.hpp:32-50);
        same parameters and tuning options, workspaces of its own (kicp_reg_clone)."""
        h = C.c_void_p()
        _check(lib().kicp_reg_clone(self._h, C.byref(h)))
        other = object.__new__(KinematicRegistration)
        other._h, other.device = h, self.device
        other.last_stats, other.last_status = Stats(), 0
        other._stats_ref = C.byref(other.last_stats)
        other._out = np.zeros(7, dtype=np.float64)
        other._out_p = C.cast(other._out.ctypes.data, _dp)
        other._cb = None
        return other

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
            rc = _lib.kicp_register_device(self._h, voxel_map._h, frame.ptr, frame.n, lp, ro, max_correspondence_distance,
                                           self._out_p, self._stats_ref)
        elif isinstance(frame, np.ndarray) and frame.dtype == np.float32:
            # float32 xyz as a PointCloud2 carries it: widened on the device (kicp_register_f32), half the bytes over PCIe
            a = np.ascontiguousarray(frame)
            rc = _lib.kicp_register_f32(self._h, voxel_map._h, a.ctypes.data, a.size // 3, lp, ro, max_correspondence_distance,
                                        self._out_p, self._stats_ref)
        else:
            a, p = _d(frame)
            rc = _lib.kicp_register(self._h, voxel_map._h, p, a.size // 3, lp, ro, max_correspondence_distance,
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
        rc = _lib.kicp_register_device_batch(self._h, voxel_map._h, batch.count, batch.ptrs, batch.ns, batch.last.ctypes.data_as(_dp),
                                             batch.rel.ctypes.data_as(_dp), max_correspondence_distance, batch.out.ctypes.data_as(_dp),
                                             batch.iterations.ctypes.data_as(C.POINTER(C.c_int)))
        self.last_status = rc if rc >= 0 else _check(rc)
        return batch.out

    def ComputeRobotMotionConcurrent(self, others, batch, voxel_map, max_correspondence_distance):
        """kicp_register_device_concurrent: the batch's INDEPENDENT scans with 1 + len(others) of them in flight, one lane per
        handle (this one and `others`).  Same poses as ComputeRobotMotionBatch, bit for bit."""
        handles = (C.c_void_p * (1 + len(others)))(self._h, *[o._h for o in others])
        rc = _lib.kicp_register_device_concurrent(handles, len(handles), voxel_map._h, batch.count, batch.ptrs, batch.ns, batch.last.ctypes.data_as(_dp),
                                                  batch.rel.ctypes.data_as(_dp), max_correspondence_distance, batch.out.ctypes.data_as(_dp),
                                                  batch.iterations.ctypes.data_as(C.POINTER(C.c_int)))
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
        ip = C.POINTER(C.c_int)
        tail = (q.ctypes.data_as(_dp), count, max_correspondence_distance, int(max_iterations), float(convergence), out.ctypes.data_as(_dp),
                iterations.ctypes.data_as(ip), status.ctypes.data_as(ip))
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
        _check(lib().kicp_occ_score_nodes(self._h, occ._h, p, a.size // 3, C.byref(window), int(level), q.ctypes.data_as(C.POINTER(C.c_ulonglong)), q.size,
                                          hits.ctypes.data_as(C.POINTER(C.c_uint))))
        return hits

    def SearchPoses(self, frame, occ, window, top_m=8):
        """kicp_search_poses: the first min(top_m, all) nodes of the window by (level-0 score descending, node index ascending), found by
        branch and bound over the pyramid -> (nodes uint64[k], hits uint32[k], poses[k, 7]).  Option "search_max_nodes" bounds the work
        (KicpError with KICP_ERR_CAPACITY beyond it); "search_nodes_scored" / "search_launches" describe the last call."""
        a, p = _d(frame)
        k = min(int(top_m), window.nodes)
        nodes, hits, poses = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint32), np.zeros((k, 7), dtype=np.float64)
        found = C.c_size_t()
        _check(lib().kicp_search_poses(self._h, occ._h, p, a.size // 3, C.byref(window), int(top_m), nodes.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                       hits.ctypes.data_as(C.POINTER(C.c_uint)), poses.ctypes.data_as(_dp), C.byref(found)))
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


class CloudLayout(C.Structure):
    """kicp_cloud_layout (include/kicp.h): where x, y, z and the per-point stamp sit inside a PointCloud2 record."""
    _fields_ = [("point_step", C.c_uint), ("offset_x", C.c_uint), ("offset_y", C.c_uint), ("offset_z", C.c_uint),
                ("stamp_datatype", C.c_int), ("offset_stamp", C.c_uint)]


FIELD_UINT32, FIELD_FLOAT32, FIELD_FLOAT64 = 6, 7, 8  # sensor_msgs::msg::PointField datatype codes


class LaserScan(C.Structure):
    """kicp_laser_scan (include/kicp.h): the sensor_msgs::msg::LaserScan fields laser_geometry's projectLaser reads."""
    _fields_ = [("angle_min", C.c_float), ("angle_max", C.c_float), ("angle_increment", C.c_float), ("time_increment", C.c_float),
                ("range_min", C.c_float), ("range_max", C.c_float)]


class PreSteps:
    """The pipeline's pre-steps on the GPU: kiss_icp::Preprocessor::Preprocess + transform_points, kiss_icp::VoxelDownsample
    (pipeline/KinematicICP.cpp:54-62).  Results live in numbered device buffers; frame(b) wraps one for ComputeRobotMotion."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().kicp_pre_create(device, C.byref(h)))
        self._h, self.device = h, device

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.kicp_pre_destroy(self._h)
            self._h = None

    def set_probe_limit(self, limit):
        """probe length at which the reference's tsl::robin_map grows its table (128: robin-map 0.6.x, default; 8192: 1.x)"""
        _check(lib().kicp_pre_set_probe_limit(self._h, int(limit)))

    def last_max_probe(self):
        """Largest robin-hood displacement the last VoxelDownsample's replay saw (kicp_pre_last_max_probe)."""
        return int(lib().kicp_pre_last_max_probe(self._h))

    def Preprocess(self, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range, deskew, dst=0):
        a, p = _d(frame)
        t, tp = _d(timestamps if timestamps is not None else np.zeros(0))
        _, r = _d(relative_motion)
        _, e = _d(lidar_to_base)
        n = C.c_size_t()
        _check(lib().kicp_pre_preprocess(self._h, p, a.size // 3, tp, t.size, r, e, max_range, min_range, int(deskew), dst, C.byref(n)))
        return n.value

    def Ingest(self, raw, n_points, point_step, offset_x, offset_y, offset_z, stamp_datatype=0, offset_stamp=0, sensor_pose=None):
        """PointCloud2 wire-format ingest (RosUtils.cpp:30-39 PointCloud2ToEigen + TimeStampHandler.cpp:57-128): ships the raw
        message bytes and decodes them on the GPU.  Returns (min_stamp, max_stamp) in seconds (0, 0 without a stamp field)."""
        buf = np.ascontiguousarray(np.frombuffer(raw, dtype=np.uint8))
        layout = CloudLayout(point_step, offset_x, offset_y, offset_z, stamp_datatype, offset_stamp)
        q = None if sensor_pose is None else _d(sensor_pose)[1]
        lo, hi = C.c_double(), C.c_double()
        _check(lib().kicp_pre_ingest(self._h, buf.ctypes.data if buf.size else None, n_points, C.byref(layout), q, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def IngestScan(self, ranges, angle_min, angle_max, angle_increment, time_increment, range_min, range_max, range_cutoff=-1.0):
        """2-D LaserScan ingest (kicp_pre_ingest_scan): laser_geometry's projectLaser(scan, cloud, range_cutoff, Timestamp) of the
        2-D node (online_node.cpp:44-58) on the GPU, then what Ingest does with the projected cloud.  `ranges`: msg.ranges (float32).
        Returns (min_stamp, max_stamp) of the kept beams in seconds (0, 0 when none was kept)."""
        r = np.ascontiguousarray(ranges, dtype=np.float32).ravel()
        scan = LaserScan(angle_min, angle_max, angle_increment, time_increment, range_min, range_max)
        lo, hi = C.c_double(), C.c_double()
        _check(lib().kicp_pre_ingest_scan(self._h, r.ctypes.data if r.size else None, r.size, C.byref(scan), float(range_cutoff),
                                          C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def IngestAhead(self, raw, n_points, point_step, offset_x, offset_y, offset_z, stamp_datatype=0, offset_stamp=0, sensor_pose=None):
        """kicp_pre_ingest_ahead: announce the NEXT message (`raw` must be a buffer whose memory the later Ingest call passes again - a
        numpy uint8 array); it is uploaded and decoded by the next Frame() call on the current one."""
        buf = np.ascontiguousarray(np.frombuffer(raw, dtype=np.uint8))
        layout = CloudLayout(point_step, offset_x, offset_y, offset_z, stamp_datatype, offset_stamp)
        q = None if sensor_pose is None else _d(sensor_pose)[1]
        self._ahead_keep = (buf, raw)  # (borrowed by the backend until the Ingest call for the same bytes)
        _check(lib().kicp_pre_ingest_ahead(self._h, buf.ctypes.data if buf.size else None, n_points, C.byref(layout), q))

    def set_option(self, name, value):
        _check(lib().kicp_pre_set_option(self._h, name.encode(), float(value)))

    def get_option(self, name):
        return float(lib().kicp_pre_get_option(self._h, name.encode()))

    def ahead_hits(self):
        return int(lib().kicp_pre_ahead_hits(self._h))

    def PreprocessIngested(self, relative_motion, lidar_to_base, max_range, min_range, deskew, dst=0):
        _, r = _d(relative_motion)
        _, e = _d(lidar_to_base)
        n = C.c_size_t()
        _check(lib().kicp_pre_preprocess_ingested(self._h, r, e, max_range, min_range, int(deskew), dst, C.byref(n)))
        return n.value

    def ingested(self):
        """(xyz (n,3) fp64, normalised stamps (n,) or None): what PointCloud2ToEigen / ProcessTimestamps hand to RegisterFrame."""
        n, has = C.c_size_t(), C.c_int()
        _check(lib().kicp_pre_ingested(self._h, None, None, 0, C.byref(n), C.byref(has)))
        xyz, st = np.empty((n.value, 3)), np.empty(n.value)
        _check(lib().kicp_pre_ingested(self._h, xyz.ctypes.data_as(_dp), st.ctypes.data_as(_dp), n.value, C.byref(n), C.byref(has)))
        return xyz, (st if has.value else None)

    def _frame(self, dtype, entry, entry_ingested, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range, deskew, voxel_a, voxel_b, want_frame):
        """Frame / FrameF32: the chained pre-steps through `entry` (or `entry_ingested`, frame=None), the preprocessed frame landing in
        an (n, 3) array of `dtype`."""
        _, r = _d(relative_motion)
        _, e = _d(lidar_to_base)
        counts = (C.c_size_t * 3)()
        f64 = dtype is np.float64
        if frame is None:
            n_in = lib().kicp_pre_ingested_count(self._h)
        else:
            a, p = _d(frame)
            t, tp = _d(timestamps if timestamps is not None else np.zeros(0))
            n_in = a.size // 3
        out = np.empty((n_in, 3), dtype=dtype) if want_frame else None
        landing = (out.ctypes.data_as(_dp) if f64 else out.ctypes.data) if want_frame and n_in else None
        tail = (r, e, max_range, min_range, int(deskew), voxel_a, voxel_b, landing, n_in, counts)
        rc = entry_ingested(self._h, *tail) if frame is None else entry(self._h, p, n_in, tp, t.size, *tail)
        if rc < 0:
            message = lib().kicp_last_error().decode(errors="replace")
            if want_frame and n_in:  # the backend's helper thread may hold a pointer into `out`: collect (and drop) the download before the array can go
                lib().kicp_pre_download_finish(self._h, 0, None, 0, None)
            raise KicpError(rc, message)
        self.last_status = rc
        if want_frame and n_in:
            n = C.c_size_t()  # (FLOAT32 records land in `out` only: collected with NULL)
            _check(lib().kicp_pre_download_finish(self._h, 0, landing if f64 else None, n_in if f64 else 0, C.byref(n)))
            out = out[:counts[0]]
        return [int(c) for c in counts], out

    def Frame(self, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range, deskew, voxel_a, voxel_b, want_frame=True):
        """kicp_pre_frame / kicp_pre_frame_ingested (frame=None: the ingested cloud): Preprocess + the two downsamples behind one
        synchronisation.  Returns (counts, preprocessed frame or None)."""
        return self._frame(np.float64, lib().kicp_pre_frame, lib().kicp_pre_frame_ingested, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range,
                           deskew, voxel_a, voxel_b, want_frame)

    def FrameF32(self, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range, deskew, voxel_a, voxel_b, want_frame=True):
        """kicp_pre_frame_f32 / kicp_pre_frame_ingested_f32: Frame() with the preprocessed frame returned as PointCloud2 records, (n, 3)
        float32 narrowed on the GPU (want_frame=False: nothing is pushed).  Returns (counts, records or None); download_f32(2) then
        reads the keypoints' records."""
        return self._frame(np.float32, lib().kicp_pre_frame_f32, lib().kicp_pre_frame_ingested_f32, frame, timestamps, relative_motion, lidar_to_base, max_range,
                           min_range, deskew, voxel_a, voxel_b, want_frame)

    def download_f32(self, buffer):
        """kicp_pre_download_f32: a buffer as PointCloud2 records, (n, 3) float32"""
        n = C.c_size_t()
        _check(lib().kicp_pre_download_f32(self._h, buffer, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.float32)
        _check(lib().kicp_pre_download_f32(self._h, buffer, out.ctypes.data if n.value else None, n.value, C.byref(n)))
        return out

    def VoxelDownsample(self, src, voxel_size, dst):
        n = C.c_size_t()
        self.last_status = _check(lib().kicp_pre_voxel_downsample(self._h, src, voxel_size, dst, C.byref(n)))  # KICP_WARN_TABLE_ORDER: see kicp.h
        return n.value

    def upload(self, buffer, points):
        a, p = _d(points)
        _check(lib().kicp_pre_upload(self._h, buffer, p, a.size // 3))

    def download(self, buffer):
        n = C.c_size_t()
        _check(lib().kicp_pre_download(self._h, buffer, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.float64)
        _check(lib().kicp_pre_download(self._h, buffer, out.ctypes.data_as(_dp), n.value, C.byref(n)))
        return out

    def download_begin(self, buffer):
        """Start copying a buffer to the host in the background; collect it with download_finish."""
        _check(lib().kicp_pre_download_begin(self._h, buffer))

    def download_finish(self, buffer):
        n = C.c_size_t()
        _check(lib().kicp_pre_download(self._h, buffer, None, 0, C.byref(n)))  # (size only)
        out = np.empty((n.value, 3), dtype=np.float64)
        _check(lib().kicp_pre_download_finish(self._h, buffer, out.ctypes.data_as(_dp), n.value, C.byref(n)))
        return out[:n.value]

    def frame(self, buffer):
        """A DeviceFrame view of a buffer (no copy; valid until the buffer is overwritten)."""
        n = C.c_size_t()
        ptr = lib().kicp_pre_device_ptr(self._h, buffer, C.byref(n))
        f = DeviceFrame.__new__(DeviceFrame)
        f.n, f.device, f.ptr, f._borrowed = n.value, self.device, C.c_void_p(ptr), True
        return f


def comm_unique_id():
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().kicp_comm_unique_id(buf))
    return buf.raw
