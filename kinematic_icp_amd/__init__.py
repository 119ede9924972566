"""kinematic_icp_amd -- MI355X-native backend of the kinematic-ICP registration hot path.

Python mirror of the reference's operator interface for this path, bound with ctypes to the C-ABI of
include/kicp.h (libkicp_amd.so, hand-written HIP for gfx950):

    kinematic_icp::KinematicRegistration   /root/reference/cpp/kinematic_icp/registration/Registration.hpp:32-50
    kiss_icp::VoxelHashMap (v1.2.0)        call sites Registration.cpp:63,74,157; KinematicICP.hpp:79,88,92; KinematicICP.cpp:79

Names, argument order and argument meaning follow the reference.  Poses are 7-vectors
[qx, qy, qz, qw, tx, ty, tz] (Sophus::SE3d parameter order); point clouds are (N, 3) float64 arrays.

There is NO CPU fallback: importing works anywhere, but creating a KinematicRegistration (or running any
device operation) without the built extension or without a visible gfx950 device raises KicpError.

The binding is one module per feature, cut as the C side's files are (DESIGN.md has the table); every name is re-exported here.
Every feature module is imported below, so the signature table is complete before lib() can first be called.  The loaded library
itself is `_ffi._lib` and is not re-exported: a copy made at import would stay None.
"""
from . import _ffi, device, elevation, explore, grid, plan, presteps, registration, search, transients, view, voxel_map  # noqa: F401
from ._ffi import (KICP_ERR_ARG, KICP_ERR_CAPACITY, KICP_ERR_COMM, KICP_ERR_HIP, KICP_ERR_INTERNAL, KICP_OK, KICP_WARN_NO_CORRESPONDENCES,  # noqa: F401
                   KICP_WARN_TABLE_ORDER, LIB_PATH, KicpError, lib)
from ._ffi import (_HERE, _PTR_CACHE, _SIGNATURES, _check, _d, _dp, _occupancy_2d, _out_array, _pose_ptr, _rect, _u8, _u32)  # noqa: F401
from .device import ALLREDUCE_FN, COMM_ID_BYTES, DeviceFrame, comm_unique_id, cpus_near_gpu, device_count, device_locality, probe_dependent_load  # noqa: F401
from .elevation import (ElevationCarveConfig, ElevationConfig, ElevationLayer, ElevationRoughConfig, ElevationSlopeConfig,  # noqa: F401
                        ElevationTraversabilityConfig, elev_rough_limit, elev_slope_limit, elev_update_columns, traversability_from_columns,
                        traversability_rough_from_columns, traversability_slope_from_columns)
from .elevation import _elev_classes, _struct, _traversability_call, _traversability_from_columns  # noqa: F401
from .explore import FRONTIER_WORDS, GAIN_WORDS, FrontierConfig, GainConfig, frontiers_from_occupancy, gain_from_occupancy  # noqa: F401
from .explore import _frontier_call, _frontier_config, _gain_config, _gain_views  # noqa: F401
from .grid import (GridClearanceConfig, GridConfig, GridFillConfig, OccupancyGrid, clearance_from_occupancy, costmap_from_occupancy,  # noqa: F401
                   fill_unknown_counts, follow_shift, nav2_cost_table, occupancy_from_counts, shift_plane, write_map)
from .grid import _clearance_config, _cost_table, _table_radius  # noqa: F401
from .plan import (ARC_TREE_MAX_DEPTH, ARC_TREE_MAX_NODES, ARC_TREE_MAX_T, ARCS_MAX_K, ARCS_MAX_P, ARCS_MAX_T, MAX_POTENTIAL, UNREACHED,  # noqa: F401
                   PlanConfig, arc_start, arc_steps, arc_tree_best, arc_tree_nodes, arcs_best, footprint_box, plan_q, plan_weights,
                   potential_from_costmap, potential_path, score_arc_tree_from_plan, score_arcs_from_plan)
from .plan import _arc_tree_args, _arc_tree_levels, _arcs_args, _plan_args, _potential_out, _potential_result  # noqa: F401
from .presteps import FIELD_FLOAT32, FIELD_FLOAT64, FIELD_UINT32, CloudLayout, LaserScan, PreSteps  # noqa: F401
from .registration import MAX_LOG_PASSES, P2P_HANDLE_BYTES, KinematicRegistration, RegConfig, Stats, _Batch, planar_grid, planar_step  # noqa: F401
from .search import OccupancyPyramid, SearchWindow, search_window_around, search_yaws  # noqa: F401
from .transients import TRANSIENT_WORDS, TransientConfig, transients_from_counts  # noqa: F401
from .transients import _transient_call, _transient_config  # noqa: F401
from .view import DepthView, ViewConfig  # noqa: F401
from .voxel_map import VoxelHashMap  # noqa: F401
