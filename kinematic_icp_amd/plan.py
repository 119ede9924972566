"""Planning over a costmap as pure host code (kicp_plan_*, kicp_potential_*, kicp_arc*, kicp_footprint_box, kicp_score_arc*_from_plan):
the cost-to-go field and its path, fans and trees of arc trajectories scored on it.  OccupancyGrid's methods of the same names run
them on the GPU and take their argument checks from here."""
import ctypes as C
import math

import numpy as np

from ._ffi import (KICP_ERR_ARG, KICP_ERR_CAPACITY, KicpError, _check, _d, _declare, _dp, _out_array, _szp, _u8, _u8p, _u32, _u32p, _u64,
                   _u64p, lib)


class PlanConfig(C.Structure):
    """kicp_plan_config: potentials are clamped at max_potential (1 .. 0xFFFFFFFE), which doubles as a planning horizon"""
    _fields_ = [("max_potential", C.c_uint)]


_u, _f64, _sz = C.c_uint, C.c_double, C.c_size_t

_ENTRIES = _declare({
    "kicp_plan_weights": (C.c_int, [_u, _u, _u, _u, _u, _u8p]),
    "kicp_potential_from_costmap": (C.c_int, [_u8p, _u, _u, _u8p, C.POINTER(PlanConfig), _u32p, _sz, _u32p, _sz, _u64p]),
    "kicp_potential_path": (C.c_int, [_u32p, _u8p, _u, _u, _u8p, _u, _u, _u32p, _sz, _szp]),
    "kicp_plan_q": (C.c_int, [_u8p, _sz, _u8p, _u8p]),
    "kicp_arc_steps": (C.c_int, [_dp, _dp, _f64, _sz, _dp]),
    "kicp_footprint_box": (C.c_int, [_f64, _f64, _f64, _f64, _f64, _dp, _sz, _szp]),
    "kicp_arcs_best": (C.c_int, [_u32p, _sz, _u, _u, _u, _u, _u, _szp]),
    "kicp_score_arcs_from_plan": (C.c_int, [_u8p, _u32p, _f64, _f64, _f64, _u, _u, _dp, _dp, _sz, _u, _dp, _sz, _u32p, _sz]),
    "kicp_arc_tree_nodes": (C.c_int, [_u, _u32p, _u32p, _szp, _szp, _u32p, _szp]),
    "kicp_arc_tree_best": (C.c_int, [_u32p, _u, _u32p, _u32p, _u, _u, _u, _u, _szp, _u32p]),
    "kicp_score_arc_tree_from_plan": (C.c_int, [_u8p, _u32p, _f64, _f64, _f64, _u, _u, _dp, _u, _u32p, _u32p, _dp, _dp, _sz, _u32p, _sz]),
})

MAX_POTENTIAL = 0xFFFFFFFE
UNREACHED = 0xFFFFFFFF


def plan_weights(neutral=50, factor_num=4, factor_den=5, lethal_from=253, unknown_weight=0):
    """kicp_plan_weights: weight[256] for the potential, uint8: min(255, neutral + b * factor_num / factor_den) for a cost b < lethal_from,
    0 (impassable) from lethal_from to 254, unknown_weight for 255 (0 keeps the planner out of unknown space).  The defaults are NavFn's."""
    args = [int(v) for v in (neutral, factor_num, factor_den, lethal_from, unknown_weight)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "the arguments of plan_weights are unsigned 32-bit integers")
    out = np.empty(256, dtype=np.uint8)
    _check(lib().kicp_plan_weights(*args, _u8(out)))
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
    _check(lib().kicp_potential_from_costmap(_u8(cm), cm.shape[1], cm.shape[0], _u8(wt), C.byref(cfg), _u32(g), len(g), _u32(out), out.size, _u64(stats)))
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


def _plan_pair(q, potential):
    """-> (q uint8, potential uint32), both (height, width): the plan the *_from_plan functions take"""
    qa, pot = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(potential, dtype=np.uint32)
    if qa.ndim != 2 or qa.size == 0 or pot.shape != qa.shape:
        raise KicpError(KICP_ERR_ARG, "q and the potential must be shaped (height, width), both at least 1")
    return qa, pot


def score_arcs_from_plan(q, potential, cell, origin_x, origin_y, start, arcs, n_steps, footprint, out=None):
    """kicp_score_arcs_from_plan: every arc of `arcs` (K, 4) rolled n_steps poses forward from `start` = (x, y, cosine, sine) with the
    footprint's samples (P, 2) laid on q (uint8 (height, width), 0 impassable: plan_q makes it) at every pose -> uint32 (K, 4):
    free_steps, cost_sum, cost_max, end_potential (the potential at the last free pose; 0xFFFFFFFF outside the grid).  out: a uint32
    (K, 4) array to write into.  Pure host code: needs no GPU."""
    qa, pot = _plan_pair(q, potential)
    s, a, f, n_steps = _arcs_args(start, arcs, n_steps, footprint)
    out = _out_array(out, (len(a), 4), np.uint32, "(K, 4)")
    _check(lib().kicp_score_arcs_from_plan(_u8(qa), _u32(pot), float(cell), float(origin_x), float(origin_y), qa.shape[1], qa.shape[0], _d(s)[1], _d(a)[1],
                                           len(a), n_steps, _d(f)[1], len(f), _u32(out), out.size))
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
        raise KicpError(KICP_ERR_ARG, "the primitives must be shaped (sum of branch, 4) = (%d, 4): dx, dy, dc, ds, level 1's rows first"
                        % int(b.sum(dtype=np.uint64)))
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
    qa, pot = _plan_pair(q, potential)
    s, b, st, p, f, n_nodes = _arc_tree_args(start, branch, steps, primitives, footprint)
    out = _out_array(out, (n_nodes, 4), np.uint32, "(N, 4) = (%d, 4)" % n_nodes)
    _check(lib().kicp_score_arc_tree_from_plan(_u8(qa), _u32(pot), float(cell), float(origin_x), float(origin_y), qa.shape[1], qa.shape[0], _d(s)[1],
                                               b.size, _u32(b), _u32(st), _d(p)[1], _d(f)[1], len(f), _u32(out), out.size))
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
