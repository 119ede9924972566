"""The case table of the relocalisation kernels' regime tests, shared by tests/test_reloc_cases.py (CPU: the premises of every case,
from numpy and the oracle alone) and tests/test_gpu_reloc_regimes.py (GPU: kicp_score.hpp k_score_poses, kicp_planar.hpp
k_planar_poses and the batch / launch loops of kicp_score.hip; kicp_search.hpp k_occ_mark, k_occ_pool, k_search_cells, k_search_score
and the piece loop of kicp_search.hip).  Nothing here calls the GPU.

Score / planar cases: a long pose list is poses[order] of 300 DISTINCT poses, so its expected rows are reference[order] and the
reference is computed once per frame size at 300 poses.  More than 30 % of the 300 lie 500 m away (no correspondence at all), at
random positions: a workgroup that strides over (tile, pose) items meets items with and without correspondences in turn, on either
of its two LDS sets.  The table states the item arithmetic of kicp_score.hip as the GPU test expects to read it from the handle's
read-only counters ("score_launches", "score_items_per_workgroup") - never from the constants themselves.

Pyramid cases: sparse maps (28 points) whose rows are 17, 17, 18, 19 and 3 words long, so that at levels 7 .. 10 (shifts of 2, 4, 8,
16 whole words) cells exist that are set ONLY through the x shift, and others ONLY through the y shift; two maps with dilate 3 and 4
whose 7- and 9-bit runs cross (or just touch) a word boundary, the runs isolated in their row.

Search cases: over cfg4's map (tests/search_cases.py), pyramids with 4 and with 10 levels."""
import collections
import functools

import numpy as np

import kinematic_icp_amd as K
from kinematic_icp_amd import synthetic as syn
from oracle import okicp
import search_cases as sc
import search_ref as sr

DISTINCT = 300   # poses of the pose set
STRIDE = 2048    # order[k] != order[k + STRIDE]: the items a workgroup of a 2 048-workgroup launch serves in turn belong to different poses
FAR_M = 500.0


# ---- one frame at many poses -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_scene():
    """-> (cfg, the oracle's map, keypoints, scan): cfg1's map and the keypoints of its first scan, as tests/test_gpu_score_poses.py
    builds them"""
    cfg, scene, scans, rng = syn.make_case("cfg1", n_scans=2)
    omap = okicp.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    syn.build_map_points(scene, cfg, omap.AddPoints, omap.num_points, rng)
    keypoints = okicp.voxel_downsample(okicp.voxel_downsample(scans[0]["frame"], cfg.voxel_size * 0.5), cfg.voxel_size * 1.5)
    keypoints.setflags(write=False)
    return cfg, omap, keypoints, scans[0]


def pose_set(scan, count=DISTINCT, seed=11):
    """-> (poses[count, 7], far[count] bool): the guess, the truth, then planar offsets of the guess up to 2 m / 20 degrees; those
    marked far (more than 30 %, at random positions) lie 500 m further along x.  All poses differ."""
    rng = np.random.default_rng(seed)
    guess = syn.pose_mul(scan["last_pose"], scan["rel_odom"])
    far = rng.random(count) < 0.36
    far[:2] = False
    poses = [guess, scan["true_pose"]]
    for k in range(2, count):
        x, y, yaw = rng.uniform(-2, 2), rng.uniform(-2, 2), np.deg2rad(rng.uniform(-20, 20))
        poses.append(syn.pose_mul(guess, syn.planar_pose(x + (FAR_M if far[k] else 0.0), y, yaw)))
    poses = np.array(poses)
    poses.setflags(write=False), far.setflags(write=False)
    return poses, far


def pose_order(count, seed, distinct=DISTINCT):
    """an index array of length count >= distinct into the pose set: every index at least once, the rest drawn with repetition, shuffled"""
    rng = np.random.default_rng(seed)
    order = np.concatenate([np.arange(distinct), rng.integers(0, distinct, count - distinct)])
    rng.shuffle(order)
    return order


def differs_at_stride(order):
    """the fraction of k with order[k] != order[(k + STRIDE) mod count]: items are numbered tile-major (item = tile * count + pose), so
    the item STRIDE further on has the pose (k + STRIDE) mod count - also where the list is shorter than STRIDE"""
    return float((order != np.roll(order, -STRIDE)).mean())


ScoreCase = collections.namedtuple("ScoreCase", "name n count score_chunk seed items_per_workgroup launches")
# (items_per_workgroup: what "score_items_per_workgroup" must at least report; launches: (how, value) for "score_launches")
SCORE_CASES = [
    # 3 tiles x 1 500 poses = 4 500 items: some workgroups serve three, so an LDS set is used a second time
    ScoreCase("stride_3", 513, 1500, None, 1, 3, ("==", 1)),
    ScoreCase("stride_full_tiles", 512, 1100, None, 2, 2, ("==", 1)),
    ScoreCase("stride_one_point", 1, 2300, None, 3, 2, ("==", 1)),  # one live lane per workgroup
    # launches of 2 100, 2 100 and 300 items: item0 = 2 100 lies inside tile 1 (1 500 .. 2 999), not on a tile's first pose
    ScoreCase("split_and_stride", 513, 1500, 2100 * 256, 4, 2, ("==", 3)),
    ScoreCase("two_batches", 65, 65536 + 300, None, 5, 2, (">=", 2)),
    # (the name the case was given; 2 x 65 536 poses are two FULL batches: the last one is full and the loop must not begin another)
    ScoreCase("three_batches_exact", 1, 2 * 65536, None, 6, 2, (">=", 2)),
]
SMALL_CASE = ScoreCase("two_tiles_seven_poses", 257, 7, None, 0, 1, ("==", 1))  # what the suite covered before: one item per workgroup
REFINE_N, REFINE_STARTS, REFINE_SLICE, REFINE_ITERATIONS = 257, 2300, 400, 5


def score_order(case):
    return pose_order(case.count, 100 + case.seed)


def refine_order(far):
    """indices into the pose set for the refinement under stride: REFINE_STARTS of the near poses, every one at least once"""
    near = np.flatnonzero(~far)
    return near[pose_order(REFINE_STARTS, 77, len(near))]


# ---- pyramids ------------------------------------------------------------------------------------------------------------------------
PYRAMID_CELL = 0.25  # exact in binary
SPARSE_LEVELS, SPARSE_DIMS_Y = 10, 600
SparseMap = collections.namedtuple("SparseMap", "dims_x seed ask_x")
# dims.x: 17, 17, 18 and 19 words per row; 70: the x shift leaves the row from s = 128 on, the y shift does not
SPARSE_MAPS = [SparseMap(543, 1, True), SparseMap(544, 1, True), SparseMap(545, 1, True), SparseMap(577, 1, True), SparseMap(70, 1, False)]
DilateMap = collections.namedtuple("DilateMap", "dilate seed")
DILATE_MAPS = [DilateMap(3, 1), DilateMap(4, 1)]
DILATE_LEVELS = 6
EDGE_X = (28, 29, 30, 31, 32, 33, 34, 35)  # cells whose x mod 32 is 28 .. 31, 0 .. 3: runs around the boundary between words 0 and 1
_DILATE_SPAN = (36, 78, 60)  # the points' extent in cells


@functools.lru_cache(maxsize=None)
def sparse_points(case):
    """28 points: the four corners of the xy box (dims = extent in cells + 3 with dilate 0: tests/search_ref.py geometry) in the lower
    of the two z slices, and 24 random ones in either"""
    cell, kx, ky = PYRAMID_CELL, case.dims_x - 3, SPARSE_DIMS_Y - 3
    rng = np.random.default_rng(1000 * case.dims_x + case.seed)
    lo, hi = np.array([0.5 * cell, 0.5 * cell, 0.5 * cell]), np.array([(kx + 0.5) * cell, (ky + 0.5) * cell, 1.5 * cell])
    corners = np.array([[x, y, 0.5 * cell] for x in (lo[0], hi[0]) for y in (lo[1], hi[1])])
    pts = np.vstack([corners, rng.uniform(lo, hi, (24, 3))])
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def dilate_points(case):
    """300 points over 36 x 78 x 60 cells (many z slices: a slice sees only the points within `dilate` of it, so level 0 does not
    saturate); eight of them sit in the cells EDGE_X, each alone in its neighbourhood (tests/test_reloc_cases.py checks that)"""
    cell, d = PYRAMID_CELL, case.dilate
    rng = np.random.default_rng(50 * d + case.seed)
    span = np.array(_DILATE_SPAN, dtype=np.float64)
    pts = rng.uniform(0.5 * cell, (span - np.array([0.0, 26.0, 0.0]) + 0.5) * cell, (300, 3))  # rows 0 .. 52 of the box
    pts[0], pts[1] = 0.5 * cell, (span + 0.5) * cell  # the box
    for k, cx in enumerate(EDGE_X):  # cell cx of the grid is cell cx - (d + 1) of the box; rows 62 and 74, slices 4, 18, 32, 46: more than 2 d apart
        pts[2 + k] = (np.array([cx - (d + 1), 62 + 12 * (k % 2), 4 + 14 * (k // 2)]) + 0.5) * cell
    pts.setflags(write=False)
    return pts


def only_through(prev, s):
    """of level h = the pool of `prev` (level h - 1, bool [z, y, x]) with shift s: how many cells are set only through the x shift
    (not in prev, not reached by the y shift or the diagonal), how many only through the y shift -> (x_only, y_only)"""
    dz, dy, dx = prev.shape
    sx, syx, sy = np.zeros_like(prev), np.zeros_like(prev), np.zeros_like(prev)
    if s < dx:
        sx[:, :, :-s] = prev[:, :, s:]
    if s < dy:
        sy[:, :-s, :] = prev[:, s:, :]
    if s < dx and s < dy:
        syx[:, :-s, :-s] = prev[:, s:, s:]
    return int((sx & ~prev & ~sy & ~syx).sum()), int((sy & ~prev & ~sx & ~syx).sum())


# ---- search --------------------------------------------------------------------------------------------------------------------------
SEARCH_NAME = "cfg4"
SEARCH_CELL = sc.CELL[SEARCH_NAME]
DEEP_LEVELS = 10
PIECE = 1 << 20  # the node lists are 2^20 + 3 and 2 x 2^20 long, one of 2^20 for comparison


@functools.lru_cache(maxsize=None)
def search_scene():
    """-> (cfg, the oracle's map, keypoints of scan 0 (250), truth, min, dims, the restatement's levels 0 .. 10)"""
    cfg, omap, items = sc.case(SEARCH_NAME)
    keypoints, truth, _ = items[0]
    mn, dims, levels = sr.pyramid(omap.Pointcloud(), SEARCH_CELL, sc.DILATE, DEEP_LEVELS)
    return cfg, omap, keypoints, truth, mn, dims, levels


def _around(truth, nx, ny, yaw0, yaw_step, nyaw):
    cell = SEARCH_CELL
    return K.SearchWindow(truth[4] - (nx // 2) * cell, truth[5] - (ny // 2) * cell, truth[6], nx, ny, yaw0, yaw_step, nyaw)


def windows_inside_and_corners():
    """the windows of tests/test_gpu_search.py _windows: inside the map; over the grid's low corner; over its high corner"""
    cfg, omap, keypoints, truth, mn, dims, levels = search_scene()
    cell, hi = SEARCH_CELL, mn + dims * SEARCH_CELL
    return [K.SearchWindow(truth[4] - 10 * cell, truth[5] - 8 * cell, truth[6], 21, 17, -0.4, 0.13, 7),
            K.SearchWindow(mn[0] - 9 * cell, mn[1] - 11 * cell, truth[6], 40, 33, 1.0, 0.7, 7),
            K.SearchWindow(hi[0] - 20 * cell, hi[1] - 15 * cell, truth[6] + 3 * cell, 35, 40, 2.9, 0.0, 1)]


MANY_YAWS = 2053  # two full trips of 1 024 yaws and a rest of 5
MANY_YAWS_PICKED = (0, 1023, 1024, 1025, 2047, 2048, 2052)


def many_yaws():
    """-> (frame (65 keypoints), window 9 x 7 x 2 053, nodes: all 63 of each picked yaw and 2 000 random ones)"""
    cfg, omap, keypoints, truth, mn, dims, levels = search_scene()
    window = _around(truth, 9, 7, -np.pi, 2.0 * np.pi / MANY_YAWS, MANY_YAWS)
    rng = np.random.default_rng(2053)
    nodes = np.concatenate([j * 63 + np.arange(63) for j in MANY_YAWS_PICKED] + [rng.integers(0, window.nodes, 2000)])
    return keypoints[:65], window, nodes


def few_yaws():
    """the 180-yaw window of the same extent: one trip"""
    cfg, omap, keypoints, truth, mn, dims, levels = search_scene()
    return _around(truth, 9, 7, -np.pi, 2.0 * np.pi / 180, 180)


def restated_scores(frame, window, h, nodes=None):
    """the restatement's scores of `nodes` (None: every node of the window, shaped [nyaw, ny, nx]; level 0 only) against level h"""
    cfg, omap, keypoints, truth, mn, dims, levels = search_scene()
    cells = sr.frame_cells(frame, K.search_yaws(window), window, mn, SEARCH_CELL)
    if nodes is None:
        assert h == 0
        return sr.score_window(levels[0], cells, window)
    return sr.score_nodes(levels[h], cells, window, nodes, h=h)


@functools.lru_cache(maxsize=None)
def many_nodes():
    """-> (frame (65 keypoints), window 21 x 17 x 7, the restatement's exhaustive level-0 scores [2 499], {length: node list}): the lists
    are drawn with repetition, hold every node at least once, and their entries 2^20 - 1, 2^20, 2^20 + 1 are three nodes with three
    different scores"""
    cfg, omap, keypoints, truth, mn, dims, levels = search_scene()
    frame, window = keypoints[:65], windows_inside_and_corners()[0]
    scores = restated_scores(frame, window, 0).reshape(-1)
    values, first = np.unique(scores, return_index=True)
    assert len(values) >= 3
    three = first[-3:]  # the first nodes with the three highest scores
    lists = {}
    for length in (PIECE, PIECE + 3, 2 * PIECE):
        rng = np.random.default_rng(length % 1000)
        nodes = np.concatenate([np.arange(window.nodes), rng.integers(0, window.nodes, length - window.nodes)])
        rng.shuffle(nodes)
        if length > PIECE:
            at = np.arange(PIECE - 1, PIECE + 2)
            for k, node in zip(at, three):  # swap the three into place: the list still holds every node
                other = np.flatnonzero(nodes == node)[0]
                nodes[other], nodes[k] = nodes[k], nodes[other]
        lists[length] = nodes.astype(np.uint64)
    return frame, window, scores, lists


def deep_windows():
    """-> (corner 40 x 33 x 7 over the grid's low corner, the same 1 100 cells lower in x and y, 8 x 8 x 1 100 around the truth: smaller
    than a top block of any level >= 3, more yaws than one trip)"""
    cfg, omap, keypoints, truth, mn, dims, levels = search_scene()
    corner = windows_inside_and_corners()[1]
    cell = SEARCH_CELL
    lower = K.SearchWindow(corner.x0 - 1100 * cell, corner.y0 - 1100 * cell, corner.z, 40, 33, 1.0, 0.7, 7)
    small = _around(truth, 8, 8, -np.pi, 2.0 * np.pi / 1100, 1100)
    return corner, lower, small


def deep_nodes(window):
    """the nodes the levels above 4 are compared at: the first node of every yaw (the top blocks), the last node, 600 random ones"""
    rng = np.random.default_rng(10)
    return np.concatenate([(np.arange(window.nyaw) * window.ny) * window.nx, [window.nodes - 1], rng.integers(0, window.nodes, 600)])


NOT_FINITE_ROWS = ((0, 0, np.nan), (1, 1, np.inf), (63, 2, -np.inf), (64, 0, 1e300), (127, 1, -1e300), (128, 2, np.nan), (200, 0, -np.inf), (249, 2, 1e300))


def not_finite():
    """-> (the 250 keypoints with 8 rows made not finite or 1e300 away in x, y or z, the same frame without those rows, the rows)"""
    cfg, omap, keypoints, truth, mn, dims, levels = search_scene()
    frame = np.array(keypoints)
    assert len(frame) == 250
    for row, axis, value in NOT_FINITE_ROWS:
        frame[row, axis] = value
    rows = np.array([r for r, _, _ in NOT_FINITE_ROWS])
    return frame, np.delete(np.array(keypoints), rows, axis=0), rows


def outside_windows():
    """-> (a window 5 000 cells beyond the grid's high corner in x, the inside window with z 50 cells above the grid)"""
    cfg, omap, keypoints, truth, mn, dims, levels = search_scene()
    cell, hi = SEARCH_CELL, mn + dims * SEARCH_CELL
    beyond = K.SearchWindow(hi[0] + 5000 * cell, truth[5] - 8 * cell, truth[6], 21, 17, -0.4, 0.13, 7)
    above = K.SearchWindow(truth[4] - 10 * cell, truth[5] - 8 * cell, hi[2] + 50 * cell, 21, 17, -0.4, 0.13, 7)
    return beyond, above
