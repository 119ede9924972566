"""The premises of tests/reloc_cases.py, proved on the CPU with numpy and the oracle alone, so that the regime each case of
tests/test_gpu_reloc_regimes.py claims is a property of its input: the pose set does mix poses with and without correspondences and
the long lists' orders put different poses on the items a workgroup serves in turn; the sparse pyramid maps have, at every level
7 .. 10, cells that only the x shift sets and cells that only the y shift sets (a lost shift changes the level); the dilated runs
cross the word boundary, alone in their row; the node lists straddle a piece with three distinguishable nodes; the frame rows that are
not finite are far at every yaw; and no search case passes on all-zero scores except the two that must."""
import numpy as np
import pytest

import kinematic_icp_amd as K
from oracle import okicp
import reloc_cases as rc
import search_cases as sc
import search_ref as sr


# ---- the pose set ------------------------------------------------------------------------------------------------------------------
def test_pose_set_mixes_poses_with_and_without_correspondences():
    cfg, omap, keypoints, scan = rc.score_scene()
    poses, far = rc.pose_set(scan)
    assert poses.shape == (rc.DISTINCT, 7) and len(np.unique(poses, axis=0)) == rc.DISTINCT
    assert far.mean() >= 0.30 and not far[:2].any()
    # at random positions: neither kind comes in long runs (a run of 16 equal flags has probability 2^-15 or less per position)
    runs = np.diff(np.flatnonzero(np.diff(far.astype(np.int8)) != 0))
    assert runs.max() < 16
    tau = cfg.first_frame_tau()
    n_corr = np.array([okicp.icp_pass(omap, keypoints, p, tau)[0][6] for p in poses])
    assert (n_corr[~far] > 0.5 * len(keypoints)).all()
    assert (n_corr[far] == 0).all()
    # the frames of the cases: prefixes of the keypoints; the single point of the n = 1 cases corresponds at some near poses
    assert len(keypoints) >= max(c.n for c in rc.SCORE_CASES)
    one = np.array([okicp.icp_pass(omap, keypoints[:1], p, tau)[0][6] for p in poses[~far]])
    assert 0 < one.sum()


@pytest.mark.parametrize("case", rc.SCORE_CASES, ids=lambda c: c.name)
def test_pose_orders(case):
    order = rc.score_order(case)
    assert order.shape == (case.count,) and np.array_equal(np.unique(order), np.arange(rc.DISTINCT))
    assert rc.differs_at_stride(order) >= 0.90


def test_refinement_order_holds_near_poses_only():
    cfg, omap, keypoints, scan = rc.score_scene()
    poses, far = rc.pose_set(scan)
    order = rc.refine_order(far)
    assert order.shape == (rc.REFINE_STARTS,) and np.array_equal(np.unique(order), np.flatnonzero(~far))
    assert rc.differs_at_stride(order) >= 0.90
    assert rc.REFINE_N <= len(keypoints) and rc.REFINE_STARTS % rc.REFINE_SLICE != 0  # (the last slice is a short one)


def test_the_item_arithmetic_the_cases_are_named_after():
    """items = tiles x poses; the names promise how they spread over at most 2 048 workgroups of a launch of at most score_chunk / 256
    items.  This restates the intent of the table, not the library's constants: the GPU test reads the counters."""
    by_name = {c.name: c for c in rc.SCORE_CASES}
    tiles = lambda c: -(-c.n // 256)
    assert tiles(by_name["stride_3"]) * 1500 == 4500 and 2 * rc.STRIDE < 4500 <= 3 * rc.STRIDE
    assert tiles(by_name["stride_full_tiles"]) * 1100 == 2200 and by_name["stride_full_tiles"].n % 256 == 0
    assert tiles(by_name["stride_one_point"]) * 2300 == 2300
    split = by_name["split_and_stride"]
    assert split.score_chunk // 256 == 2100 and 1500 < 2100 < 3000 and 4500 - 2 * 2100 == 300
    assert by_name["two_batches"].count == 65536 + 300 and by_name["three_batches_exact"].count == 2 * 65536
    assert rc.SMALL_CASE.n == 257 and rc.SMALL_CASE.count == 7


# ---- the sparse pyramid maps -----------------------------------------------------------------------------------------------------------
def _kept_by_a_map(points, voxel_size, cap):
    """every point survives the voxel map the GPU test builds (so Pointcloud() is this set)"""
    m = okicp.VoxelHashMap(voxel_size, 1.0e7, cap)
    m.AddPoints(np.array(points))
    got, want = m.Pointcloud(), np.array(points)
    return np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])])


@pytest.mark.parametrize("case", rc.SPARSE_MAPS, ids=lambda c: "dims_x_%d" % c.dims_x)
def test_sparse_maps_have_cells_only_one_shift_sets(case):
    pts = rc.sparse_points(case)
    assert pts.shape == (28, 3) and _kept_by_a_map(pts, 1.0, 20)
    mn, dims, levels = sr.pyramid(pts, rc.PYRAMID_CELL, 0, rc.SPARSE_LEVELS)
    assert dims.tolist()[:2] == [case.dims_x, rc.SPARSE_DIMS_Y] and dims[2] <= 4
    assert (case.dims_x + 31) // 32 == {543: 17, 544: 17, 545: 18, 577: 19, 70: 3}[case.dims_x]
    for h in range(7, rc.SPARSE_LEVELS + 1):
        s = 1 << (h - 1)
        x_only, y_only = rc.only_through(levels[h - 1], s)
        print("dims.x %d level %d (shift %d): %d cells only through x, %d only through y, %.1f %% set" % (case.dims_x, h, s, x_only, y_only, 100.0 * levels[h].mean()))
        assert y_only > 0
        if case.ask_x:
            assert x_only > 0
        elif s >= 128:
            assert x_only == 0 and (s >> 5) >= (case.dims_x + 31) // 32  # the shifted word lies beyond the row
    assert levels[rc.SPARSE_LEVELS].mean() < 0.5


@pytest.mark.parametrize("case", rc.DILATE_MAPS, ids=lambda c: "dilate_%d" % c.dilate)
def test_dilated_runs_cross_the_word_boundary(case):
    """Each of the eight cells EDGE_X holds a point whose run of 2 d + 1 bits stands alone in its row (the bit before and the bit after
    are clear), so no neighbour hides a wrong mask.  A run centred on cx covers cx - d .. cx + d: with d = 4 all eight cross the
    boundary between bits 31 and 32; with d = 3 the six inner ones cross, the run of cell 28 ends exactly on bit 31 and the run of
    cell 35 begins exactly on bit 0 of the next word - the two masks' other edge."""
    d = case.dilate
    pts = rc.dilate_points(case)
    assert pts.shape == (300, 3) and _kept_by_a_map(pts, 0.2, 50)
    mn, dims, levels = sr.pyramid(pts, rc.PYRAMID_CELL, d, rc.DILATE_LEVELS)
    assert dims[0] > 35 + d + 1 and levels[0].mean() < 0.6
    cells = sr.cells_of(pts, mn, rc.PYRAMID_CELL)
    crossing = 0
    for k, cx in enumerate(rc.EDGE_X):
        x, y, z = cells[2 + k]
        assert x == cx and x % 32 == (28 + k) % 32
        row = levels[0][z, y]
        assert row[x - d:x + d + 1].all() and not row[x - d - 1] and not row[x + d + 1]
        crossing += (x - d) >> 5 != (x + d) >> 5
        if d == 3 and cx in (28, 35):
            assert (x + d == 31) if cx == 28 else (x - d == 32)
        else:
            assert (x - d) >> 5 == 0 and (x + d) >> 5 == 1
    assert crossing == (8 if d == 4 else 6)


# ---- node lists and windows ------------------------------------------------------------------------------------------------------------
def test_many_yaws_window_and_nodes():
    frame, window, nodes = rc.many_yaws()
    assert len(frame) == 65 and (window.nx, window.ny, window.nyaw) == (9, 7, rc.MANY_YAWS) and window.yaw_step == 2.0 * np.pi / 2053
    assert rc.MANY_YAWS == 2 * 1024 + 5
    for j in rc.MANY_YAWS_PICKED:
        assert np.isin(j * 63 + np.arange(63), nodes).all()
    assert len(nodes) == 7 * 63 + 2000 and nodes.max() < window.nodes
    for h in (0, sc.LEVELS):
        scores = rc.restated_scores(frame, window, h, nodes)
        by_yaw = [scores[k * 63:(k + 1) * 63].max() for k in range(len(rc.MANY_YAWS_PICKED))]
        print("many_yaws level %d: best score per picked yaw %s, of the random nodes %d" % (h, by_yaw, scores[7 * 63:].max()))
        assert min(by_yaw) > 0 and scores[7 * 63:].max() > 0  # every trip of the yaw loop is seen through non-zero scores
    few = rc.few_yaws()
    assert few.nyaw == 180 and (few.nx, few.ny, few.x0, few.y0) == (window.nx, window.ny, window.x0, window.y0)
    assert rc.restated_scores(frame, few, 0).max() > 0


def test_many_nodes_lists():
    frame, window, scores, lists = rc.many_nodes()
    assert (window.nx, window.ny, window.nyaw) == (21, 17, 7) and window.nodes == 2499 and len(frame) == 65
    assert sorted(lists) == [rc.PIECE, rc.PIECE + 3, 2 * rc.PIECE] and rc.PIECE == 2 ** 20
    assert scores.shape == (2499,) and scores.max() > 0
    for length, nodes in lists.items():
        assert nodes.shape == (length,) and nodes.dtype == np.uint64
        assert np.array_equal(np.unique(nodes), np.arange(2499, dtype=np.uint64))
        if length > rc.PIECE:
            three = nodes[rc.PIECE - 1:rc.PIECE + 2].astype(np.int64)
            assert len(set(three.tolist())) == 3 and len(set(scores[three].tolist())) == 3


def test_deep_pyramid_windows_reach_below_the_grid():
    cfg, omap, keypoints, truth, mn, dims, levels = rc.search_scene()
    assert len(levels) == rc.DEEP_LEVELS + 1 and len(keypoints) == 250
    corner, lower, small = rc.deep_windows()
    assert (corner.nx, corner.ny, corner.nyaw) == (40, 33, 7) and (small.nx, small.ny, small.nyaw) == (8, 8, 1100)
    top = 1 << rc.DEEP_LEVELS
    assert max(corner.nx, corner.ny, small.nx, small.ny) < top  # one top block per yaw: search_children clips on every level
    cells = sr.frame_cells(keypoints, K.search_yaws(corner), corner, mn, rc.SEARCH_CELL)
    x = cells[:, :, 0][:, :, None] + np.arange(corner.nx)[None, None, :]
    assert ((x < 0) & (x > -top)).any()  # reads column 0 at level 10
    assert ((x < 0) & (x > -top) & (x <= -(1 << 7))).any()  # ... where level 7 already reads nothing
    cells = sr.frame_cells(keypoints, K.search_yaws(lower), lower, mn, rc.SEARCH_CELL)
    x = cells[:, :, 0][:, :, None] + np.arange(lower.nx)[None, None, :]
    assert (x <= -top).any() and ((x < 0) & (x > -top)).any()  # on either side of `lowest`
    assert x.max() <= -(1 << 7)  # ... and beyond the reach of level 7: it scores nothing there
    # not vacuous: the corner window and the small one score at level 0, the lowered one through the clamp at level 10
    assert rc.restated_scores(keypoints, corner, 0).max() > 0
    assert rc.restated_scores(keypoints, small, 0).max() > 0
    assert rc.restated_scores(keypoints, corner, 5, rc.deep_nodes(corner)).max() > 0
    assert rc.restated_scores(keypoints, lower, rc.DEEP_LEVELS, rc.deep_nodes(lower)).max() > 0
    assert not rc.restated_scores(keypoints, lower, 7, rc.deep_nodes(lower)).any()


def test_not_finite_rows_are_far_and_outside_windows_score_nothing():
    cfg, omap, keypoints, truth, mn, dims, levels = rc.search_scene()
    frame, without, rows = rc.not_finite()
    assert len(frame) == 250 and len(without) == 242 and {0, 63, 64, 249} <= set(rows.tolist())
    assert {axis for _, axis, _ in rc.NOT_FINITE_ROWS} == {0, 1, 2}
    values = [v for _, _, v in rc.NOT_FINITE_ROWS]
    assert any(np.isnan(v) for v in values) and np.inf in values and -np.inf in values and 1e300 in values and -1e300 in values
    inside = rc.windows_inside_and_corners()
    for window in inside:
        cells = sr.frame_cells(frame, K.search_yaws(window), window, mn, rc.SEARCH_CELL)
        assert (cells[:, rows, :] == -2 ** 40).any(axis=2).all()  # a coordinate beyond every grid, at every yaw
        full = rc.restated_scores(frame, window, 0)
        assert full.max() > 0 and np.array_equal(full, rc.restated_scores(without, window, 0))
    for window in rc.outside_windows():
        assert (window.nx, window.ny, window.nyaw) == (21, 17, 7)
        for f in (frame, keypoints):
            assert not rc.restated_scores(f, window, 0).any()
        nodes = np.arange(window.nodes)
        assert not rc.restated_scores(keypoints, window, sc.LEVELS, nodes).any()
