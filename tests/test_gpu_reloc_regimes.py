"""The relocalisation kernels on the GPU in the regimes tests/test_gpu_score_poses.py, test_gpu_planar.py, test_gpu_relocalize.py and
test_gpu_search.py never enter (the cases and their premises: tests/reloc_cases.py, proved on the CPU in tests/test_reloc_cases.py):

  A  a workgroup of k_score_poses / k_planar_poses that serves several (tile, pose) items: the stride loop, the two alternating LDS
     sets, items with and without correspondences in turn
  B  a split into launches (item0 > 0, inside a tile) together with A
  C  more poses than one batch of the host loop (first > 0), and the handle's life after it
  D  k_search_cells with more yaws than its grid has rows
  E  a node list longer than one piece of score_prepared
  F  k_occ_pool with shifts of whole words (levels 7 .. 10)
  G  k_occ_mark with dilate 3 and 4 (runs of 7 and 9 bits across a word boundary)
  H  k_search_score above level 4, and a pyramid with more levels than the window has cells per axis
  I  frame points that are not finite or 1e300 away, windows wholly outside the grid

Every comparison is exact except the two the older files already make with a tolerance (the oracle's sums: SUM_RTOL / SUM_ATOL of
tests/test_gpu_score_poses.py; S_x and S_b: the bounds of tests/test_gpu_planar.py).  A long pose list is poses[order] of 300
distinct poses: its rows must be the rows of the 300-pose call - one item per workgroup, the regime the older files tie to
kicp_pass_sums - indexed by the order.  That each regime was entered is read from the handle's read-only counters
("score_items_per_workgroup", "score_launches", "search_yaw_trips", "search_launches"), never from the library's constants: a moved
threshold fails here instead of silently uncovering the path."""
import numpy as np
import pytest

import kinematic_icp_amd as K
from checkers import okicp
import planar_ref as pr
import reloc_cases as rc
import search_cases as sc
import search_ref as sr
from test_gpu_planar import EPS, _assert_shared_sums
from test_gpu_score_poses import SUM_ATOL, SUM_RTOL
from test_gpu_search import _assert_pyramid, _map_of

pytestmark = pytest.mark.gpu


def _sorted(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])]


# ---- one frame at many poses -------------------------------------------------------------------------------------------------------
class _Scoring:
    """cfg1's map on the GPU, the pose set, the two handles, and per frame size the rows at the 300 distinct poses (computed on first
    use, once, and checked there against kicp_pass_sums, planar_ref and the oracle)"""

    def __init__(self):
        self.cfg, self.omap, self.keypoints, scan = rc.score_scene()
        self.gmap = K.VoxelHashMap(self.cfg.voxel_size, self.cfg.max_range, self.cfg.max_points_per_voxel)
        self.gmap.AddPoints(self.omap.Pointcloud())
        assert self.gmap.num_points() == self.omap.num_points()
        self.poses, self.far = rc.pose_set(scan)
        self.tau = self.cfg.first_frame_tau()
        generic = K.KinematicRegistration()
        generic.set_option("small", 0)
        self.handles = (K.KinematicRegistration(), generic)
        self._rows, self._oracle = {}, {}

    def frame(self, n):
        return self.keypoints[:n]

    def rows(self, n):
        """-> per handle (n_corr[300], ssr[300], planar sums[300, 8]) of ONE call each at the 300 distinct poses"""
        if n not in self._rows:
            self._rows[n] = [self._reference(reg, n) for reg in self.handles]
        return self._rows[n]

    def _reference(self, reg, n):
        frame, tau = self.frame(n), self.tau
        want = np.array([reg.pass_sums(frame, self.gmap, p, tau) for p in self.poses]).reshape(-1, 7)
        n_corr, ssr = reg.ScorePoses(frame, self.gmap, self.poses, tau)
        assert reg.get_option("score_items_per_workgroup") == 1 and reg.get_option("score_launches") == 1
        assert np.array_equal(n_corr, want[:, 6]) and np.array_equal(ssr, want[:, 5])
        sums = reg.PlanarSums(frame, self.gmap, self.poses, tau)
        assert reg.get_option("score_items_per_workgroup") == 1 and reg.get_option("score_launches") == 1
        _assert_shared_sums(sums, want)
        assert not n_corr[self.far].any() and not sums[self.far].any()
        if n >= 64:
            assert (n_corr[~self.far] > 0.25 * n).all()
        worst_x = worst_b = 0.0
        for k in np.flatnonzero(~self.far):  # S_x and S_b: the bounds of tests/test_gpu_planar.py test_the_two_new_sums
            idx, d2, nn = reg.pass_correspondences(frame, self.gmap, self.poses[k], tau)
            ref = pr.planar_sums_from(idx >= 0, nn, frame, self.poses[k])
            count = ref[0]
            assert sums[k, 0] == count
            err_x, err_b = abs(sums[k, 1] - ref[1]), abs(sums[k, 5] - ref[5])
            bound_x, bound_b = count * 2.0 ** -41 + np.spacing(abs(ref[1])), count * (2.0 ** -41 + 16 * EPS * tau)
            worst_x, worst_b = max(worst_x, err_x / bound_x if bound_x else 0.0), max(worst_b, err_b / bound_b if bound_b else 0.0)
            assert err_x <= bound_x and err_b <= bound_b
        print("n %d: worst |S_x - ref| / bound %.3f, worst |S_b - ref| / bound %.3f over %d poses" % (n, worst_x, worst_b, int((~self.far).sum())))
        return n_corr, ssr, sums

    def oracle(self, n, k):
        if (n, k) not in self._oracle:
            self._oracle[(n, k)] = okicp.icp_pass(self.omap, self.frame(n), self.poses[k], self.tau)[0]
        return self._oracle[(n, k)]


@pytest.fixture(scope="module")
def scoring():
    return _Scoring()


def _counters(reg):
    return int(reg.get_option("score_launches")), int(reg.get_option("score_items_per_workgroup"))


def _assert_counters(case, launches, items):
    assert items >= case.items_per_workgroup
    how, value = case.launches
    assert launches == value if how == "==" else launches >= value


def _run_case(scoring, reg, case, which):
    """one call of ScorePoses ("score") or PlanarSums ("planar") of a case's long list on `reg` -> (result, launches, items per workgroup)"""
    order = rc.score_order(case)
    long_list = scoring.poses[order]
    if case.score_chunk is not None:
        reg.set_option("score_chunk", case.score_chunk)
    try:
        call = reg.ScorePoses if which == "score" else reg.PlanarSums
        got = call(scoring.frame(case.n), scoring.gmap, long_list, scoring.tau)
        launches, items = _counters(reg)
    finally:
        reg.set_option("score_chunk", 0)
    print("%s %s small=%d: score_launches %d, score_items_per_workgroup %d" % (case.name, which, int(reg.get_option("small")), launches, items))
    return order, got, launches, items


@pytest.mark.parametrize("case", rc.SCORE_CASES, ids=lambda c: c.name)
def test_score_poses_under_stride_split_and_batches(scoring, case):
    for reg, (want_n, want_ssr, _) in zip(scoring.handles, scoring.rows(case.n)):
        order, (n_corr, ssr), launches, items = _run_case(scoring, reg, case, "score")
        assert n_corr.shape == ssr.shape == (case.count,)
        assert np.array_equal(n_corr, want_n[order]) and np.array_equal(ssr, want_ssr[order])
        _assert_counters(case, launches, items)
    # the oracle at 32 places of the list (the first, the last, 30 between): tests/test_gpu_score_poses.py test_scores_match_the_oracle
    for at in np.linspace(0, case.count - 1, 32).astype(np.int64):
        o = scoring.oracle(case.n, int(order[at]))
        assert n_corr[at] == o[6]
        np.testing.assert_allclose(ssr[at], o[5], rtol=SUM_RTOL, atol=SUM_ATOL)
    assert (n_corr > 0).any() and (n_corr == 0).any()


@pytest.mark.parametrize("case", rc.SCORE_CASES, ids=lambda c: c.name)
def test_planar_sums_under_stride_split_and_batches(scoring, case):
    for reg, (_, _, want) in zip(scoring.handles, scoring.rows(case.n)):
        order, sums, launches, items = _run_case(scoring, reg, case, "planar")
        assert sums.shape == (case.count, 8)
        assert np.array_equal(sums, want[order])  # all eight sums, bit for bit, the two new ones included
        _assert_counters(case, launches, items)
    assert (sums[:, 0] > 0).any() and not sums[scoring.far[order]].any()


def test_the_small_cases_serve_one_item_per_workgroup(scoring):
    """what the older files cover (n = 257, seven poses: 14 items) - pinned, so that the cases above are known to add to it"""
    case = rc.SMALL_CASE
    for reg, (want_n, want_ssr, want) in zip(scoring.handles, scoring.rows(case.n)):
        n_corr, ssr = reg.ScorePoses(scoring.frame(case.n), scoring.gmap, scoring.poses[:case.count], scoring.tau)
        assert _counters(reg) == (1, 1)
        assert np.array_equal(n_corr, want_n[:case.count]) and np.array_equal(ssr, want_ssr[:case.count])
        sums = reg.PlanarSums(scoring.frame(case.n), scoring.gmap, scoring.poses[:case.count], scoring.tau)
        assert _counters(reg) == (1, 1)
        assert np.array_equal(sums, want[:case.count])


def test_a_handle_after_more_than_one_batch(scoring):
    """the buffers stay at the batch's size: a short list afterwards must get what a fresh handle gets, and a strided one its own
    result - rows beyond the list's length hold the long list's sums and must not leak"""
    by_name = {c.name: c for c in rc.SCORE_CASES}
    big, strided = by_name["two_batches"], by_name["stride_3"]
    reg, fresh = K.KinematicRegistration(), K.KinematicRegistration()
    seven = scoring.poses[:7]
    for which in ("score", "planar"):
        call, call_fresh = (reg.ScorePoses, fresh.ScorePoses) if which == "score" else (reg.PlanarSums, fresh.PlanarSums)
        order, got, launches, items = _run_case(scoring, reg, big, which)
        _assert_counters(big, launches, items)
        want = scoring.rows(big.n)[0]
        if which == "score":
            assert np.array_equal(got[0], want[0][order]) and np.array_equal(got[1], want[1][order])
        else:
            assert np.array_equal(got, want[2][order])
        for n in (big.n, 257):
            a, b = call(scoring.frame(n), scoring.gmap, seven, scoring.tau), call_fresh(scoring.frame(n), scoring.gmap, seven, scoring.tau)
            assert np.array_equal(np.asarray(a), np.asarray(b))
            assert _counters(reg) == (1, 1)
        order, got, launches, items = _run_case(scoring, reg, strided, which)
        _assert_counters(strided, launches, items)
        want = scoring.rows(strided.n)[0]
        if which == "score":
            assert np.array_equal(got[0], want[0][order]) and np.array_equal(got[1], want[1][order])
        else:
            assert np.array_equal(got, want[2][order])


def test_refinement_under_stride_equals_its_slices(scoring):
    """2 300 starts at n = 257 (two tiles: 4 600 items in the first iteration) against the same call in slices of 400 - the regime
    tests/test_gpu_planar.py test_refinement_equals_its_restatement ties to the restatement"""
    frame = scoring.frame(rc.REFINE_N)
    start = scoring.poses[rc.refine_order(scoring.far)]
    for reg in scoring.handles:
        whole = reg.RefinePosesPlanar(frame, scoring.gmap, start, scoring.tau, rc.REFINE_ITERATIONS, 1e-4)
        launches, items = _counters(reg)
        print("refinement small=%d: score_launches %d, score_items_per_workgroup %d" % (int(reg.get_option("small")), launches, items))
        assert items >= 2 and launches >= 1
        parts, most = [], 0
        for first in range(0, len(start), rc.REFINE_SLICE):
            parts.append(reg.RefinePosesPlanar(frame, scoring.gmap, start[first:first + rc.REFINE_SLICE], scoring.tau, rc.REFINE_ITERATIONS, 1e-4))
            most = max(most, _counters(reg)[1])
        assert most == 1  # the slices: one item per workgroup
        for g, w in zip(whole, (np.concatenate([p[i] for p in parts]) for i in range(3))):
            assert np.array_equal(g, w)
        poses, iterations, status = whole
        assert (iterations > 0).any() and len(np.unique(iterations)) > 1  # poses leave the lock step at different iterations


# ---- pyramids ------------------------------------------------------------------------------------------------------------------------
def _assert_rows_end_clean(occ, dims, levels):
    """the last word of every row holds no bit beyond dims.x, at every level"""
    spare = int(dims[0]) % 32
    for h in range(levels + 1):
        words = occ.level(h)
        assert words.shape[2] == (int(dims[0]) + 31) // 32
        if spare:
            assert not (words[:, :, -1] >> np.uint32(spare)).any(), "level %d" % h


@pytest.mark.parametrize("case", rc.SPARSE_MAPS, ids=lambda c: "dims_x_%d" % c.dims_x)
def test_pyramid_pooling_by_whole_words(case):
    pts = rc.sparse_points(case)
    gmap = _map_of(pts)
    assert np.array_equal(_sorted(gmap.Pointcloud()), _sorted(pts))
    occ = K.OccupancyPyramid(gmap, rc.PYRAMID_CELL, 0, rc.SPARSE_LEVELS)
    mn, dims, want = _assert_pyramid(occ, gmap.Pointcloud(), rc.PYRAMID_CELL, 0, rc.SPARSE_LEVELS)
    assert dims.tolist()[:2] == [case.dims_x, rc.SPARSE_DIMS_Y]
    _assert_rows_end_clean(occ, dims, rc.SPARSE_LEVELS)


@pytest.mark.parametrize("case", rc.DILATE_MAPS, ids=lambda c: "dilate_%d" % c.dilate)
def test_pyramid_dilated_runs_across_a_word_boundary(case):
    pts = rc.dilate_points(case)
    gmap = _map_of(pts, voxel_size=0.2, cap=50)
    assert np.array_equal(_sorted(gmap.Pointcloud()), _sorted(pts))
    occ = K.OccupancyPyramid(gmap, rc.PYRAMID_CELL, case.dilate, rc.DILATE_LEVELS)
    mn, dims, want = _assert_pyramid(occ, gmap.Pointcloud(), rc.PYRAMID_CELL, case.dilate, rc.DILATE_LEVELS)
    _assert_rows_end_clean(occ, dims, rc.DILATE_LEVELS)


# ---- search --------------------------------------------------------------------------------------------------------------------------
class _Search:
    """cfg4's map on the GPU with a pyramid of 4 and one of 10 levels, both held to the restatement level by level"""

    def __init__(self):
        self.cfg, omap, self.keypoints, self.truth, self.mn, self.dims, self.levels = rc.search_scene()
        self.gmap = K.VoxelHashMap(self.cfg.voxel_size, self.cfg.max_range, self.cfg.max_points_per_voxel)
        self.gmap.AddPoints(omap.Pointcloud())
        assert np.array_equal(_sorted(self.gmap.Pointcloud()), _sorted(omap.Pointcloud()))
        self.occ4 = K.OccupancyPyramid(self.gmap, rc.SEARCH_CELL, sc.DILATE, sc.LEVELS)
        self.occ10 = K.OccupancyPyramid(self.gmap, rc.SEARCH_CELL, sc.DILATE, rc.DEEP_LEVELS)
        for occ, levels in ((self.occ4, sc.LEVELS), (self.occ10, rc.DEEP_LEVELS)):
            info = occ.info()
            assert np.array_equal(info["min"], self.mn) and np.array_equal(info["dims"], self.dims) and info["levels"] == levels
            for h in range(levels + 1):
                assert np.array_equal(occ.level(h), sr.pack(self.levels[h])), "level %d" % h
        self.reg = K.KinematicRegistration()

    def cells(self, frame, window):
        return sr.frame_cells(frame, K.search_yaws(window), window, self.mn, rc.SEARCH_CELL)

    def all_nodes(self, frame, occ, window, level=0):
        return self.reg.ScoreNodes(frame, occ, window, level, np.arange(window.nodes, dtype=np.uint64))


@pytest.fixture(scope="module")
def search():
    return _Search()


def test_score_nodes_with_more_yaws_than_one_trip(search):
    frame, window, nodes = rc.many_yaws()
    few, reg = rc.few_yaws(), search.reg
    first = search.all_nodes(frame, search.occ4, few)
    assert reg.get_option("search_yaw_trips") == 1
    assert np.array_equal(first.reshape(few.nyaw, few.ny, few.nx), rc.restated_scores(frame, few, 0)) and first.any()
    cells = search.cells(frame, window)
    for level in (0, sc.LEVELS):
        got = reg.ScoreNodes(frame, search.occ4, window, level, nodes)
        trips = int(reg.get_option("search_yaw_trips"))
        print("many_yaws level %d: search_yaw_trips %d, best score %d" % (level, trips, got.max()))
        assert trips == 3
        assert np.array_equal(got, sr.score_nodes(search.levels[level], cells, window, nodes, h=level))
        assert got[:7 * 63].reshape(7, 63).max(axis=1).min() > 0  # every picked yaw scores somewhere
    # the cells buffer shrinks logically, not physically: the short table again, over what the long one left behind
    assert np.array_equal(search.all_nodes(frame, search.occ4, few), first)
    assert reg.get_option("search_yaw_trips") == 1


def test_score_nodes_of_lists_longer_than_one_piece(search):
    frame, window, scores, lists = rc.many_nodes()
    reg = search.reg
    exhaustive = search.all_nodes(frame, search.occ4, window)
    assert reg.get_option("search_launches") == 1
    assert np.array_equal(exhaustive, scores)
    for length in sorted(lists):
        nodes = lists[length]
        got = reg.ScoreNodes(frame, search.occ4, window, 0, nodes)
        launches = int(reg.get_option("search_launches"))
        print("many_nodes %d nodes: search_launches %d" % (length, launches))
        assert launches == (1 if length == rc.PIECE else 2) and reg.get_option("search_nodes_scored") == length
        assert np.array_equal(got, exhaustive[nodes.astype(np.int64)])


def test_deep_pyramid_score_nodes_above_level_4(search):
    corner, lower, small = rc.deep_windows()
    reg, keypoints = search.reg, search.keypoints
    hit = {}
    for name, window in (("corner", corner), ("lower", lower)):
        cells = search.cells(keypoints, window)
        nodes = rc.deep_nodes(window)
        for h in (5, 7, rc.DEEP_LEVELS):
            got = reg.ScoreNodes(keypoints, search.occ10, window, h, nodes)
            assert np.array_equal(got, sr.score_nodes(search.levels[h], cells, window, nodes, h=h)), (name, h)
            hit[(name, h)] = int(got.max())
    print("deep_pyramid best scores: %s" % hit)
    assert hit[("corner", 5)] > 0 and hit[("lower", rc.DEEP_LEVELS)] > 0 and hit[("lower", 7)] == 0  # 1 100 cells below the grid: only the clamp of level 10 reaches it


def test_deep_pyramid_bounds_every_node_of_a_block(search):
    """tests/test_gpu_search.py test_top_level_scores_bound_every_node_of_their_block at h = 7 and h = 10: one block per yaw"""
    corner, lower, small = rc.deep_windows()
    reg, keypoints = search.reg, search.keypoints
    exact = search.all_nodes(keypoints, search.occ10, corner).reshape(corner.nyaw, corner.ny, corner.nx)
    assert np.array_equal(exact, rc.restated_scores(keypoints, corner, 0))
    for h in (7, rc.DEEP_LEVELS):
        b = 1 << h
        ix, iy, j = np.meshgrid(np.arange(0, corner.nx, b), np.arange(0, corner.ny, b), np.arange(corner.nyaw), indexing="ij")
        blocks = ((j * corner.ny + iy) * corner.nx + ix).reshape(-1)
        assert len(blocks) == corner.nyaw
        bounds = reg.ScoreNodes(keypoints, search.occ10, corner, h, blocks)
        for node, bound in zip(blocks, bounds):
            x, row = node % corner.nx, node // corner.nx
            assert bound >= exact[row // corner.ny, row % corner.ny:row % corner.ny + b, x:x + b].max()


def test_deep_pyramid_search_equals_the_exhaustive_top_m(search):
    corner, lower, small = rc.deep_windows()
    reg, keypoints = search.reg, search.keypoints
    rng = np.random.default_rng(11)
    for name, window in (("corner", corner), ("small", small)):
        scores = search.all_nodes(keypoints, search.occ10, window)
        if window.nodes < 10000:
            assert np.array_equal(scores.reshape(window.nyaw, window.ny, window.nx), rc.restated_scores(keypoints, window, 0))
        else:
            sample = rng.integers(0, window.nodes, 2000)
            assert np.array_equal(scores[sample], rc.restated_scores(keypoints, window, 0, sample))
        assert scores.max() > 0
        for top_m in (1, 8, 500):
            want_nodes, want_hits = sr.top_m(scores, top_m)
            nodes, hits, poses = reg.SearchPoses(keypoints, search.occ10, window, top_m)
            scored, launches, trips = (int(reg.get_option(k)) for k in ("search_nodes_scored", "search_launches", "search_yaw_trips"))
            print("deep_pyramid %s top_m %d: %d of %d nodes scored in %d launches, search_yaw_trips %d" % (name, top_m, scored, window.nodes, launches, trips))
            assert np.array_equal(nodes, want_nodes.astype(np.uint64)) and np.array_equal(hits, want_hits)
            assert launches >= 2 * rc.DEEP_LEVELS + 1 and trips == (2 if name == "small" else 1)
            for k in (0, len(nodes) - 1):
                assert np.array_equal(poses[k], sr.node_pose(window, rc.SEARCH_CELL, nodes[k]))
            shallow = reg.SearchPoses(keypoints, search.occ4, window, top_m)
            assert np.array_equal(shallow[0], nodes) and np.array_equal(shallow[1], hits) and np.array_equal(shallow[2], poses)


def test_frame_points_that_are_not_finite_and_windows_outside_the_grid(search):
    frame, without, rows = rc.not_finite()
    reg, keypoints = search.reg, search.keypoints
    for window in rc.windows_inside_and_corners():
        for occ, level in ((search.occ4, 0), (search.occ10, rc.DEEP_LEVELS)):
            got = search.all_nodes(frame, occ, window, level)
            assert np.array_equal(got, search.all_nodes(without, occ, window, level))
            if level == 0:
                assert np.array_equal(got.reshape(window.nyaw, window.ny, window.nx), rc.restated_scores(frame, window, 0)) and got.any()
            else:
                nodes = np.arange(0, window.nodes, 37)
                assert np.array_equal(got[nodes], rc.restated_scores(frame, window, level, nodes))
        top = reg.SearchPoses(frame, search.occ10, window, 8)
        clean = reg.SearchPoses(without, search.occ10, window, 8)
        assert all(np.array_equal(a, b) for a, b in zip(top, clean)) and top[1][0] > 0
    for window in rc.outside_windows():
        for f in (keypoints, frame):
            for occ, level in ((search.occ4, 0), (search.occ4, sc.LEVELS), (search.occ10, rc.DEEP_LEVELS)):
                assert not search.all_nodes(f, occ, window, level).any()
            for occ in (search.occ4, search.occ10):
                nodes, hits, poses = reg.SearchPoses(f, occ, window, 3)
                assert nodes.tolist() == [0, 1, 2] and not hits.any()
