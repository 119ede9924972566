"""Whole-map relocalisation on the GPU (include/kicp.h: kicp_occ_*, kicp_occ_score_nodes, kicp_search_poses, kicp_relocalize_search).
Everything here is integer and exact - no tolerance anywhere:
  - the occupancy pyramid equals the numpy restatement (tests/search_ref.py over Pointcloud()) bit for bit at every level;
  - ScoreNodes equals the restatement fed with K.search_yaws' own doubles;
  - SearchPoses equals the exhaustive stable top-M, the exhaustive scores being ScoreNodes at level 0 over ALL nodes (validated by the
    test before, so no heavy numpy runs here), and on the pinned windows the scores tests/test_search_host.py pins on the CPU;
  - RelocalizeSearch equals SearchPoses followed by RelocalizePlanar bit for bit, and ends within one cell and one yaw step of the
    truth on the pinned inputs - the condition tests/test_search_host.py shows the CPU oracle alone to meet."""
import functools

import numpy as np
import pytest

import kinematic_icp_amd as K
from kinematic_icp_amd import synthetic as syn
import search_cases as sc
import search_ref as sr

pytestmark = pytest.mark.gpu


def _assert_pyramid(occ, points, cell, dilate, levels):
    mn, dims, want = sr.pyramid(points, cell, dilate, levels)
    info = occ.info()
    assert np.array_equal(info["min"], mn) and np.array_equal(info["dims"], dims)
    assert (info["cell"], info["dilate"], info["levels"]) == (cell, dilate, levels)
    assert info["set_cells"] == int(want[0].sum())
    for h in range(levels + 1):
        assert np.array_equal(occ.level(h), sr.pack(want[h])), "level %d" % h
    return mn, dims, want


def _map_of(points, voxel_size=1.0, cap=20, max_distance=1.0e7):
    m = K.VoxelHashMap(voxel_size, max_distance, cap)
    m.AddPoints(np.asarray(points, dtype=np.float64))
    return m


class _Cases:
    """the GPU side of the pinned cases, built once per module and released with it (maps and pyramids hold device memory)"""

    @functools.lru_cache(maxsize=None)
    def __call__(self, name):
        """-> (cfg, gmap, items, occ, (min, dims, the restatement's levels))"""
        cfg, omap, items = sc.case(name)
        gmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
        gmap.AddPoints(omap.Pointcloud())
        assert gmap.num_points() == omap.num_points()
        occ = K.OccupancyPyramid.build(gmap, sc.CELL[name], sc.DILATE, sc.LEVELS)
        return cfg, gmap, items, occ, sr.pyramid(gmap.Pointcloud(), sc.CELL[name], sc.DILATE, sc.LEVELS)

    @functools.lru_cache(maxsize=None)
    def exhaustive(self, name, scan):
        """level-0 scores of all nodes of a pinned window, by ScoreNodes"""
        cfg, gmap, items, occ, _ = self(name)
        keypoints, truth, window = items[scan]
        return K.KinematicRegistration().ScoreNodes(keypoints, occ, window, 0, np.arange(window.nodes, dtype=np.uint64))


@pytest.fixture(scope="module")
def gpu_case():
    cases = _Cases()
    yield cases
    _Cases.__call__.cache_clear(), _Cases.exhaustive.cache_clear()


# ---- the pyramid ------------------------------------------------------------------------------------------------------------------
def test_pyramid_of_one_point():
    p = np.array([[0.3, -1.7, 0.45]])
    for dilate in (0, 1, 2):
        mn, dims, want = _assert_pyramid(K.OccupancyPyramid(_map_of(p), 0.25, dilate, 3), p, 0.25, dilate, 3)
        assert dims.tolist() == [2 * dilate + 3] * 3 and want[0].sum() == (2 * dilate + 1) ** 3


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_pyramid_points_at_the_extremes_of_the_box(dilate):
    # the eight corners of a box, on and off cell borders, and a few points inside
    rng = np.random.default_rng(11)
    lo, hi = np.array([-3.0, 1.25, -0.5]), np.array([4.1, 6.0, 0.75])
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    pts = np.vstack([corners, rng.uniform(lo, hi, (30, 3))])
    gmap = _map_of(pts, voxel_size=0.5)
    mn, dims, want = _assert_pyramid(K.OccupancyPyramid(gmap, 0.25, dilate, 4), gmap.Pointcloud(), 0.25, dilate, 4)
    assert not want[0][:, :, 0].any() and not want[0][:, :, -1].any() and want[0][:, :, 1].any() and want[0][:, :, -2].any()


@pytest.mark.parametrize("cells_x", [31, 32, 33, 64, 65])
def test_pyramid_pooling_within_across_and_beyond_a_word(cells_x):
    # dims.x = k + 3 for points from 0.5 cell to (k + 0.5) cells with dilate 0 (cell 0.25: exact in binary); levels 6: shifts 1 .. 32
    rng = np.random.default_rng(cells_x)
    k, cell = cells_x - 3, 0.25
    pts = rng.uniform([0.5 * cell, 0.0, 0.0], [(k + 0.5) * cell, 70 * cell, 2 * cell], (300, 3))
    pts[0, 0], pts[1, 0] = 0.5 * cell, (k + 0.5) * cell
    gmap = _map_of(pts, voxel_size=0.2, cap=50)
    mn, dims, want = _assert_pyramid(K.OccupancyPyramid(gmap, cell, 0, 6), gmap.Pointcloud(), cell, 0, 6)
    assert dims[0] == cells_x and dims[1] > 64


def test_pyramid_of_cfg4_and_cfg1(gpu_case):
    for name in ("cfg4", "cfg1"):
        cfg, gmap, items, occ, (mn, dims, want) = gpu_case(name)
        _assert_pyramid(occ, gmap.Pointcloud(), sc.CELL[name], sc.DILATE, sc.LEVELS)


def test_pyramid_of_a_map_whose_newest_state_is_on_the_device():
    rng = np.random.default_rng(5)
    gmap = K.VoxelHashMap(0.5, 60.0, 10)
    gmap.AddPoints(rng.uniform(-8, 8, (3000, 3)) * np.array([1, 1, 0.1]))
    scan = rng.uniform(-6, 6, (2000, 3)) * np.array([1, 1, 0.1])
    assert gmap.UpdateDevice(K.DeviceFrame(scan), syn.planar_pose(3.0, -2.0, 0.4))
    occ = K.OccupancyPyramid(gmap, 0.125, 1, 5)  # built from the device copy, before anything brings the host copy up to date
    _assert_pyramid(occ, gmap.Pointcloud(), 0.125, 1, 5)
    # a snapshot: a later update does not change it
    before = occ.level(0).copy()
    gmap.UpdateDevice(K.DeviceFrame(scan + 20.0), syn.planar_pose(0.0, 0.0, 0.0))
    assert np.array_equal(occ.level(0), before)


def test_pyramid_of_an_empty_map_and_errors():
    empty = K.VoxelHashMap(1.0, 100.0, 20)
    occ = K.OccupancyPyramid(empty, 0.5, 1, 3)
    info = occ.info()
    assert info["dims"].tolist() == [1, 1, 1] and info["set_cells"] == 0 and not info["min"].any()
    assert all(not occ.level(h).any() and occ.level(h).shape == (1, 1, 1) for h in range(4))
    reg = K.KinematicRegistration()
    frame = np.random.default_rng(0).uniform(-1, 1, (70, 3))
    window = K.search_window_around(occ, [0.0, 0.0], 1.0, 1.5, 0.0, np.deg2rad(90.0))
    assert (window.nx, window.ny, window.nyaw) == (5, 7, 4) and (window.x0, window.y0) == (-1.0, -1.5)
    assert not reg.ScoreNodes(frame, occ, window, 3, np.arange(window.nodes)).any()
    nodes, hits, poses = reg.SearchPoses(frame, occ, window, 5)
    assert nodes.tolist() == [0, 1, 2, 3, 4] and not hits.any()
    gmap = _map_of(np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 0.5]]))
    for cell, dilate, levels in ((0.0, 1, 2), (-1.0, 1, 2), (np.nan, 1, 2), (0.5, -1, 2), (0.5, 5, 2), (0.5, 1, -1), (0.5, 1, 11)):
        with pytest.raises(K.KicpError) as e:
            K.OccupancyPyramid(gmap, cell, dilate, levels)
        assert e.value.code == K.KICP_ERR_ARG
    K.OccupancyPyramid(gmap, 0.5, 4, 10), K.OccupancyPyramid(gmap, 0.5, 0, 0)  # the limits themselves are fine
    wide = _map_of(np.array([[0.0, 0.0, 0.0], [1000.0, 1000.0, 10.0]]))
    with pytest.raises(K.KicpError) as e:
        K.OccupancyPyramid(wide, 0.01, 1, 4)  # 1e5 x 1e5 x 1e3 cells
    assert e.value.code == K.KICP_ERR_CAPACITY and "bytes" in str(e.value) and "1 GiB" in str(e.value)
    with pytest.raises(K.KicpError) as e:
        K.OccupancyPyramid(_map_of(np.array([[0.0, 0.0, 0.0], [1.0e6, 0.0, 0.0]])), 0.01, 0, 0)  # 1e8 cells along x
    assert e.value.code == K.KICP_ERR_CAPACITY
    with pytest.raises(K.KicpError) as e:
        occ.level(4)
    assert e.value.code == K.KICP_ERR_ARG


# ---- ScoreNodes -------------------------------------------------------------------------------------------------------------------
def _windows(mn, dims, cell, truth):
    """inside the map; over the grid's low corner and over its high corner (cells leave the grid on every side); 7 yaws and 1"""
    hi = mn + dims * cell
    return [K.SearchWindow(truth[4] - 10 * cell, truth[5] - 8 * cell, truth[6], 21, 17, -0.4, 0.13, 7),
            K.SearchWindow(mn[0] - 9 * cell, mn[1] - 11 * cell, truth[6], 40, 33, 1.0, 0.7, 7),
            K.SearchWindow(hi[0] - 20 * cell, hi[1] - 15 * cell, truth[6] + 3 * cell, 35, 40, 2.9, 0.0, 1)]


@pytest.mark.parametrize("name", ["cfg1", "cfg4"])
def test_score_nodes_equals_the_restatement(name, gpu_case):
    cfg, gmap, items, occ, (mn, dims, levels) = gpu_case(name)
    cell = sc.CELL[name]
    keypoints, truth, _ = items[0]
    reg = K.KinematicRegistration()
    rng = np.random.default_rng(17)
    counts = [1, 3, 4, 5, 1000]
    checked = outside = 0
    for wi, window in enumerate(_windows(mn, dims, cell, truth)):
        cs = K.search_yaws(window)
        for si, size in enumerate([1, 63, 64, 65, 255, 256, 257, len(keypoints)]):
            frame = keypoints[:size] if size <= len(keypoints) else np.vstack([keypoints, keypoints[:size - len(keypoints)] + 0.01])
            cells = sr.frame_cells(frame, cs, window, mn, cell)
            outside += int(((cells[:, :, 0] < 0) | (cells[:, :, 0] + window.nx > dims[0]) | (cells[:, :, 1] < 0) | (cells[:, :, 1] + window.ny > dims[1])).sum())
            for level in (0, sc.LEVELS):
                count = counts[(wi + si + level) % len(counts)]
                nodes = rng.integers(0, window.nodes, count)
                nodes[0], nodes[-1] = (0, window.nodes - 1) if count > 1 else (window.nodes - 1, window.nodes - 1)
                got = reg.ScoreNodes(frame, occ, window, level, nodes)
                assert reg.get_option("search_nodes_scored") == count and reg.get_option("search_launches") == 1
                want = sr.score_nodes(levels[level], cells, window, nodes, h=level)
                assert np.array_equal(got, want), (name, wi, size, level)
                checked += int(want.sum())
    assert checked > 1000 and outside > 1000  # the cases are not vacuous: points were hit, and cells did leave the grid
    # an empty frame: zeros; arguments
    window = _windows(mn, dims, cell, truth)[0]
    assert not reg.ScoreNodes(np.zeros((0, 3)), occ, window, 0, [0, 1, 2]).any()
    for level, nodes in ((-1, [0]), (sc.LEVELS + 1, [0]), (0, [window.nodes])):
        with pytest.raises(K.KicpError) as e:
            reg.ScoreNodes(keypoints, occ, window, level, nodes)
        assert e.value.code == K.KICP_ERR_ARG
    sharded = K.KinematicRegistration()
    sharded.set_allreduce(lambda ptr, count, stream: None)
    with pytest.raises(K.KicpError) as e:
        sharded.ScoreNodes(keypoints, occ, window, 0, [0])
    assert e.value.code == K.KICP_ERR_ARG and "detach the multi-GPU exchange first" in str(e.value)


def test_top_level_scores_bound_every_node_of_their_block(gpu_case):
    """the property the search rests on, on the window over the grid's low corner (where blocks start below the grid)"""
    cfg, gmap, items, occ, (mn, dims, levels) = gpu_case("cfg4")
    keypoints, truth, _ = items[0]
    window = _windows(mn, dims, sc.CELL["cfg4"], truth)[1]
    reg = K.KinematicRegistration()
    exact = reg.ScoreNodes(keypoints, occ, window, 0, np.arange(window.nodes)).reshape(window.nyaw, window.ny, window.nx)
    for h in (1, sc.LEVELS):
        b = 1 << h
        ix, iy, j = np.meshgrid(np.arange(0, window.nx, b), np.arange(0, window.ny, b), np.arange(window.nyaw), indexing="ij")
        blocks = ((j * window.ny + iy) * window.nx + ix).reshape(-1)
        bounds = reg.ScoreNodes(keypoints, occ, window, h, blocks)
        for node, bound in zip(blocks, bounds):
            x, row = node % window.nx, node // window.nx
            assert bound >= exact[row // window.ny, row % window.ny:row % window.ny + b, x:x + b].max()


# ---- SearchPoses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scan", [("cfg4", 0), ("cfg4", 1), ("cfg1", 0), ("cfg1", 1)])
def test_search_poses_equals_the_exhaustive_top_m_on_the_pinned_windows(name, scan, gpu_case):
    cfg, gmap, items, occ, _ = gpu_case(name)
    keypoints, truth, window = items[scan]
    scores = gpu_case.exhaustive(name, scan)
    reg = K.KinematicRegistration()
    for top_m in (1, 8, 1000):
        nodes, hits, poses = reg.SearchPoses(keypoints, occ, window, top_m)
        want_nodes, want_hits = sr.top_m(scores, top_m)
        assert np.array_equal(nodes, want_nodes.astype(np.uint64)) and np.array_equal(hits, want_hits)
        for k in (0, len(nodes) - 1):
            assert np.array_equal(poses[k], sr.node_pose(window, sc.CELL[name], nodes[k]))
        scored, launches = reg.get_option("search_nodes_scored"), reg.get_option("search_launches")
        print("%s scan %d top_m %d: %d of %d nodes scored in %d launches" % (name, scan, top_m, scored, window.nodes, launches))
        if top_m == 8:
            assert hits.tolist() == sc.PINNED_HITS[(name, scan)][0]  # what the CPU restatement pins
            assert 0 < scored < window.nodes and launches >= 2 * sc.LEVELS + 1
    if (name, scan) == ("cfg1", 0):  # four nodes tie at all keypoints: the lower index first
        nodes, hits, _ = reg.SearchPoses(keypoints, occ, window, 4)
        assert hits.tolist() == [len(keypoints)] * 4 and (np.diff(nodes.astype(np.int64)) > 0).all()
    # a budget below the top level's blocks, and one that the walk exceeds: the capacity error, never a result
    reg.SearchPoses(keypoints, occ, window, 8)
    for budget in (10, int(reg.get_option("search_nodes_scored")) - 1):
        reg.set_option("search_max_nodes", budget)
        with pytest.raises(K.KicpError) as e:
            reg.SearchPoses(keypoints, occ, window, 8)
        assert e.value.code == K.KICP_ERR_CAPACITY and "search_max_nodes" in str(e.value)
    reg.set_option("search_max_nodes", 0)
    assert reg.get_option("search_max_nodes") == 2.0 ** 26
    assert len(reg.SearchPoses(keypoints, occ, window, 8)[0]) == 8


def test_search_poses_odd_windows_and_a_pyramid_without_levels(gpu_case):
    cfg, gmap, items, occ, _ = gpu_case("cfg4")
    keypoints, truth, pinned = items[0]
    cell = sc.CELL["cfg4"]
    flat = K.OccupancyPyramid(gmap, cell, sc.DILATE, 0)
    reg = K.KinematicRegistration()
    odd = K.SearchWindow(truth[4] - 17.3 * cell, truth[5] - 24.6 * cell, truth[6], 37, 50, -0.3, np.deg2rad(4.0), 9)
    one = K.SearchWindow(truth[4], truth[5], truth[6], 1, 1, 2.0 * np.arctan2(truth[2], truth[3]), 0.0, 1)
    for pyramid in (occ, flat):
        for window in (odd, one):
            scores = reg.ScoreNodes(keypoints, pyramid, window, 0, np.arange(window.nodes))
            for top_m in (1, 8, 20000):  # (the last one: above the node count)
                nodes, hits, poses = reg.SearchPoses(keypoints, pyramid, window, top_m)
                want_nodes, want_hits = sr.top_m(scores, top_m)
                assert len(nodes) == min(top_m, window.nodes)
                assert np.array_equal(nodes, want_nodes.astype(np.uint64)) and np.array_equal(hits, want_hits)
    assert reg.ScoreNodes(keypoints, occ, one, 0, [0])[0] > 0  # at the truth the scan does hit the map
    with pytest.raises(K.KicpError) as e:
        reg.SearchPoses(keypoints, occ, odd, 0)
    assert e.value.code == K.KICP_ERR_ARG
    # an empty frame: every score is zero, the first nodes by index
    nodes, hits, _ = reg.SearchPoses(np.zeros((0, 3)), occ, odd, 3)
    assert nodes.tolist() == [0, 1, 2] and not hits.any()


def test_search_window_around(gpu_case):
    cfg, gmap, items, occ, (mn, dims, _) = gpu_case("cfg1")
    cell = sc.CELL["cfg1"]
    w = K.search_window_around(occ, [1.0, -2.0], 1.1, 0.5, 0.3, np.deg2rad(7.0))
    assert (w.nx, w.ny, w.nyaw) == (9, 5, 52) and (w.x0, w.y0, w.z) == (0.0, -2.5, 0.3)
    assert w.yaw0 == -np.pi and w.yaw_step == 2 * np.pi / 52
    whole = K.search_window_around(occ, None, 0.0, -1.0, 0.0, 0.0)
    assert (whole.nx, whole.ny, whole.nyaw) == (dims[0], dims[1], 1) and (whole.x0, whole.y0) == (mn[0], mn[1]) and whole.yaw_step == 0.0


# ---- RelocalizeSearch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg4", "cfg1"])
def test_relocalize_search_equals_its_restatement_and_finds_the_truth(name, gpu_case):
    cfg, gmap, items, occ, _ = gpu_case(name)
    cell = sc.CELL[name]
    reg = K.KinematicRegistration()
    for scan, (keypoints, truth, window) in enumerate(items):
        for tau in (cfg.first_frame_tau(), 2.0 * cfg.first_frame_tau()):
            nodes, hits, poses = reg.SearchPoses(keypoints, occ, window, sc.TOP_M)
            want = reg.RelocalizePlanar(keypoints, gmap, poses, tau, top_m=len(poses), max_iterations=100, convergence=1e-4)
            want_status = reg.last_status
            pose, node, before, after = reg.RelocalizeSearch(keypoints, gmap, occ, window, tau, top_m=sc.TOP_M, max_iterations=100, convergence=1e-4)
            assert reg.last_status == want_status == K.KICP_OK
            assert np.array_equal(pose, want[0]) and (node, before, after) == (int(nodes[want[1]]), want[2], want[3])
            d, yaw = sc.offset(truth, pose)
            print("%s scan %d tau %.3f: node %d (%d hits), %.4f m and %.4f deg from the truth, cost %.6g -> %.6g"
                  % (name, scan, tau, node, hits[want[1]], d, np.degrees(yaw), before, after))
            assert d < cell and yaw < sc.YAW_STEP
    # nothing to correspond with: the fall-back of RelocalizePlanar
    keypoints, truth, window = items[0]
    pose, node, before, after = reg.RelocalizeSearch(np.zeros((0, 3)), gmap, occ, window, 1.0)
    assert reg.last_status == K.KICP_WARN_NO_CORRESPONDENCES and node == 0 and np.array_equal(pose, sr.node_pose(window, cell, 0))
    with pytest.raises(K.KicpError) as e:
        reg.RelocalizeSearch(keypoints, gmap, occ, window, 1.0, top_m=0)
    assert e.value.code == K.KICP_ERR_ARG
