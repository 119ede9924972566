"""The exploration frontiers on the GPU (kicp_grid_frontiers: K.OccupancyGrid.frontiers) against the pure-host entry
(K.frontiers_from_occupancy) and the restatement of include/kicp.h's text (tests/frontier_ref.py).  Everything is integer and the
result is unique: np.array_equal, no tolerance anywhere.  The grids are set with set_counts, so the shapes are exact."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import frontier_ref as fr

pytestmark = pytest.mark.gpu

CASES = fr.cases()


def grid_for(width, height, cell=0.05):
    return K.OccupancyGrid(cell, 0.0, 0.0, width, height, 0.0, 1.0, 1.0)


def grid_of(occ):
    grid = grid_for(occ.shape[1], occ.shape[0])
    grid.set_counts(fr.counts_of(occ))
    return grid


def check(grid, occ, want_rows, want_labels, **kw):
    rows, labels = grid.frontiers(return_labels=True, **kw)
    assert rows.dtype == np.uint64 and rows.shape[1:] == (K.FRONTIER_WORDS,) and labels.dtype == np.uint32 and labels.shape == occ.shape
    bad = labels != want_labels
    print("%d x %d %s: %d frontiers (want %d), %d of %d labels differ" % (occ.shape[1], occ.shape[0], kw, len(rows), len(want_rows), bad.sum(), bad.size))
    assert not bad.any(), (np.argwhere(bad)[:5], labels[bad][:5], want_labels[bad][:5])
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(grid.frontiers(**kw), want_rows)  # without the label plane
    return rows, labels


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(name):
    """sides of 31 / 32 / 33 and 63 / 64 / 65, 1 x 1, 1 x 70, 70 x 1, grids without a frontier, a single cell, pairs through a tile
    corner, a frontier along a tile border, the serpentine, the checkerboard, rings, random grids - against the restatement and the
    host entry, with min_size 1 and 5"""
    occ = CASES[name]
    want_rows, want_labels = fr.frontiers(occ)
    grid = grid_of(occ)
    assert np.array_equal(grid.occupancy(), occ)
    rows, _ = check(grid, occ, want_rows, want_labels)
    host_rows, host_labels = K.frontiers_from_occupancy(occ, return_labels=True)
    assert np.array_equal(host_rows, want_rows) and np.array_equal(host_labels, want_labels)
    check(grid, occ, fr.rows_of(want_labels, None, 5), want_labels, min_size=5)
    if name in ("all_unknown", "all_clear", "all_occupied", "one_cell_clear"):
        assert len(rows) == 0
    if name.startswith("corner_pair") or name in ("serpentine_130x100", "checkerboard_65", "diamond_ring", "u_shape", "single_clear_cell"):
        assert len(rows) == 1
    if name == "two_apart":
        assert len(rows) == 6
    if name == "serpentine_130x100":
        assert rows[0].tolist()[:2] == [131, 25 * 128 + 24 * 3]
    if name == "checkerboard_65":
        assert rows[0].tolist()[:2] == [0, 2113]


def test_thresholds_and_min_observations():
    """counters on which min_observations and occupied_thresh change the classes: cells seen once or twice turn unknown at 3, a cell at
    66 is occupied at 0.65 and clear at 1, a cell at 1 is occupied at 0"""
    rng = np.random.default_rng(5)
    H, W = 50, 70
    counts = np.zeros((H, W, 2), dtype=np.uint16)
    seen = rng.integers(0, 6, (H, W))  # observations per cell: 0 .. 5
    hits = np.minimum(rng.integers(0, 6, (H, W)), seen)
    hits[rng.random((H, W)) < 0.6] = 0
    counts[..., 0], counts[..., 1] = hits, seen - hits
    grid = grid_for(W, H)
    grid.set_counts(counts)
    seen_rows = {}
    for min_observations in (1, 3):
        occ = K.occupancy_from_counts(counts, min_observations)
        assert np.array_equal(grid.occupancy(min_observations), occ)
        for thresh in (0.0, 0.65, 1.0):
            want_rows, want_labels = fr.frontiers(occ, thresh)
            check(grid, occ, want_rows, want_labels, min_observations=min_observations, occupied_thresh=thresh)
            assert np.array_equal(K.frontiers_from_occupancy(occ, min_observations, thresh), want_rows)
            seen_rows[(min_observations, thresh)] = want_rows
    assert not np.array_equal(seen_rows[(1, 0.65)], seen_rows[(3, 0.65)]) and not np.array_equal(seen_rows[(1, 0.0)], seen_rows[(1, 1.0)])
    assert len(seen_rows[(1, 0.65)]) > 0 and len(seen_rows[(3, 0.65)]) > 0


def test_capacity_on_the_device():
    occ = CASES["random_70x50_seed2"]
    want, _ = fr.frontiers(occ)
    F = len(want)
    grid = grid_of(occ)
    cfg = K.FrontierConfig(1, 0.65, 1)
    u64 = C.POINTER(C.c_ulonglong)
    for cap in (0, F - 1, F):
        rows, n = np.full((F + 1, 10), 77, dtype=np.uint64), C.c_size_t(99)
        rc = K.lib().kicp_grid_frontiers(grid._h, C.byref(cfg), 0, rows.ctypes.data_as(u64) if cap else None, cap, C.byref(n), None, 0)
        assert rc == (K.KICP_OK if cap >= F else K.KICP_ERR_CAPACITY) and n.value == F
        assert np.array_equal(rows[:cap], want[:cap]) and (rows[cap:] == 77).all()
    # more frontiers than the wrapper's first capacity: it calls once more
    occ = fr.in_unknown(120, 30, [(x, y) for x in range(1, 119, 3) for y in range(1, 29, 3)])
    rows = grid_of(occ).frontiers()
    assert len(rows) == 400 and np.array_equal(rows, fr.frontiers(occ)[0])


def plan_on(grid, occ, goal):
    """a plan over the grid's own costmap from one goal -> the device's potential"""
    table = K.nav2_cost_table(0.05, 2, 0.05, 3.0)
    return grid.potential(table, K.plan_weights(), [goal])


def test_use_plan():
    occ = CASES["random_130x100_seed1"].copy()
    occ[40:60, 50:80] = 0  # an open room around the goal
    occ[10:20, 10:30] = -1
    occ[12:18, 12:28] = 100  # a walled pocket: the frontier inside is unreached
    occ[14:16, 14:26] = 0
    occ[15, 18:22] = -1
    grid = grid_of(occ)
    cfg = K.FrontierConfig(1, 0.65, 1)
    n = C.c_size_t(7)
    assert not grid.has_plan()
    assert K.lib().kicp_grid_frontiers(grid._h, C.byref(cfg), 1, None, 0, C.byref(n), None, 0) == K.KICP_ERR_ARG and n.value == 0  # refused before any potential call
    with pytest.raises(K.KicpError) as e:
        grid.frontiers(use_plan=True)
    assert e.value.code == K.KICP_ERR_ARG and "kicp_grid_potential" in str(e.value)
    pot = plan_on(grid, occ, (65, 50))
    assert grid.has_plan() and pot[50, 65] == 0
    _, want_labels = fr.frontiers(occ)
    want = fr.rows_of(want_labels, pot)
    rows, _ = check(grid, occ, want, want_labels, use_plan=True)
    assert np.array_equal(K.frontiers_from_occupancy(occ, potential=pot), want)  # the host entry fed the device's own potential
    inside = rows[(rows[:, 4] >= 14) & (rows[:, 5] <= 25) & (rows[:, 6] >= 14) & (rows[:, 7] <= 15)]
    assert len(inside) >= 1 and (inside[:, 8] == fr.NONE).all() and np.array_equal(inside[:, 9], inside[:, 0])  # wholly in unreached space
    assert (rows[:, 8] < fr.NONE).any()
    # without the plan the same call still reads "no potential", and the plan survives both
    check(grid, occ, fr.rows_of(want_labels), want_labels)
    assert grid.has_plan()
    check(grid, occ, fr.rows_of(want_labels, pot, 5), want_labels, use_plan=True, min_size=5)


def test_two_cells_tie_at_the_least_potential():
    """a straight frontier seen from a goal on its axis of symmetry: the two cells beside the axis tie, the lower index wins"""
    occ = np.zeros((41, 41), dtype=np.int8)
    occ[30:, :] = -1
    occ[29, :10] = occ[29, 31:] = 100  # the frontier is row 29, x = 10 .. 30; the goal below its middle, on an occupied cell's column
    occ[25, 20] = 100
    grid = grid_of(occ)
    pot = grid.potential_of_costmap(np.where(occ == 100, 254, np.where(occ < 0, 255, 0)).astype(np.uint8), K.plan_weights(), [(20, 20)])
    rows = grid.frontiers(use_plan=True)
    _, want_labels = fr.frontiers(occ)
    assert np.array_equal(rows, fr.rows_of(want_labels, pot)) and len(rows) == 1
    row = pot[29, 10:31].astype(np.int64)
    best = row.min()
    assert (row == best).sum() >= 2 and rows[0, 8] == best and rows[0, 9] == 29 * 41 + 10 + int(np.argmin(row))


def test_a_real_drive():
    """260 x 200 cells of 0.1 m from a few integrated synthetic frames: the frontiers with use_plan after a potential from the robot's
    cell against the host entry over the grid's own readout and that potential"""
    cfg, frames, places = fr.room_drive()
    grid = K.OccupancyGrid(*cfg)
    for pts, pose, sensor in frames:
        assert grid.integrate(pts, pose, sensor)[0] > 500
    counts = grid.counts()
    robot = (int(np.floor((places[-1][0] + 0.2 + 13.0) / 0.1)), int(np.floor((places[-1][1] + 10.0) / 0.1)))  # the sensor's cell where the drive ended
    table = K.nav2_cost_table(0.1, 3, 0.15, 3.0)
    for min_observations in (1, 2):
        occ = grid.occupancy(min_observations)
        assert occ[robot[1], robot[0]] == 0
        pot = grid.potential(table, K.plan_weights(), [robot], min_observations=min_observations)
        assert pot[robot[1], robot[0]] == 0
        rows, labels = grid.frontiers(min_observations=min_observations, use_plan=True, return_labels=True)
        host_rows, host_labels = K.frontiers_from_occupancy(occ, min_observations, potential=pot, return_labels=True)
        print("min_observations %d: %d frontiers, %d frontier cells, largest %d, %d reached" % (min_observations, len(rows), int(rows[:, 1].sum()), int(rows[:, 1].max()),
                                                                                            int((rows[:, 8] != fr.NONE).sum())))
        assert np.array_equal(labels, host_labels) and np.array_equal(rows, host_rows)
        assert len(rows) >= 2 and (rows[:, 8] != fr.NONE).any()
    want_rows, want_labels = fr.frontiers(occ)
    assert np.array_equal(labels, want_labels) and np.array_equal(rows[:, :8], want_rows[:, :8])
    assert np.array_equal(grid.counts(), counts)


def test_handle_state():
    """repeated calls on one handle with F growing and shrinking; a frontier call changes neither the plan nor the counters"""
    grid = grid_for(130, 100)
    for name in ("random_130x100_seed1", "serpentine_130x100", "random_130x100_seed2", "random_130x100_seed1"):
        occ = CASES[name]
        grid.set_counts(fr.counts_of(occ))
        check(grid, occ, *fr.frontiers(occ))
    for occ in (np.full((100, 130), -1, dtype=np.int8), fr.in_unknown(130, 100, [(x, y) for x in range(1, 129, 2) for y in range(1, 99, 2)]), CASES["random_130x100_seed3"]):
        grid.set_counts(fr.counts_of(occ))
        check(grid, occ, *fr.frontiers(occ))
    occ = CASES["random_130x100_seed3"]
    assert not grid.has_plan()
    grid.frontiers()
    assert not grid.has_plan()
    costmap = np.where(occ > 65, 254, np.where(occ < 0, 255, 0)).astype(np.uint8)
    goal = tuple(int(v) for v in np.argwhere(costmap == 0)[len(costmap) // 2][::-1])
    pot = grid.potential_of_costmap(costmap, K.plan_weights(), [goal])
    start = K.arc_start((goal[0] + 0.5) * 0.05, (goal[1] + 0.5) * 0.05, 0.3)
    arcs = K.arc_steps(np.linspace(0.1, 0.6, 12), np.linspace(-1.0, 1.0, 12), 0.1)
    footprint = K.footprint_box(-0.05, 0.05, -0.05, 0.05, 0.05)
    before, counts = grid.score_arcs(start, arcs, 20, footprint), grid.counts()
    rows, labels = grid.frontiers(use_plan=True, return_labels=True)
    assert np.array_equal(rows, fr.rows_of(fr.frontiers(occ)[1], pot))
    assert grid.has_plan() and np.array_equal(grid.score_arcs(start, arcs, 20, footprint), before) and np.array_equal(grid.counts(), counts)
    assert np.array_equal(before, K.score_arcs_from_plan(K.plan_q(costmap, K.plan_weights()), pot, 0.05, 0.0, 0.0, start, arcs, 20, footprint))


def test_argument_errors_on_the_device():
    occ = CASES["pinned_8x6"]
    grid = grid_of(occ)

    def code(**kw):
        with pytest.raises(K.KicpError) as e:
            grid.frontiers(**kw)
        return e.value.code

    for kw in (dict(min_observations=0), dict(min_observations=-1), dict(occupied_thresh=-0.01), dict(occupied_thresh=1.01), dict(occupied_thresh=float("nan")),
               dict(min_size=0), dict(use_plan=True)):
        assert code(**kw) == K.KICP_ERR_ARG, kw
    u64, u32 = C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)
    cfg = K.FrontierConfig(1, 0.65, 1)
    rows, labels, n = np.zeros((8, 10), dtype=np.uint64), np.zeros(48, dtype=np.uint32), C.c_size_t(5)
    pr, pl = rows.ctypes.data_as(u64), labels.ctypes.data_as(u32)
    f = K.lib().kicp_grid_frontiers
    assert f(grid._h, C.byref(cfg), 0, pr, 8, C.byref(n), pl, 48) == K.KICP_OK and n.value == 2
    want_occ, want_labels, want_rows = fr.pinned_8x6()
    assert np.array_equal(rows[:2], want_rows) and np.array_equal(labels.reshape(6, 8), want_labels)
    for args in ((None, C.byref(cfg), 0, pr, 8, C.byref(n), pl, 48), (grid._h, None, 0, pr, 8, C.byref(n), pl, 48), (grid._h, C.byref(cfg), 0, pr, 8, None, pl, 48),
                 (grid._h, C.byref(cfg), 0, None, 8, C.byref(n), pl, 48), (grid._h, C.byref(cfg), 0, pr, 8, C.byref(n), pl, 47), (grid._h, C.byref(cfg), 0, pr, 8, C.byref(n), pl, 49),
                 (grid._h, C.byref(cfg), 0, pr, 8, C.byref(n), None, 48), (grid._h, C.byref(cfg), 0, pr, 8, C.byref(n), pl, 0),
                 (grid._h, C.byref(K.FrontierConfig(1, 0.65, 0)), 0, pr, 8, C.byref(n), pl, 48), (grid._h, C.byref(cfg), 1, pr, 8, C.byref(n), pl, 48)):
        assert f(*args) == K.KICP_ERR_ARG
    assert np.array_equal(grid.frontiers(), want_rows)  # the handle is unharmed
