"""One occupancy-grid handle driven through all of its features in turn (K.OccupancyGrid: occupancy, clearance, costmap, potential,
score_arcs, frontiers, gain, integrate).  The other GPU suites each drive one feature; this one checks the state the features share
in the handle: the counters every one of them reads, the plan - q and the potential - that score_arcs and frontiers(use_plan) read
and a later costmap must not disturb, the plan's validity after a potential call that fails, and the scratch buffers that grow.

Every result is compared with np.array_equal against the Python restatements of include/kicp.h (grid_ref, clearance_ref,
potential_ref, arcs_ref, frontier_ref, gain_ref), computed from grid.counts() as read back at that point of the sequence - never
against the library's own host entries.  Arrays handed in through out= hold a sentinel before the call.

The grid is 300 x 70 cells: x crosses a 256-cell clearance segment and nine 32-cell tiles, y two tiles and a partial third.  The
sequence runs twice on the same handle, the second time with three times as many arcs and viewpoints, so that the buffers sized by
them grow once."""
import math

import numpy as np
import pytest

import kinematic_icp_amd as K
import arcs_ref as ar
import clearance_ref as cr
import frontier_ref as fr
import gain_ref as gn
import grid_ref as gr
import potential_ref as pr

pytestmark = pytest.mark.gpu

W, H, CELL = 300, 70, 0.05
CFG = gr.make_config(CELL, 0.0, 0.0, W, H, 0.0, 1.0, 1.0)  # a reach of 20 cells
SENTINEL = 0xDEADBEEF
ROBOT = (20, 30)
MIN_SIZE = 5


def scene_counts():
    """occupied walls round a free interior, the rest unknown; two doorways, two unknown pockets and one unknown cell inside, so that
    four frontiers pass MIN_SIZE and one does not; an obstacle in front of the arcs' start and a few cells seen both ways"""
    counts = np.zeros((H, W, 2), dtype=np.uint16)
    counts[5:65, 7:293] = (3, 0)
    counts[6:64, 8:292] = (0, 2)
    counts[64, 40:46] = counts[30:36, 292] = (0, 2)  # the doorways
    counts[20:30, 100:130] = counts[40:50, 200:260] = counts[58, 280] = (0, 0)
    counts[30:45, 60] = (3, 0)
    counts[12:14, 150:180] = (5, 1)
    counts[50:55, 20:30] = (1, 1)  # 50: below the threshold, clear
    return counts


def frame():
    """a ring of returns 0.6 m round a sensor beside the first pocket, turned by 0.3 rad, with a NaN and a point outside the band"""
    a = np.linspace(0.0, 2.0 * math.pi, 40, endpoint=False)
    pts = np.stack([0.6 * np.cos(a), 0.6 * np.sin(a), np.full(40, 0.5)], axis=1)
    pts = np.concatenate([pts, [[np.nan, 0.0, 0.5], [0.3, 0.3, 1.5]]])
    pose = np.array([0.0, 0.0, math.sin(0.15), math.cos(0.15), (95 + 0.5) * CELL, (25 + 0.5) * CELL, 0.0])
    return pts, pose, np.zeros(3)


def raises_arg(call):
    with pytest.raises(K.KicpError) as e:
        call()
    assert e.value.code == K.KICP_ERR_ARG
    return str(e.value)


def sequence(grid, scale):
    grid.set_counts(scene_counts())
    counts = grid.counts()
    assert np.array_equal(counts, scene_counts())
    # 1: occupancy
    occ = gr.occupancy(counts)
    assert np.array_equal(grid.occupancy(), occ)
    assert (occ == 100).any() and (occ == 0).any() and (occ == -1).any() and (occ == 50).any()
    # 2: clearance of a sub-rectangle wider than a segment, with sources outside it
    rect = (20, 3, 270, 62)
    assert np.array_equal(grid.clearance(7, rect=rect), cr.clearance(occ, 7, rect=rect))
    # 3: costmap, R = 5
    table5, table9 = cr.mixed_table(5), cr.mixed_table(9)[::-1].copy()
    costmap5 = cr.costmap(occ, table5, inflate_unknown=True)
    assert np.array_equal(grid.costmap(table5, inflate_unknown=True), costmap5)
    # 4: potential: one goal in the free interior, one in unknown space that is not used
    weight, goals = pr.weights(), [ROBOT, (2, 2)]
    want_pot, want_stats = pr.potential_dijkstra(costmap5, weight, goals)
    out = np.full((H, W), SENTINEL, dtype=np.uint32)
    pot, stats = grid.potential(table5, weight, goals, inflate_unknown=True, return_stats=True, out=out)
    assert pot is out and np.array_equal(pot, want_pot) and stats[:3] == tuple(want_stats)[:3] and stats[0] == 1
    assert grid.has_plan()
    # 5: score_arcs: 7 arcs x 12 steps, 6 footprint samples, towards the obstacle
    n_arcs = 7 * scale
    arcs = ar.arc_steps(np.linspace(0.2, 1.0, n_arcs), np.linspace(-1.5, 1.5, n_arcs), 0.1)
    footprint = ar.footprint_box(-0.05, 0.05, -0.025, 0.025, 0.05)
    assert len(footprint) == 6
    start = (ar.centre(CELL, 0.0, 0.0, 55, 37)) + (1.0, 0.0)
    q5 = weight[costmap5]
    want_arcs = ar.score_arcs(q5, want_pot, CELL, 0.0, 0.0, start, arcs, 12, footprint)
    assert len({int(v) for v in want_arcs[:, 0]}) > 1  # some arcs are cut short
    out = np.full((n_arcs, 4), SENTINEL, dtype=np.uint32)
    assert grid.score_arcs(start, arcs, 12, footprint, out=out) is out and np.array_equal(out, want_arcs)
    # 6: frontiers ranked by the plan, with labels
    want_rows, want_labels = fr.frontiers(occ, min_size=MIN_SIZE, potential=want_pot)
    assert len(want_rows) == 4 and (want_labels != fr.NONE).sum() > want_rows[:, 1].sum()  # one frontier is below MIN_SIZE
    assert (want_rows[:, 8] < pr.MAX_POTENTIAL).all()  # every frontier is reachable
    rows, labels = grid.frontiers(min_size=MIN_SIZE, use_plan=True, return_labels=True)
    assert np.array_equal(rows, want_rows) and np.array_equal(labels, want_labels)
    # 7: gain on the frontiers' best cells, R = 6
    views = np.concatenate([rows[:, 9], rows[:, 0], rows[::-1, 9]][:scale]).astype(np.uint32)  # best cells, then least cells
    assert len(views) == 4 * scale
    want_gain = gn.gain(occ, views, 6)
    assert (want_gain[:, 0] > 0).all()
    assert np.array_equal(grid.gain(views, 6), want_gain)
    # 8: a costmap with another table and R = 9 overwrites the costmap buffer
    costmap9 = cr.costmap(occ, table9)
    assert not np.array_equal(costmap9, costmap5)
    assert np.array_equal(grid.costmap(table9), costmap9)
    # 9: the plan is q and the potential, not the costmap
    out[:] = SENTINEL
    grid.score_arcs(start, arcs, 12, footprint, out=out)
    assert np.array_equal(out, want_arcs) and grid.has_plan()
    assert np.array_equal(grid.frontiers(min_size=MIN_SIZE, use_plan=True), want_rows)
    # 10: integrate one small frame
    pts, pose, sensor = frame()
    want_counts = counts.copy()
    want_frame = gr.integrate(CFG, want_counts, pts, pose, sensor)
    assert grid.integrate(pts, pose, sensor) == want_frame and want_frame[0] == 40 and want_frame[1] == 2
    counts = grid.counts()
    assert np.array_equal(counts, want_counts) and not np.array_equal(counts, scene_counts())
    # 11: gain and frontiers see the new counters; the plan is still the one of step 4
    occ = gr.occupancy(counts)
    assert np.array_equal(grid.occupancy(), occ)
    want_gain2 = gn.gain(occ, views, 6)
    assert not np.array_equal(want_gain2, want_gain)
    assert np.array_equal(grid.gain(views, 6), want_gain2)
    want_rows2, want_labels2 = fr.frontiers(occ, min_size=MIN_SIZE, potential=want_pot)
    assert not np.array_equal(want_labels2, want_labels)
    rows, labels = grid.frontiers(min_size=MIN_SIZE, use_plan=True, return_labels=True)
    assert np.array_equal(rows, want_rows2) and np.array_equal(labels, want_labels2)
    assert np.array_equal(grid.frontiers(min_size=MIN_SIZE), fr.frontiers(occ, min_size=MIN_SIZE)[0])
    # 12: a potential call that fails on its arguments leaves no plan
    out = np.full((H, W), SENTINEL, dtype=np.uint32)
    assert "goal 1 " in raises_arg(lambda: grid.potential(table5, weight, [ROBOT, (W, 3)], out=out))
    assert (out == SENTINEL).all() and not grid.has_plan()
    assert "no plan" in raises_arg(lambda: grid.score_arcs(start, arcs, 12, footprint))
    assert "no plan" in raises_arg(lambda: grid.frontiers(use_plan=True))
    assert np.array_equal(grid.frontiers(min_size=MIN_SIZE), fr.frontiers(occ, min_size=MIN_SIZE)[0])  # without the plan: as before
    # 13: a valid potential_of_costmap brings a plan back: that of the costmap it was given
    want_pot9, want_stats9 = pr.potential_dijkstra(costmap9, weight, [ROBOT])
    pot, stats = grid.potential_of_costmap(costmap9, weight, [ROBOT], return_stats=True, out=out)
    assert pot is out and np.array_equal(pot, want_pot9) and stats[:3] == tuple(want_stats9)[:3]
    assert grid.has_plan() and not np.array_equal(want_pot9, want_pot)
    assert np.array_equal(grid.score_arcs(start, arcs, 12, footprint), ar.score_arcs(weight[costmap9], want_pot9, CELL, 0.0, 0.0, start, arcs, 12, footprint))
    assert np.array_equal(grid.counts(), counts)


def test_one_handle_through_every_feature_twice():
    grid = K.OccupancyGrid(CELL, 0.0, 0.0, W, H, 0.0, 1.0, 1.0)
    sequence(grid, 1)
    sequence(grid, 3)
