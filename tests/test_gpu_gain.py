"""The information gain on the GPU (kicp_grid_gain: K.OccupancyGrid.gain) against the pure-host entry (K.gain_from_occupancy) and the
restatement of include/kicp.h's text (tests/gain_ref.py).  Everything is integer and the result is unique: np.array_equal, no tolerance
anywhere.  The grids are set with set_counts, so the shapes are exact.

What the cases cover (tests/gain_ref.py cases()): R = 1, 2, 63, 64, 65 - a wave takes 64 steps of a ray per trip - 128 and 361, the
largest window, whose bit plane fills the LDS a launch gets; windows of (2 R + 1)^2 bits, an odd number and so never a multiple of 32
(test_window_bits_never_fill_their_last_word); viewpoints in the four corners and on the four edges; grids of 1 x 1 and 1 x 70;
all-unknown, all-clear and all-occupied grids; rings of unknown cells round the viewpoint that many rays cross; occupied cells on
the disc's edge and just beyond it; a thin wall and a diagonal one; an unknown region shadowed by an obstacle; random grids of
70 x 50 and 130 x 100 with 30 % unknown and 10 % occupied; 1, 300 and duplicate viewpoints with unknown and occupied ones mixed in."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import frontier_ref as fr
import gain_ref as gr

pytestmark = pytest.mark.gpu

CASES = gr.cases()


def grid_for(width, height, cell=0.05):
    return K.OccupancyGrid(cell, 0.0, 0.0, width, height, 0.0, 1.0, 1.0)


def grid_of(occ):
    grid = grid_for(occ.shape[1], occ.shape[0])
    grid.set_counts(gr.counts_of(occ))
    return grid


def check(grid, occ, views, R, want, **kw):
    got = grid.gain(views, R, **kw)
    assert got.dtype == np.uint32 and got.shape == (len(views), K.GAIN_WORDS)
    bad = (got != want).any(axis=1)
    print("%d x %d, R = %d, %d viewpoints %s: %d rows differ" % (occ.shape[1], occ.shape[0], R, len(views), kw, bad.sum()))
    assert not bad.any(), (np.flatnonzero(bad)[:5], got[bad][:5], want[bad][:5])
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(name):
    occ, views, ranges = CASES[name]
    grid = grid_of(occ)
    assert np.array_equal(grid.occupancy(), occ)
    for R in ranges:
        want = gr.reference()[(name, R)]
        check(grid, occ, views, R, want)
        assert np.array_equal(K.gain_from_occupancy(occ, views, R), want)


def test_window_bits_never_fill_their_last_word():
    """(2 R + 1)^2 is odd: the last word of every window's plane is partly unused, at every R of the cases - and the counts over it are
    right on a plane where every bit of the disc is set: an all-unknown grid round one clear cell"""
    ranges = sorted({R for _, _, rs in CASES.values() for R in rs})
    assert {1, 2, 63, 64, 65, 128, 361} <= set(ranges) and all((2 * R + 1) ** 2 % 32 != 0 for R in ranges)
    for R in (1, 2, 5, 64, 65):
        side = 2 * R + 1
        occ = np.full((side, side), -1, dtype=np.int8)
        occ[R, R] = 0
        yy, xx = np.mgrid[-R:R + 1, -R:R + 1]
        disc = int((xx * xx + yy * yy <= R * R).sum()) - 1
        assert grid_of(occ).gain([(R, R)], R).tolist() == [[disc, 0, 0, 0]]


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
    counts[20:30, 30:40] = (0, 4)  # clear round the middle, at either min_observations
    grid = grid_for(W, H)
    grid.set_counts(counts)
    views = [(35, 25), (31, 21), (38, 28), (0, 0), (69, 49), (10, 10), (50, 40)]
    rows = {}
    for min_observations in (1, 3):
        occ = K.occupancy_from_counts(counts, min_observations)
        assert np.array_equal(grid.occupancy(min_observations), occ)
        for thresh in (0.0, 0.65, 1.0):
            want = gr.gain(occ, views, 12, thresh)
            check(grid, occ, views, 12, want, min_observations=min_observations, occupied_thresh=thresh)
            assert np.array_equal(K.gain_from_occupancy(occ, views, 12, min_observations, thresh), want)
            rows[(min_observations, thresh)] = want
    assert not np.array_equal(rows[(1, 0.65)], rows[(3, 0.65)]) and not np.array_equal(rows[(1, 0.0)], rows[(1, 1.0)])
    assert rows[(1, 0.65)][0, 0] > 0 and rows[(3, 0.65)][0, 0] > rows[(1, 0.65)][0, 0]


def test_handle_state():
    """one handle reused with N growing and shrinking and R changing; a gain call changes neither the plan nor the counters"""
    occ = CASES["random_130x100_views"][0]
    grid = grid_of(occ)
    for n, R, seed in ((1, 20, 1), (300, 3, 2), (7, 64, 3), (40, 9, 4), (2, 128, 5), (120, 1, 6)):
        views = gr.spread_views(occ, n, seed)
        if n <= 7:
            views[0] = 50 * 130 + 65
        want = K.gain_from_occupancy(occ, views, R)
        check(grid, occ, views, R, want)
        if n * R * R <= 12000:
            assert np.array_equal(want, gr.gain(occ, views, R))
    assert grid.gain([], 5).shape == (0, 4) and grid.gain(np.zeros((0, 2), dtype=np.int64), 5).shape == (0, 4)
    assert not grid.has_plan()
    grid.gain([0, 1, 2], 7)
    assert not grid.has_plan()
    costmap = np.where(occ > 65, 254, np.where(occ < 0, 255, 0)).astype(np.uint8)
    goal = tuple(int(v) for v in np.argwhere(costmap == 0)[len(costmap) // 2][::-1])
    pot = grid.potential_of_costmap(costmap, K.plan_weights(), [goal])
    start = K.arc_start((goal[0] + 0.5) * 0.05, (goal[1] + 0.5) * 0.05, 0.3)
    arcs = K.arc_steps(np.linspace(0.1, 0.6, 12), np.linspace(-1.0, 1.0, 12), 0.1)
    footprint = K.footprint_box(-0.05, 0.05, -0.05, 0.05, 0.05)
    before, counts = grid.score_arcs(start, arcs, 20, footprint), grid.counts()
    views = gr.spread_views(occ, 50, 8)
    check(grid, occ, views, 15, K.gain_from_occupancy(occ, views, 15))
    assert grid.has_plan() and np.array_equal(grid.score_arcs(start, arcs, 20, footprint), before) and np.array_equal(grid.counts(), counts)
    assert np.array_equal(before, K.score_arcs_from_plan(K.plan_q(costmap, K.plan_weights()), pot, 0.05, 0.0, 0.0, start, arcs, 20, footprint))


def test_a_real_drive():
    """260 x 200 cells of 0.1 m from a few integrated synthetic frames: the viewpoints are the frontiers' best cells under a plan from
    the robot's cell - word 9 of their rows, passed as it is - at the sensor's own range of 60 cells and at 20"""
    cfg, frames, places = fr.room_drive()
    grid = K.OccupancyGrid(*cfg)
    for pts, pose, sensor in frames:
        assert grid.integrate(pts, pose, sensor)[0] > 500
    counts = grid.counts()
    robot = (int(np.floor((places[-1][0] + 0.2 + 13.0) / 0.1)), int(np.floor((places[-1][1] + 10.0) / 0.1)))
    grid.potential(K.nav2_cost_table(0.1, 3, 0.15, 3.0), K.plan_weights(), [robot])
    rows = grid.frontiers(use_plan=True)
    views = rows[:, 9]
    assert len(views) >= 2
    occ = grid.occupancy()
    for R in (20, 60):
        got = grid.gain(views, R)
        host = K.gain_from_occupancy(occ, views, R)
        print("R = %d: %d frontiers' best cells see %s unknown cells" % (R, len(views), got[:, 0].tolist()[:12]))
        assert np.array_equal(got, host)
        assert (got[:, 3] == 0).all() and (got[:, 0] > 0).all()  # a frontier cell is clear and has an unknown edge neighbour, which a ray sees
    few = views[:3]
    assert np.array_equal(grid.gain(few, 20), gr.gain(occ, few, 20))
    assert np.array_equal(grid.gain(np.stack([views % 260, views // 260], axis=1), 60), got)  # the same viewpoints as (x, y)
    assert np.array_equal(grid.counts(), counts) and grid.has_plan()


def test_argument_errors_on_the_device():
    occ, views, want = gr.pinned_9x7()
    grid = grid_of(occ)

    def code(v=views, **kw):
        args = dict(range_cells=3)
        args.update(kw)
        with pytest.raises(K.KicpError) as e:
            grid.gain(v, **args)
        return e.value.code, str(e.value)

    for kw in (dict(min_observations=0), dict(min_observations=-1), dict(occupied_thresh=-0.01), dict(occupied_thresh=1.01), dict(occupied_thresh=float("nan")),
               dict(range_cells=0), dict(range_cells=362)):
        assert code(**kw)[0] == K.KICP_ERR_ARG, kw
    for bad in ([(3, 3), (9, 0)], [(0, 7)], [5, -1], [1 << 32]):
        assert code(bad)[0] == K.KICP_ERR_ARG
    c, message = code([5, 62, 63, 7, 900])
    assert c == K.KICP_ERR_ARG and "viewpoint 2 " in message and "63" in message
    u32 = C.POINTER(C.c_uint)
    cfg = K.GainConfig(1, 0.65, 3)
    v = np.array([y * 9 + x for x, y in views], dtype=np.uint32)
    out = np.full(24, 77, dtype=np.uint32)
    pv, po = v.ctypes.data_as(u32), out.ctypes.data_as(u32)
    f = K.lib().kicp_grid_gain
    assert f(grid._h, C.byref(cfg), pv, 5, po, 20) == K.KICP_OK and np.array_equal(out[:20].reshape(5, 4), want[3]) and (out[20:] == 77).all()
    bad_view = v.copy()
    bad_view[4] = 63
    for args in ((None, C.byref(cfg), pv, 5, po, 20), (grid._h, None, pv, 5, po, 20), (grid._h, C.byref(cfg), None, 5, po, 20), (grid._h, C.byref(cfg), pv, 5, None, 20),
                 (grid._h, C.byref(cfg), pv, 5, po, 19), (grid._h, C.byref(cfg), pv, 5, po, 24), (grid._h, C.byref(cfg), pv, 0, po, 20),
                 (grid._h, C.byref(K.GainConfig(0, 0.65, 3)), pv, 5, po, 20), (grid._h, C.byref(K.GainConfig(1, 1.5, 3)), pv, 5, po, 20),
                 (grid._h, C.byref(K.GainConfig(1, 0.65, 0)), pv, 5, po, 20), (grid._h, C.byref(K.GainConfig(1, 0.65, 362)), pv, 5, po, 20),
                 (grid._h, C.byref(cfg), bad_view.ctypes.data_as(u32), 5, po, 20)):
        out[:] = 77
        assert f(*args) == K.KICP_ERR_ARG
        assert (out == 77).all()  # nothing written
    assert b"viewpoint 4 " in K.lib().kicp_last_error()
    assert f(grid._h, C.byref(cfg), None, 0, None, 0) == K.KICP_OK
    for R in want:
        assert np.array_equal(grid.gain(views, R), want[R])  # the handle is unharmed, and the header's example holds on the device
