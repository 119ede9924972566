"""The transient obstacles on the GPU: kicp_grid_transients and kicp_grid_transients_device on grids whose counters the test sets,
against the restatement (tests/transient_ref.py) and the host entry on the scenes of tests/transient_cases.py and on frames of 20 000
returns - np.array_equal, no tolerance; what a call leaves behind and what it must not touch; and the switch: clearance, costmap and
potential with the plane's cells as sources against the pure-host entries over the patched readout, an arc that collides with a
transient, and everything that must ignore the plane."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import transient_cases as tc
import transient_ref as tr

pytestmark = pytest.mark.gpu

CASES = tc.cases()


def _reference(s, **kw):
    return tr.transients(s["cfg"], s["counts"], s["points"], s["pose"], s["sensor"], **dict(s["params"], **kw))


@pytest.fixture(scope="module")
def reference():
    """name -> (rows, labels, plane, stats) by the restatement - computed once"""
    return {name: _reference(s) for name, s in CASES.items()}


def _grid(s):
    """a grid with the scene's counters that has integrated a frame before, so that it has a frame count and a last window to keep"""
    grid = K.OccupancyGrid(*s["args"])
    grid.integrate(np.array([[0.3, 0.2, 0.5]]), tc.IDENTITY)
    grid.set_counts(s["counts"])
    assert grid.info()["frames"] == 1
    return grid


def _run(grid, s, device, **kw):
    """-> (rows, labels, stats) of one of the two device entries"""
    p = dict(s["params"], **kw)
    if not device:
        return grid.transients(s["points"], s["pose"], s["sensor"], return_labels=True, return_stats=True, **p)
    pts = s["points"]
    frame = K.DeviceFrame(pts if len(pts) else np.zeros((1, 3)))
    return grid.transients_device(frame, s["pose"], s["sensor"], n=len(pts), return_labels=True, return_stats=True, **p)


def _state(grid):
    return grid.counts(), grid.info()["frames"], grid.last_window(), grid.has_plan()


def _same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def _check(got, plane, want):
    rows, labels, stats = got
    want_rows, want_labels, want_plane, want_stats = want
    print("stats %s (restatement %s), %d rows (restatement %d)" % (stats, want_stats, len(rows), len(want_rows)))
    assert rows.dtype == np.uint64 and labels.dtype == np.uint32 and plane.dtype == np.uint8
    assert stats == want_stats
    assert np.array_equal(labels, want_labels), np.argwhere(labels != want_labels)[:5]
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(plane, want_plane)


@pytest.mark.parametrize("name", sorted(CASES))
def test_scenes(name, reference):
    s = CASES[name]
    grid = _grid(s)
    assert not grid.transient_plane().any() and not grid.uses_transients()  # before the first call
    before = _state(grid)
    host = K.transients_from_counts(s["counts"], s["args"], s["points"], s["pose"], s["sensor"], return_labels=True, return_stats=True, return_plane=True, **s["params"])
    for device in (False, True):
        got = _run(grid, s, device)
        plane = grid.transient_plane()
        _check(got, plane, reference[name])
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]) and got[2] == host[2] and np.array_equal(plane, host[3])
        assert _same_state(_state(grid), before)
    # another min_size on the same handle: the rows and the plane follow, the labels stay
    want = _reference(s, min_size=3)
    got = _run(grid, s, True, min_size=3)
    _check(got, grid.transient_plane(), want)
    if name == "5000_returns_in_one_cell":
        assert got[0].shape[0] == 0 and _run(grid, s, False)[0][0, 2] == 5007
    if name == "no_points":
        assert (got[1] == tr.NONE).all() and got[2] == (0, 0, 0, 0)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_a_frame_of_20000_returns(seed):
    s = tc.random_scene(260, 200, seed, 20000)
    want = _reference(s)
    assert want[3][0] > 15000 and len(want[0]) > 50 and want[0][:, 1].max() > 8
    grid = _grid(s)
    for device in (True, False):
        _check(_run(grid, s, device), grid.transient_plane(), want)


def test_no_residue_between_calls(reference):
    """A, then B at another place, then A again on one handle: only the last call's cells are in the plane, and A's arrays come back -
    nothing is left in the counts, the flags or the plane"""
    a, b = CASES["along_a_tile_border"], CASES["two_blobs_touch_at_a_corner"]
    grid = _grid(a)
    first = _run(grid, a, True)
    plane_a = grid.transient_plane()
    _check(first, plane_a, reference["along_a_tile_border"])
    _check(_run(grid, b, False), grid.transient_plane(), reference["two_blobs_touch_at_a_corner"])
    assert not (grid.transient_plane() & plane_a).any()
    again = _run(grid, a, False)
    _check(again, grid.transient_plane(), reference["along_a_tile_border"])
    # a frame without a point, and clear(), empty the plane; the switch survives clear()
    grid.use_transients(True)
    _run(grid, CASES["no_points"], True)
    assert not grid.transient_plane().any()
    _run(grid, a, True)
    assert grid.transient_plane().any()
    grid.clear()
    assert not grid.transient_plane().any() and grid.uses_transients()
    grid.use_transients(False)
    assert not grid.uses_transients()


def test_the_capacity_path_has_replaced_the_plane(reference):
    s = CASES["random_65x63"]
    want_rows, _, want_plane, _ = reference["random_65x63"]
    grid = _grid(s)
    cfg = K.TransientConfig(**s["params"])
    pts = np.ascontiguousarray(s["points"])
    sensor = np.ascontiguousarray(s["sensor"])
    dp, u64 = C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
    rows, n = np.full((3, 10), 77, dtype=np.uint64), C.c_size_t(99)
    rc = K.lib().kicp_grid_transients(grid._h, pts.ctypes.data_as(dp), len(pts), s["pose"].ctypes.data_as(dp), sensor.ctypes.data_as(dp), C.byref(cfg),
                                      rows.ctypes.data_as(u64), 2, C.byref(n), None, 0, None)
    assert rc == K.KICP_ERR_CAPACITY and n.value == len(want_rows) > 2
    assert np.array_equal(rows[:2], want_rows[:2]) and (rows[2] == 77).all()
    assert np.array_equal(grid.transient_plane(), want_plane)
    # a call that fails its argument checks leaves the plane as it was
    n.value = 99
    bad = K.TransientConfig(1, 101, 1, 1)
    rc = K.lib().kicp_grid_transients(grid._h, pts.ctypes.data_as(dp), len(pts), s["pose"].ctypes.data_as(dp), sensor.ctypes.data_as(dp), C.byref(bad),
                                      rows.ctypes.data_as(u64), 3, C.byref(n), None, 0, None)
    assert rc == K.KICP_ERR_ARG and n.value == 0 and np.array_equal(grid.transient_plane(), want_plane)
    with pytest.raises(K.KicpError):
        grid.transients(s["points"], s["pose"], s["sensor"], min_points=0)
    assert np.array_equal(grid.transient_plane(), want_plane)


R, RECT = 6, (17, 9, 40, 33)


def _plan_arrays(grid, table, weight, goals):
    """every array a planner reads off the grid, for the full grid and the off-centre rectangle, in both unknown modes"""
    out = {}
    for unknown in (False, True):
        for rect in (None, RECT):
            out["clearance", unknown, rect] = grid.clearance(R, unknown_is_obstacle=unknown, rect=rect)
            for inflate in (False, True):
                out["costmap", unknown, inflate, rect] = grid.costmap(table, unknown_is_obstacle=unknown, inflate_unknown=inflate, rect=rect)
    out["potential"] = grid.potential(table, weight, goals)
    return out


def test_the_switch():
    s = tc.switch_scene()
    grid = _grid(s)
    table, weight, goals = K.nav2_cost_table(0.1, R, 0.15, 3.0), K.plan_weights(), [(45, 35), (5, 60)]
    before = _plan_arrays(grid, table, weight, goals)
    frontiers, gain = grid.frontiers(return_labels=True), grid.gain([(45, 35), (20, 20)], 30)
    occupancy = grid.occupancy()
    _, _, want_plane, _ = _reference(s)
    grid.transients(s["points"], s["pose"], s["sensor"], **s["params"])
    assert np.array_equal(grid.transient_plane(), want_plane) and want_plane.sum() > 20
    # off: every array equals the one taken before the first transient call
    off = _plan_arrays(grid, table, weight, goals)
    assert all(np.array_equal(off[k], before[k]) for k in before)
    grid.use_transients(True)
    assert grid.uses_transients()
    on = _plan_arrays(grid, table, weight, goals)
    patched = tr.patched_readout(s["counts"], want_plane)
    differs = 0
    for key, got in on.items():
        if key[0] == "clearance":
            want = K.clearance_from_occupancy(patched, R, unknown_is_obstacle=key[1], rect=key[2])
        elif key[0] == "costmap":
            want = K.costmap_from_occupancy(patched, table, unknown_is_obstacle=key[1], inflate_unknown=key[2], rect=key[3])
            if key[3] is None:
                assert (got[want_plane == 1] == 254).all()
        else:
            want = K.potential_from_costmap(on["costmap", False, False, None], weight, goals)
        assert got.dtype == want.dtype and np.array_equal(got, want), key
        differs += not np.array_equal(got, before[key])
    assert differs == len(on)  # the transients change every one of them
    # the rectangle's result is the full grid's restricted to it
    x0, y0, w, h = RECT
    assert np.array_equal(on["costmap", False, True, RECT], on["costmap", False, True, None][y0:y0 + h, x0:x0 + w])
    # what ignores the plane whatever the switch says
    again = grid.frontiers(return_labels=True)
    assert np.array_equal(again[0], frontiers[0]) and np.array_equal(again[1], frontiers[1])
    assert np.array_equal(grid.gain([(45, 35), (20, 20)], 30), gain) and np.array_equal(grid.occupancy(), occupancy) and np.array_equal(grid.counts(), s["counts"])
    assert np.array_equal(grid.potential_of_costmap(before["costmap", False, False, None], weight, goals), before["potential"])
    # a plan is a snapshot: a later detection without a transient neither changes nor invalidates it
    plan = grid.potential(table, weight, goals)
    start, arcs, footprint = K.arc_start(0.5, 0.5, 0.3), K.arc_steps([0.5, 0.4], [0.0, 0.6], 0.2), K.footprint_box(-0.1, 0.1, -0.1, 0.1, 0.1)
    scored = grid.score_arcs(start, arcs, 20, footprint)
    _run(grid, CASES["no_points"] | dict(args=s["args"]), True)
    assert not grid.transient_plane().any() and grid.has_plan() and np.array_equal(grid.score_arcs(start, arcs, 20, footprint), scored)
    assert np.array_equal(plan, on["potential"])
    # the plane is empty again: on equals off
    empty = _plan_arrays(grid, table, weight, goals)
    assert all(np.array_equal(empty[k], before[k]) for k in before)


def test_an_arc_across_a_transient_collides():
    """free space, a box of returns across the way from cell (10, 30) to the goal (60, 30): the straight arc drives through under a plan
    made with the switch off and stops in front of the box under one made with it on"""
    args = tc.grid_args(70, 70)
    s = tc.scene(args, tc.free_counts(70, 70), [(x, y, 3) for x in (30, 31) for y in range(27, 34)], sensor_cell=(10, 30), min_size=4)
    grid = _grid(s)
    rows = grid.transients(s["points"], s["pose"], s["sensor"], **s["params"])
    assert rows[:, :3].tolist() == [[27 * 70 + 30, 14, 42]] and rows[0, 9] >> 32 == 20 * 20
    table, weight = K.nav2_cost_table(0.1, 3, 0.1, 3.0), K.plan_weights()
    start = K.arc_start(args[1] + 10.5 * 0.1, args[2] + 30.5 * 0.1, 0.0)
    arcs, footprint = np.array([[0.1, 0.0, 1.0, 0.0]]), np.zeros((1, 2))
    grid.potential(table, weight, [(60, 30)])
    off = grid.score_arcs(start, arcs, 40, footprint)
    grid.use_transients(True)
    pot = grid.potential(table, weight, [(60, 30)])
    on = grid.score_arcs(start, arcs, 40, footprint)
    print("free_steps off %d, on %d" % (off[0, 0], on[0, 0]))
    assert off[0, 0] == 40 and on[0, 0] == 18  # cells 11 .. 28 are free; 29 is at distance 1 of the box: inscribed, lethal to the planner
    assert pot[30, 30] == 0xFFFFFFFF and pot[30, 20] != 0xFFFFFFFF  # the way round the box is open
    assert grid.occupancy()[30, 30] == 0
