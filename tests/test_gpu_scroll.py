"""The scroll on the GPU: kicp_grid_scroll and kicp_elev_scroll against the restatement (tests/scroll_ref.py) on the shapes and shifts
of tests/scroll_cases.py - np.array_equal, no tolerance -, the origin bit for bit, that a scrolled handle is indistinguishable from one
created at the reported configuration with the shifted counters, the plan's invalidation, the translated last window, kicp_grid_follow
and kicp_elev_follow, the rectangles of counters with a paging round trip, and that nothing stale is left for the next frame."""
import ctypes as C
import struct

import numpy as np
import pytest

import kinematic_icp_amd as K
import clearance_ref as cr
import frontier_ref as fr
import gain_ref as gnr
import grid_cases as gc
import grid_ref as gr
import potential_ref as pr
import scroll_cases as sc
import scroll_ref as sr
import transient_cases as tc
import transient_ref as tr

pytestmark = pytest.mark.gpu

SHAPES = sc.SMALL + [sc.LARGE]


def _bits(x):
    return struct.pack("<d", x)


def _code(fn, *a, **kw):
    with pytest.raises(K.KicpError) as e:
        fn(*a, **kw)
    return e.value.code


def _grid(width, height, cell=0.1, origin=(-1.0, -2.0), max_ray=3.0):
    return K.OccupancyGrid(cell, origin[0], origin[1], width, height, 0.0, 1.0, max_ray)


# ---- 1. the shifts of the three planes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_counters_shift(shape):
    width, height = shape
    grid, counts = _grid(width, height), sc.counters(width, height)
    for dx, dy in sc.shifts(width, height):
        grid.set_counts(counts)
        grid.scroll(dx, dy)
        got = grid.counts()
        assert np.array_equal(got, sr.shift(counts, dx, dy)), (dx, dy, np.argwhere(got != sr.shift(counts, dx, dy))[:4])
        if abs(dx) >= width or abs(dy) >= height:
            assert not got.any()
    grid.set_counts(counts)
    grid.scroll(0, 0)
    assert np.array_equal(grid.counts(), counts)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_columns_shift(shape):
    width, height = shape
    layer, columns = K.ElevationLayer(0.1, -1.0, -2.0, width, height, -1.0, 0.0625, 3.0), sc.columns(width, height)
    for dx, dy in sc.shifts(width, height):
        layer.set_columns(columns)
        layer.scroll(dx, dy)
        got = layer.columns()
        assert np.array_equal(got, sr.shift(columns, dx, dy)), (dx, dy, np.argwhere(got != sr.shift(columns, dx, dy))[:4])
        if abs(dx) >= width or abs(dy) >= height:
            assert not got.any()
    layer.set_columns(columns)
    layer.scroll(0, 0)
    assert np.array_equal(layer.columns(), columns)


# the alignments of a byte plane's source against a 16-byte chunk, the last surviving row and column, and the emptying shifts
PLANE_SHIFTS = [(1, 0), (-1, 0), (3, 2), (-4, -1), (5, 0), (15, 1), (-16, 0), (17, -3), (0, 1), (0, -5), (89, 0), (0, 69), (-89, -69), (90, 0), (0, -70), (93, 73)]


def test_transient_plane_shift():
    s = tc.switch_scene()  # 90 x 70
    want_plane = tr.transients(s["cfg"], s["counts"], s["points"], s["pose"], s["sensor"], **s["params"])[2]
    assert want_plane.sum() > 20
    for dx, dy in PLANE_SHIFTS:
        grid = K.OccupancyGrid(*s["args"])
        grid.set_counts(s["counts"])
        grid.transients(s["points"], s["pose"], s["sensor"], **s["params"])
        assert np.array_equal(grid.transient_plane(), want_plane)
        grid.use_transients(True)
        grid.scroll(dx, dy)
        assert np.array_equal(grid.transient_plane(), sr.shift(want_plane, dx, dy)), (dx, dy)
        assert np.array_equal(grid.counts(), sr.shift(s["counts"], dx, dy)) and grid.uses_transients()
        if abs(dx) >= 90 or abs(dy) >= 70:
            assert not grid.transient_plane().any()
    grid.scroll(0, 0)
    assert np.array_equal(grid.transient_plane(), sr.shift(want_plane, *PLANE_SHIFTS[-1]))
    # a handle that never looked for transients has no plane to shift, before or after
    grid = K.OccupancyGrid(*s["args"])
    grid.scroll(3, 3)
    assert not grid.transient_plane().any()


# ---- 2. the origin ----------------------------------------------------------------------------------------------------------------
def test_origin_bit_for_bit():
    for cell, ox, oy in ((0.05, -40.0, -40.0), (0.1, 0.30000000000000004, -7.7), (1.0 / 3.0, 1e6 + 0.1, -1e-3)):
        grid = K.OccupancyGrid(cell, ox, oy, 37, 29, 0.1, 1.5, 1.0)
        layer = K.ElevationLayer(cell, ox, oy, 37, 29, -1.0, 0.0625, 1.0)
        grid.integrate(np.array([[0.3, 0.2, 0.5]]), gc.IDENTITY)
        before = grid.info()
        grid.scroll(64, -3)
        info = grid.info()
        assert _bits(info["origin_x"]) == _bits(sr.origin(ox, 64, cell)) and _bits(info["origin_y"]) == _bits(sr.origin(oy, -3, cell))
        want_x, want_y = sr.origin(ox, 64, cell), sr.origin(oy, -3, cell)
        layer.scroll(64, -3)
        rng = np.random.default_rng(5)
        for _ in range(20):  # twenty in a row with mixed signs, emptying ones among them
            dx, dy = (int(v) for v in rng.integers(-70, 71, 2))
            grid.scroll(dx, dy), layer.scroll(dx, dy)
            want_x, want_y = sr.origin(want_x, dx, cell), sr.origin(want_y, dy, cell)
        info, linfo = grid.info(), layer.info()
        assert _bits(info["origin_x"]) == _bits(want_x) and _bits(info["origin_y"]) == _bits(want_y)
        assert _bits(linfo["origin_x"]) == _bits(want_x) and _bits(linfo["origin_y"]) == _bits(want_y)  # the same sequence, the same origin
        for key in ("cell", "width", "height", "z_min", "z_max", "max_ray", "reach", "frames"):
            assert _bits(float(info[key])) == _bits(float(before[key])), key
        assert info["frames"] == 1 and linfo["frames"] == 0 and linfo["slab"] == 0.0625 and linfo["z_origin"] == -1.0
    # an origin that would not be finite: refused, nothing changed
    grid = K.OccupancyGrid(1e300, 1e308, 0.0, 4, 4, 0.0, 1.0, 1e300)
    counts = sc.counters(4, 4)
    grid.set_counts(counts)
    assert _code(grid.scroll, 2147483647, 0) == K.KICP_ERR_ARG
    assert grid.info()["origin_x"] == 1e308 and np.array_equal(grid.counts(), counts)
    assert K.lib().kicp_grid_scroll(None, 1, 0) == K.KICP_ERR_ARG and K.lib().kicp_elev_scroll(None, 1, 0) == K.KICP_ERR_ARG


# ---- 3. no hidden state -----------------------------------------------------------------------------------------------------------
R = 6
VIEWS = [(100, 80), (20, 20), (150, 100)]


def _arrays(grid, table, weight, goals, plan=True):
    """everything a caller reads off a grid"""
    out = {"counts": grid.counts(), "occupancy": grid.occupancy(), "occupancy2": grid.occupancy(2), "clearance": grid.clearance(R),
           "clearance_rect": grid.clearance(R, unknown_is_obstacle=True, rect=(17, 9, 40, 33)), "costmap": grid.costmap(table, inflate_unknown=True),
           "frontiers": grid.frontiers(return_labels=True)[0], "labels": grid.frontiers(return_labels=True)[1], "gain": grid.gain(VIEWS, 30),
           "window": np.array(grid.last_window())}
    if plan:
        out["potential"] = grid.potential(table, weight, goals, inflate_unknown=True)
        out["frontiers_plan"] = grid.frontiers(use_plan=True)
    return out


def _restated(counts, table, weight, goals):
    occ = gr.occupancy(counts)
    cost = cr.costmap(occ, table, inflate_unknown=True, clear=cr.clearance_by_offsets(occ, R))
    pot = pr.potential_sweeps(cost, weight, goals)[0]
    return {"counts": counts, "occupancy": occ, "occupancy2": gr.occupancy(counts, 2), "clearance": cr.clearance_by_offsets(occ, R),
            "clearance_rect": cr.clearance_by_offsets(occ, R, unknown_is_obstacle=True)[9:9 + 33, 17:17 + 40], "costmap": cost,
            "frontiers": fr.frontiers(occ)[0], "labels": fr.frontiers(occ)[1], "gain": gnr.gain(occ, VIEWS, 30), "potential": pot,
            "frontiers_plan": fr.frontiers(occ, potential=pot)[0]}


def _same(got, want, what):
    for key in want:
        assert np.array_equal(got[key], want[key]), (what, key)


def _unclipped_window(cfg, pose, sensor):
    _, _, (sx, sy) = gr.endpoints(cfg, np.zeros((0, 3)), pose, sensor)
    return int(sx) - cfg["reach"], int(sy) - cfg["reach"], 2 * cfg["reach"] + 1


def test_no_hidden_state():
    cfg, frames = gc.random_drive()
    frames = [frames[k] for k in (0, 1, 2, 3, 1)]  # three frames, the scroll, two more - the first of them near the border
    args = (cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_min"], cfg["z_max"], cfg["max_ray"])
    table, weight, goals = K.nav2_cost_table(0.1, R, 0.15, 3.0), K.plan_weights(unknown_weight=60), [(100, 80), (30, 120)]
    a, counts = K.OccupancyGrid(*args), np.zeros((cfg["height"], cfg["width"], 2), dtype=np.uint16)
    for pts, pose, sensor in frames[:3]:
        a.integrate(pts, pose, sensor), gr.integrate(cfg, counts, pts, pose, sensor)
    # a transient plane to carry along: the fourth frame against the counters so far
    tparams = dict(min_observations=1, free_max=65, min_points=1, min_size=1)
    a.transients(*frames[3], **tparams)
    plane = tr.transients(cfg, counts, *frames[3], **tparams)[2]
    assert np.array_equal(a.transient_plane(), plane) and plane.sum() > 5
    now, b = dict(cfg), None
    for step, (dx, dy) in enumerate(((5, -3), (-5, 3))):  # there and back: the live and the spare buffer swap in both directions
        a.scroll(dx, dy)
        counts, plane = sr.shift(counts, dx, dy), sr.shift(plane, dx, dy)
        now = dict(now, origin_x=sr.origin(now["origin_x"], dx, now["cell"]), origin_y=sr.origin(now["origin_y"], dy, now["cell"]))
        info = a.info()
        assert _bits(info["origin_x"]) == _bits(now["origin_x"]) and _bits(info["origin_y"]) == _bits(now["origin_y"]) and info["frames"] == 3 + 2 * step
        b = K.OccupancyGrid(info["cell"], info["origin_x"], info["origin_y"], info["width"], info["height"], info["z_min"], info["z_max"], info["max_ray"])
        b.set_counts(counts)
        assert np.array_equal(a.transient_plane(), plane) and not a.has_plan()
        # the switch on: the shifted plane's cells are sources on A (B has no plane to give it)
        a.use_transients(True)
        patched = tr.patched_readout(counts, plane)
        assert np.array_equal(a.costmap(table, inflate_unknown=True), cr.costmap(patched, table, inflate_unknown=True, clear=cr.clearance_by_offsets(patched, R)))
        assert np.array_equal(a.clearance(R), cr.clearance_by_offsets(patched, R))
        a.use_transients(False)
        for pts, pose, sensor in frames[3:]:
            sa, sb = a.integrate(pts, pose, sensor), b.integrate(pts, pose, sensor)
            assert sa == sb == gr.integrate(now, counts, pts, pose, sensor)
        got_a, got_b, want = _arrays(a, table, weight, goals), _arrays(b, table, weight, goals), _restated(counts, table, weight, goals)
        _same(got_a, want, "A against the restatement"), _same(got_b, got_a, "B against A")
        assert tuple(got_a["window"]) == cr.window(now, frames[4][1], frames[4][2]) and got_a["window"][2] > 0
        assert a.info()["frames"] == b.info()["frames"] + 3 + 2 * step
        # the next detection on both: no stale cell index in the transient scratch
        ra, rb = a.transients(*frames[0], **tparams), b.transients(*frames[0], **tparams)
        want_t = tr.transients(now, counts, *frames[0], **tparams)
        assert np.array_equal(ra, rb) and np.array_equal(ra, want_t[0]) and np.array_equal(a.transient_plane(), want_t[2])
        assert np.array_equal(b.transient_plane(), want_t[2])
        plane = want_t[2]


# ---- 4. the plan --------------------------------------------------------------------------------------------------------------------
def test_a_scroll_invalidates_the_plan():
    s = tc.switch_scene()
    grid = K.OccupancyGrid(*s["args"])
    grid.set_counts(s["counts"])
    table, weight, goals = K.nav2_cost_table(0.1, R, 0.15, 3.0), K.plan_weights(), [(45, 35), (5, 60)]
    start, arcs, footprint = K.arc_start(0.5, 0.5, 0.3), K.arc_steps([0.5, 0.4], [0.0, 0.6], 0.2), K.footprint_box(-0.1, 0.1, -0.1, 0.1, 0.1)
    branch, steps, prims = [2, 2], [5, 5], K.arc_steps([0.5, 0.4, 0.5, 0.3], [0.0, 0.6, -0.4, 0.2], 0.2)
    pot = grid.potential(table, weight, goals)
    scored, tree, fronts = grid.score_arcs(start, arcs, 20, footprint), grid.score_arc_tree(start, branch, steps, prims, footprint), grid.frontiers(use_plan=True)
    grid.scroll(0, 0)  # keeps the plan and its results
    assert grid.has_plan() and np.array_equal(grid.score_arcs(start, arcs, 20, footprint), scored)
    assert np.array_equal(grid.score_arc_tree(start, branch, steps, prims, footprint), tree) and np.array_equal(grid.frontiers(use_plan=True), fronts)
    assert grid.follow(s["args"][1] + 4.5, s["args"][2] + 3.5, 10, 8) == (0, 0) and grid.has_plan()  # a follow that does not scroll keeps it too
    grid.scroll(2, -1)
    assert not grid.has_plan()
    assert _code(grid.score_arcs, start, arcs, 20, footprint) == K.KICP_ERR_ARG
    assert _code(grid.score_arc_tree, start, branch, steps, prims, footprint) == K.KICP_ERR_ARG
    assert _code(grid.frontiers, use_plan=True) == K.KICP_ERR_ARG
    assert len(grid.frontiers()) > 0  # without the plan the frontiers are there
    again = grid.potential(table, weight, goals)
    assert grid.has_plan() and not np.array_equal(again, pot)
    shifted = sr.shift(s["counts"], 2, -1)
    want = K.potential_from_costmap(K.costmap_from_occupancy(gr.occupancy(shifted), table), weight, goals)
    assert np.array_equal(again, want)
    grid.score_arcs(start, arcs, 20, footprint), grid.score_arc_tree(start, branch, steps, prims, footprint)
    assert np.array_equal(grid.frontiers(use_plan=True), fr.frontiers(gr.occupancy(shifted), potential=want)[0])
    grid.scroll(1000, 0)  # an emptying scroll invalidates it as well
    assert not grid.has_plan()


# ---- 5. the last window -------------------------------------------------------------------------------------------------------------
def test_last_window_is_translated():
    cfg, frames = gc.random_drive()
    args = (cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_min"], cfg["z_max"], cfg["max_ray"])
    pts, pose, sensor = frames[1]
    x0, y0, side = _unclipped_window(cfg, pose, sensor)
    layer = K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], -1.0, 0.0625, cfg["max_ray"])
    for dx, dy in ((3, -2), (-70, 0), (0, 90), (100, 100), (x0 + side, 0), (x0 + side - 1, 0), (0, y0 - 160), (0, y0 - 159), (-300, 5), (2000, 2000)):
        grid = K.OccupancyGrid(*args)
        assert grid.last_window() == (0, 0, 0, 0)
        grid.scroll(1, 1)
        assert grid.last_window() == (0, 0, 0, 0)  # no frame yet: nothing to translate
        grid.scroll(-1, -1)
        cfg1 = dict(cfg, origin_x=grid.info()["origin_x"], origin_y=grid.info()["origin_y"])
        grid.integrate(pts, pose, sensor)
        wx0, wy0, _ = _unclipped_window(cfg1, pose, sensor)
        assert grid.last_window() == sr.window(wx0, wy0, side, 0, 0, 200, 160) == cr.window(cfg1, pose, sensor)
        grid.scroll(dx, dy)
        assert grid.last_window() == sr.window(wx0, wy0, side, dx, dy, 200, 160), (dx, dy)
    assert sr.window(x0, y0, side, x0 + side, 0, 200, 160) == (0, 0, 0, 0) and sr.window(x0, y0, side, x0 + side - 1, 0, 200, 160)[2] == 1  # wholly outside, one column
    # a window pushed beyond 2^30 cells is forgotten, as on a fresh handle: the way back does not bring it
    grid.scroll(-2000, -2000), grid.scroll((1 << 30) + 500, 0), grid.scroll(-(1 << 30) - 500, 0)
    assert grid.last_window() == (0, 0, 0, 0)
    grid.integrate(pts, pose, sensor)
    assert grid.last_window()[2] > 0
    layer.integrate(pts, pose, sensor)
    layer.scroll(-70, 12)
    assert layer.last_window() == sr.window(x0, y0, side, -70, 12, 200, 160)
    layer.scroll(5000, 0)
    assert layer.last_window() == (0, 0, 0, 0)


# ---- 6. following -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grid", "layer"])
def test_follow(kind):
    width, height, cell, ox, oy, margin, step = 64, 48, 0.1, -3.2, -2.4, 10, 8
    if kind == "grid":
        h, state, fill = _grid(width, height, cell, (ox, oy)), sc.counters(width, height), "set_counts"
        read = h.counts
    else:
        h, state, fill = K.ElevationLayer(cell, ox, oy, width, height, -1.0, 0.0625, 3.0), sc.columns(width, height), "set_columns"
        read = h.columns
    getattr(h, fill)(state)
    at = lambda cx, cy: (ox + (cx + 0.5) * cell, oy + (cy + 0.5) * cell)  # noqa: E731
    # inside the band, its four corners included: nothing moves, by bytes
    for cx, cy in ((10, 10), (53, 37), (10, 37), (53, 10), (30, 20)):
        assert sr.follow(*at(cx, cy), ox, oy, cell, width, height, margin, step) == (0, 0)
        assert h.follow(*at(cx, cy), margin, step) == (0, 0)
        assert np.array_equal(read(), state) and _bits(h.info()["origin_x"]) == _bits(ox) and _bits(h.info()["origin_y"]) == _bits(oy)
    # a position that is not finite, a cell beyond 2^30, a bad margin or step: refused, the bytes unchanged
    for x, y, m, s in ((float("nan"), 0.0, margin, step), (0.0, float("inf"), margin, step), (-float("inf"), 0.0, margin, step), (1e9, 0.0, margin, step),
                       (0.0, -1.2e8, margin, step), (0.0, 0.0, 0, step), (0.0, 0.0, margin, 0), (0.0, 0.0, 20, 9), (0.0, 0.0, 24, 1)):
        assert _code(h.follow, x, y, m, s) == K.KICP_ERR_ARG, (x, y, m, s)
        assert np.array_equal(read(), state) and _bits(h.info()["origin_x"]) == _bits(ox)
    assert h.follow(0.0, 0.0, 20, 8) == (0, 0)  # 2 * 20 + 8 == 48: accepted
    # at both margins on both axes, and beyond: what kicp_follow_shift says for the cell the grid's arithmetic gives
    now_x, now_y = ox, oy
    for cx, cy in ((9, 20), (54, 20), (30, 9), (30, 38), (-1, -1), (64, 48), (9, 38), (200, -150), (-3000, 4000)):
        getattr(h, fill)(state)
        x, y = now_x + (cx + 0.5) * cell, now_y + (cy + 0.5) * cell
        gx, gy = sr.cell_of(x, now_x, cell), sr.cell_of(y, now_y, cell)
        want = (K.follow_shift(gx, width, margin, step), K.follow_shift(gy, height, margin, step))
        assert want == sr.follow(x, y, now_x, now_y, cell, width, height, margin, step) and want != (0, 0)
        assert h.follow(x, y, margin, step) == want, (cx, cy)
        assert np.array_equal(read(), sr.shift(state, *want))
        now_x, now_y = sr.origin(now_x, want[0], cell), sr.origin(now_y, want[1], cell)
        info = h.info()
        assert _bits(info["origin_x"]) == _bits(now_x) and _bits(info["origin_y"]) == _bits(now_y)
        assert margin <= sr.cell_of(x, now_x, cell) < width - margin and margin <= sr.cell_of(y, now_y, cell) < height - margin
        assert h.follow(x, y, margin, step) == (0, 0)  # it is in the band now
    entry = K.lib().kicp_grid_follow if kind == "grid" else K.lib().kicp_elev_follow
    assert entry(None, 0.0, 0.0, margin, step, None, None) == K.KICP_ERR_ARG
    assert entry(h._h, now_x + 3.0, now_y + 2.0, margin, step, None, None) == K.KICP_OK  # the outputs are nullable


# ---- 7. rectangles ------------------------------------------------------------------------------------------------------------------
def test_rectangles_of_counters():
    width, height = 37, 29
    grid, counts = _grid(width, height), sc.counters(width, height)
    grid.set_counts(counts)
    table, weight = K.nav2_cost_table(0.1, 3, 0.1, 3.0), K.plan_weights()
    grid.potential(table, weight, [(5, 5)])
    rects = [(0, 0, 1, 1), (36, 28, 1, 1), (0, 0, 37, 29), (0, 0, 37, 1), (0, 28, 37, 1), (0, 0, 1, 29), (36, 0, 1, 29), (5, 7, 13, 11), (33, 3, 4, 26), (1, 1, 35, 27)]
    for x0, y0, w, h in rects:
        got = grid.counts_rect((x0, y0, w, h))
        assert got.dtype == np.uint16 and got.shape == (h, w, 2) and np.array_equal(got, counts[y0:y0 + h, x0:x0 + w]), (x0, y0, w, h)
    want = counts.copy()
    for k, (x0, y0, w, h) in enumerate(rects):
        patch = sc.counters(w, h, seed=10 + k)
        grid.set_counts_rect((x0, y0, w, h), patch)
        want[y0:y0 + h, x0:x0 + w] = patch
        assert np.array_equal(grid.counts(), want), (x0, y0, w, h)  # exactly the rectangle
    assert grid.has_plan()  # a rectangle written invalidates nothing
    for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (37, 0, 1, 1), (0, 29, 1, 1), (30, 0, 8, 1), (0, 20, 1, 10), (36, 28, 2, 1), (0, 0, 38, 29), (4294967295, 0, 2, 1)):
        assert _code(grid.counts_rect, bad) == K.KICP_ERR_ARG, bad
        assert _code(grid.set_counts_rect, bad, np.zeros((max(bad[3], 1), max(min(bad[2], 64), 1), 2), dtype=np.uint16)) == K.KICP_ERR_ARG, bad
    L, buf = K.lib(), np.zeros((4, 4, 2), dtype=np.uint16)
    p = buf.ctypes.data_as(C.POINTER(C.c_ushort))
    assert L.kicp_grid_counts_rect(grid._h, 0, 0, 4, 4, p, 15) == K.KICP_ERR_ARG and L.kicp_grid_counts_rect(grid._h, 0, 0, 4, 4, p, 17) == K.KICP_ERR_ARG
    assert L.kicp_grid_set_counts_rect(grid._h, 0, 0, 4, 4, p, 15) == K.KICP_ERR_ARG and L.kicp_grid_counts_rect(grid._h, 0, 0, 4, 4, None, 16) == K.KICP_ERR_ARG
    assert L.kicp_grid_counts_rect(None, 0, 0, 4, 4, p, 16) == K.KICP_ERR_ARG and L.kicp_grid_set_counts_rect(grid._h, 0, 0, 4, 4, None, 16) == K.KICP_ERR_ARG
    assert np.array_equal(grid.counts(), want)


@pytest.mark.parametrize("shift", [(4, -6), (-5, 0), (0, 3), (-36, 28)])
def test_paging_round_trip(shift):
    width, height = 37, 29
    dx, dy = shift
    grid, counts = _grid(width, height), sc.counters(width, height)
    grid.set_counts(counts)
    strips = [r for r in sr.leaving_strips(dx, dy, width, height) if r is not None]
    saved = [grid.counts_rect(r) for r in strips]
    assert sum(s.shape[0] * s.shape[1] for s in saved) == width * height - (width - abs(dx)) * (height - abs(dy))  # every cell that leaves, once
    grid.scroll(dx, dy)
    assert np.array_equal(grid.counts(), sr.shift(counts, dx, dy))
    grid.scroll(-dx, -dy)
    assert not np.array_equal(grid.counts(), counts)  # what left is gone ...
    for r, s in zip(strips, saved):
        grid.set_counts_rect(r, s)
    assert np.array_equal(grid.counts(), counts)  # ... until its owner puts it back


# ---- 8. no residue ------------------------------------------------------------------------------------------------------------------
def test_no_residue_after_a_scroll():
    """a detection and a frame before the scroll, then both again after it: the frame-local planes and the transient scratch are relative
    to the window and zero between calls, so nothing may remember a cell index of before"""
    s = tc.switch_scene()
    cfg, params = dict(s["cfg"]), s["params"]
    grid, counts = K.OccupancyGrid(*s["args"]), s["counts"].copy()
    grid.set_counts(counts)
    layer = K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], -1.0, 0.0625, cfg["max_ray"])
    for dx, dy in ((0, 0), (7, -4), (-13, 9), (1, 1)):
        grid.scroll(dx, dy), layer.scroll(dx, dy)
        counts = sr.shift(counts, dx, dy)
        cfg = dict(cfg, origin_x=sr.origin(cfg["origin_x"], dx, cfg["cell"]), origin_y=sr.origin(cfg["origin_y"], dy, cfg["cell"])) if (dx, dy) != (0, 0) else cfg
        want = tr.transients(cfg, counts, s["points"], s["pose"], s["sensor"], **params)
        rows, labels, stats = grid.transients(s["points"], s["pose"], s["sensor"], return_labels=True, return_stats=True, **params)
        assert np.array_equal(rows, want[0]) and np.array_equal(labels, want[1]) and stats == want[3] and np.array_equal(grid.transient_plane(), want[2]), (dx, dy)
        assert grid.integrate(s["points"], s["pose"], s["sensor"]) == gr.integrate(cfg, counts, s["points"], s["pose"], s["sensor"])
        assert np.array_equal(grid.counts(), counts), (dx, dy)
    # the layer under the same shifts: its columns after a frame equal a fresh layer's at the reported origin
    info = layer.info()
    assert _bits(info["origin_x"]) == _bits(cfg["origin_x"]) and _bits(info["origin_y"]) == _bits(cfg["origin_y"])
    fresh = K.ElevationLayer(info["cell"], info["origin_x"], info["origin_y"], info["width"], info["height"], info["z_origin"], info["slab"], info["max_ray"])
    assert layer.integrate(s["points"], s["pose"], s["sensor"]) == fresh.integrate(s["points"], s["pose"], s["sensor"])
    assert np.array_equal(layer.columns(), fresh.columns()) and layer.columns().any() and layer.last_window() == fresh.last_window()
