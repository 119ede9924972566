"""The grid's clearance and costmap on the GPU (kicp_grid_clearance, kicp_grid_costmap, kicp_grid_last_window: K.OccupancyGrid.clearance,
.costmap, .last_window) against the numpy restatement of include/kicp.h's text (tests/clearance_ref.py).  Everything is exact:
np.array_equal, no tolerance anywhere.  The counters are set with set_counts, so only the last test drives frames.  Column distances
of 253 .. 255 and scans to k = 254 (R = 253 and 254 on grids 520 cells long): tests/test_gpu_plan_regimes.py."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import clearance_ref as cr
import grid_cases as gc
import grid_ref as gr

pytestmark = pytest.mark.gpu

CASES = cr.host_cases()


def grid_of(counts, cell=0.05, max_ray=1.0):
    h, w = counts.shape[:2]
    grid = K.OccupancyGrid(cell, 0.0, 0.0, w, h, 0.0, 1.0, max_ray)
    grid.set_counts(counts)
    return grid


def check(grid, occ, radius, full, uio=False, rects=(None,), min_observations=1, inflates=(False, True)):
    """clearance and costmap of every rectangle equal the slice of the restatement's full-grid clearance `full` and of its costmap"""
    table = cr.mixed_table(radius)
    H, W = occ.shape
    for inflate in inflates:
        want_cost = cr.costmap(occ, table, 0.65, uio, inflate, clear=full)
        for rect in rects:
            x0, y0, w, h = rect or (0, 0, W, H)
            got = grid.clearance(radius, min_observations=min_observations, unknown_is_obstacle=uio, rect=rect)
            assert got.dtype == np.uint16 and got.shape == (h, w)
            bad = got != full[y0:y0 + h, x0:x0 + w]
            print("R %d rect %s uio %d: %d of %d clearances differ" % (radius, rect, uio, bad.sum(), bad.size))
            assert not bad.any(), np.argwhere(bad)[:5]
            got = grid.costmap(table, min_observations=min_observations, unknown_is_obstacle=uio, inflate_unknown=inflate, rect=rect)
            assert got.dtype == np.uint8 and got.shape == (h, w)
            bad = got != want_cost[y0:y0 + h, x0:x0 + w]
            assert not bad.any(), np.argwhere(bad)[:5]


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_cases(name):
    occ, radius = CASES[name]
    grid = grid_of(cr.counts_of(occ))
    assert np.array_equal(grid.occupancy(), occ)
    rects = cr.rectangles(occ.shape[1], occ.shape[0])
    for uio in (False, True):
        full = cr.clearance(occ, radius, unknown_is_obstacle=uio)
        check(grid, occ, radius, full, uio, rects)
        assert np.array_equal(K.clearance_from_occupancy(occ, radius, unknown_is_obstacle=uio), full)
    if name == "pinned_8x6":
        _, _, want, want_uio = cr.pinned_8x6()
        assert np.array_equal(grid.clearance(3), want) and np.array_equal(grid.clearance(3, unknown_is_obstacle=True), want_uio)


@pytest.mark.parametrize("width,height", [(300, 5), (5, 300)])
def test_a_row_across_segments_and_a_column_across_strips(width, height):
    """300 cells cross the 256-cell segment of a row / the 32-row strips of a column; the few sources sit next to those borders"""
    occ = np.zeros((height, width), dtype=np.int8)
    occ[1, 2] = -1
    long_axis = [0, 30, 31, 32, 63, 64, 100, 254, 255, 256, 257, 299]
    for k, at in enumerate(long_axis):
        if k % 2 == 0:
            occ[(k % height, at) if width > height else (at, k % width)] = 100
    grid = grid_of(cr.counts_of(occ))
    for radius in (3, 40):
        full = cr.clearance(occ, radius)
        assert (full == radius * radius + 1).any() or radius == 40
        rects = [None, (255, 0, 3, 5), (250, 2, 50, 3), (0, 4, 300, 1)] if width > height else [None, (0, 255, 5, 3), (2, 250, 3, 50), (4, 0, 1, 300), (0, 31, 5, 2)]
        check(grid, occ, radius, full, False, rects)
        full_uio = cr.clearance(occ, radius, unknown_is_obstacle=True)
        check(grid, occ, radius, full_uio, True, rects[:2], inflates=(True,))


@pytest.fixture(scope="module")
def big():
    """520 x 260 cells: about 1 % sources (no early exit: most scans run far) and 40 % (every scan stops at once), R = 20 - the
    restatement's clearance computed once"""
    out = {}
    for name, fraction, unknown in (("sparse", 0.01, 0.05), ("dense", 0.4, 0.2)):
        occ = cr.random_occupancy(520, 260, fraction, 17, unknown)
        out[name] = (occ, cr.clearance_by_offsets(occ, 20))
    return out


@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_520x260(big, name):
    occ, full = big[name]
    grid = grid_of(cr.counts_of(occ))
    rects = [None, (255, 100, 3, 7), (519, 259, 1, 1), (500, 0, 20, 260), (0, 255, 520, 5), (100, 31, 300, 34)]  # the grid's last column and row among them
    check(grid, occ, 20, full, False, rects)
    assert np.array_equal(K.clearance_from_occupancy(occ, 20), full)
    sources = (occ > 65).mean()
    assert (0.005 < sources < 0.02) if name == "sparse" else (0.35 < sources < 0.45)
    assert (full > 16).mean() > 0.3 if name == "sparse" else (full <= 4).mean() > 0.99  # scans that run far / that stop at once


@pytest.mark.parametrize("width", [255, 256, 257])
def test_widths_around_a_segment(width):
    occ = cr.random_occupancy(width, 7, 0.02, width)
    occ[3, width - 1] = occ[0, 0] = 100
    for radius in (5, 200):
        full = cr.clearance_by_offsets(occ, radius)
        check(grid_of(cr.counts_of(occ)), occ, radius, full, False, [None, (width - 1, 6, 1, 1), (width - 4, 0, 4, 7), (0, 6, width, 1)], inflates=(True,))


def test_counters_at_65535_and_min_observations():
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 4, (40, 70, 2)).astype(np.uint16)
    pairs = [(65535, 65535), (65535, 0), (0, 65535), (65535, 21845), (43690, 21845), (65535, 35288), (65535, 35289)]  # 50, 100, 0, 75, 67, 65, 65
    for k, pair in enumerate(pairs):
        counts[5 + 4 * k, 10 + 7 * k] = pair
        counts[39 - k, 69] = pair
    for min_observations in (1, 3, 6):
        occ = gr.occupancy(counts, min_observations)
        grid = grid_of(counts)
        assert np.array_equal(grid.occupancy(min_observations), occ)
        for uio in (False, True):
            full = cr.clearance_by_offsets(occ, 6, unknown_is_obstacle=uio)
            check(grid, occ, 6, full, uio, [None, (60, 30, 10, 10)], min_observations)
    assert gr.occupancy(np.array(pairs, dtype=np.uint16)).tolist() == [50, 100, 0, 75, 67, 65, 65]
    occ1 = gr.occupancy(counts, 1)
    assert grid.clearance(6)[5, 10] > 0 and grid.clearance(6)[9, 17] == 0 and grid.clearance(6)[25, 45] > 0  # 50 and 65 are clear, 100 is a source
    assert (occ1 == -1).any() and (gr.occupancy(counts, 6) == -1).mean() > 0.9


def test_thresholds_on_the_device():
    occ = np.tile(np.array([64, 65, 66, 100, 0, -1, 1, 50], dtype=np.int8), (3, 1))
    grid = grid_of(cr.counts_of(occ))
    for thresh in (0.0, 0.5, 0.65, 0.655, 1.0):
        got = grid.clearance(2, occupied_thresh=thresh)
        assert np.array_equal(got, cr.clearance(occ, 2, thresh)), thresh
        assert np.array_equal(got, K.clearance_from_occupancy(occ, 2, occupied_thresh=thresh))


def test_costmap_follows_the_last_window_of_a_drive():
    """After each frame: the costmap of last_window() grown by R and clipped, pasted into the previous full costmap, is the new full
    costmap; last_window() is the window the restatement derives from the sensor's cell"""
    cfg, frames = gc.random_drive()
    W, H, radius = cfg["width"], cfg["height"], 10  # 1 m of 0.1 m cells
    grid = K.OccupancyGrid(cfg["cell"], cfg["origin_x"], cfg["origin_y"], W, H, cfg["z_min"], cfg["z_max"], cfg["max_ray"])
    table = K.nav2_cost_table(cfg["cell"], radius, 0.35, 3.0)
    kw = dict(min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=True)
    assert grid.last_window() == (0, 0, 0, 0)  # before any frame
    kept = grid.costmap(table, **kw)
    assert (kept == 255).all()
    want_counts = np.zeros((H, W, 2), dtype=np.uint16)
    for pts, pose, sensor in frames:
        grid.integrate(pts, pose, sensor)
        gr.integrate(cfg, want_counts, pts, pose, sensor)
        window = grid.last_window()
        assert window == cr.window(cfg, pose, sensor) and window[2] > 0 and window[3] > 0
        x0, y0, w, h = cr.grown(window, radius, W, H)
        kept[y0:y0 + h, x0:x0 + w] = grid.costmap(table, rect=(x0, y0, w, h), **kw)
        full = grid.costmap(table, **kw)
        changed = int((kept != full).sum())
        print("window %s grown %s: %d cells differ from the full costmap" % (window, (x0, y0, w, h), changed))
        assert changed == 0
        occ = gr.occupancy(want_counts)
        assert np.array_equal(full, cr.costmap(occ, table, inflate_unknown=True, clear=cr.clearance_by_offsets(occ, radius)))
    assert any(cr.window(cfg, pose, sensor)[2] < 2 * cfg["reach"] + 1 for _, pose, sensor in frames)  # a window was clipped by the border
    assert (full == 254).any() and (full == 253).any() and ((full > 0) & (full < 253)).any() and (full == 0).any() and (full == 255).any()
    far_pose = np.array([0.0, 0.0, 0.0, 1.0, 500.0, 0.0, 0.0])
    grid.integrate(np.zeros((0, 3)), far_pose, frames[0][2])  # a window that lies outside the grid, and one that is nowhere
    assert grid.last_window() == (0, 0, 0, 0) == cr.window(cfg, far_pose, frames[0][2])
    grid.integrate(np.zeros((0, 3)), frames[0][1], frames[0][2])  # an empty frame still has its window
    assert grid.last_window() == cr.window(cfg, frames[0][1], frames[0][2])
    grid.integrate(np.zeros((0, 3)), np.array([0.0, 0.0, 0.0, 1.0, np.nan, 0.0, 0.0]), frames[0][2])
    assert grid.last_window() == (0, 0, 0, 0)
    assert np.array_equal(grid.costmap(table, **kw), full)  # none of them changed a counter
    grid.integrate(*frames[0])
    grid.clear()
    assert grid.last_window() == (0, 0, 0, 0)


def test_argument_errors_on_the_device():
    occ = np.zeros((4, 6), dtype=np.int8)
    grid = grid_of(cr.counts_of(occ))
    table = cr.mixed_table(2)

    def code(fn, **kw):
        with pytest.raises(K.KicpError) as e:
            fn(**kw)
        return e.value.code, str(e.value)

    def clearance(radius_cells=2, **kw):
        return grid.clearance(radius_cells, **kw)

    def costmap(table=table, **kw):
        return grid.costmap(table, **kw)

    bad = [dict(min_observations=0), dict(occupied_thresh=-0.01), dict(occupied_thresh=1.01), dict(occupied_thresh=float("nan")), dict(rect=(0, 0, 7, 4)),
           dict(rect=(0, 0, 6, 5)), dict(rect=(6, 0, 1, 1)), dict(rect=(0, 4, 1, 1)), dict(rect=(2, 2, 0, 1)), dict(rect=(2, 2, 1, 0)), dict(rect=(5, 3, 2, 1))]
    for kw in bad + [dict(radius_cells=0), dict(radius_cells=-1)]:
        assert code(clearance, **kw)[0] == K.KICP_ERR_ARG, kw
    for kw in bad + [dict(table=table[:-1])]:
        assert code(costmap, **kw)[0] == K.KICP_ERR_ARG, kw
    c, msg = code(clearance, radius_cells=255)
    assert c == K.KICP_ERR_CAPACITY and "254" in msg
    c, msg = code(costmap, table=np.zeros(255 * 255 + 2, dtype=np.uint8))
    assert c == K.KICP_ERR_CAPACITY and "254" in msg
    lib = K.lib()
    cfg = K.GridClearanceConfig(1, 0.65, 0, 2)
    u8, u16, ui = C.POINTER(C.c_ubyte), C.POINTER(C.c_ushort), C.c_uint
    o16, o8 = np.zeros(24, dtype=np.uint16), np.zeros(24, dtype=np.uint8)
    pt, p16, p8 = table.ctypes.data_as(u8), o16.ctypes.data_as(u16), o8.ctypes.data_as(u8)
    assert lib.kicp_grid_clearance(grid._h, C.byref(cfg), 0, 0, 6, 4, p16, 24) == K.KICP_OK
    assert lib.kicp_grid_clearance(grid._h, None, 0, 0, 6, 4, p16, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance(grid._h, C.byref(cfg), 0, 0, 6, 4, None, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance(grid._h, C.byref(cfg), 0, 0, 6, 4, p16, 23) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance(grid._h, C.byref(cfg), 0xFFFFFFFF, 0, 2, 1, p16, 2) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap(grid._h, C.byref(cfg), pt, 6, 0, 0, 0, 6, 4, p8, 24) == K.KICP_OK
    assert lib.kicp_grid_costmap(grid._h, None, pt, 6, 0, 0, 0, 6, 4, p8, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap(grid._h, C.byref(cfg), None, 6, 0, 0, 0, 6, 4, p8, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap(grid._h, C.byref(cfg), pt, 6, 0, 0, 0, 6, 4, None, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap(grid._h, C.byref(cfg), pt, 7, 0, 0, 0, 6, 4, p8, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap(grid._h, C.byref(cfg), pt, 6, 0, 0, 0, 6, 4, p8, 25) == K.KICP_ERR_ARG
    v = [ui() for _ in range(4)]
    assert lib.kicp_grid_last_window(grid._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), None) == K.KICP_ERR_ARG
    assert lib.kicp_grid_last_window(grid._h, *[C.byref(x) for x in v]) == K.KICP_OK
    assert np.array_equal(grid.clearance(2), np.full((4, 6), 5, dtype=np.uint16))  # the handle is unharmed
