"""The slope limit of the height columns on the GPU (kicp_elev_traversability_slope, kicp_elev_to_grid_slope: K.ElevationLayer) against
the numpy restatement of include/kicp.h's semantics (tests/elev_slope_ref.py) on the cases of tests/elev_slope_cases.py, which
tests/test_elev_slope_cases.py proves to enter their regimes.  Everything is exact: every class, ground byte, determinant and count
must be equal - no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import clearance_ref as cr
import elev_slope_cases as sc
import elev_slope_ref as sr

pytestmark = pytest.mark.gpu


def layer_for(columns, cell=0.25, slab=0.125):
    height, width = columns.shape
    layer = K.ElevationLayer(cell, 0.0, 0.0, width, height, 0.0, slab, 2.0)
    layer.set_columns(columns)
    return layer


def check_case(case, layer=None):
    name, columns, (S, H), slope, rects = case
    layer = layer or layer_for(columns)
    for rect in rects:
        got, ground, fit, counts = layer.traversability_slope(S, H, slope, rect=rect, return_ground=True, return_fit=True, return_counts=True)
        sc.check_result(case, rect, got, ground, fit, counts)
    # each optional output alone, and none
    rect = rects[-1]
    got, ground = layer.traversability_slope(S, H, slope, rect=rect, return_ground=True)
    sc.check_result(case, rect, got, got_ground=ground)
    got, fit = layer.traversability_slope(S, H, slope, rect=rect, return_fit=True)
    sc.check_result(case, rect, got, got_fit=fit)
    got, counts = layer.traversability_slope(S, H, slope, rect=rect, return_counts=True)
    sc.check_result(case, rect, got, got_counts=counts)
    sc.check_result(case, rect, layer.traversability_slope(S, H, slope, rect=rect))
    return layer


def test_hand_made_cases():
    for case in sc.small_cases():
        check_case(case)


@pytest.mark.parametrize("kind", ["dense", "sparse", "zero"])
def test_random_columns(kind):
    layer = None
    for case in sc.random_cases():
        if ("random_%s_" % kind) in case[0]:
            layer = check_case(case, layer)
            # wherever a cell is not SLOPE only, its value is kicp_elev_traversability's
            want = sc.expected(case)
            only = want.slope & ~want.body & ~want.step
            got, plain = layer.traversability_slope(*case[2], case[3]), layer.traversability(*case[2])
            assert np.array_equal(got[~only], plain[~only]) and (got[only] == 100).all() and (plain[only] == 0).all()


@pytest.mark.parametrize("case", sc.radius_cases(), ids=lambda case: case[0])
def test_every_radius(case):
    """the instantiation of each L = 1 .. 8, read out and into a grid"""
    name, columns, (S, H), slope, rects = case
    assert (sc.expected(case).fit[:, :, 0] > 0).any(), name  # some cell has a fit
    layer = layer_for(columns)
    for rect in rects:
        got, ground, fit, counts = layer.traversability_slope(S, H, slope, rect=rect, return_ground=True, return_fit=True, return_counts=True)
        sc.check_result(case, rect, got, ground, fit, counts)
    grid = K.OccupancyGrid(0.25, 0.0, 0.0, columns.shape[1], columns.shape[0], -1.0, 1.0, 2.0)
    layer.to_grid_slope(grid, S, H, slope)
    assert np.array_equal(grid.occupancy(1), sc.expected(case).classes), name


def test_to_grid_slope():
    case = [c for c in sc.random_cases() if c[0] == "random_sparse_1"][0]
    name, columns, (S, H), slope, _ = case
    layer = layer_for(columns)
    want = sc.expected(case)
    assert (want.slope & ~want.body & ~want.step).any() and (want.classes == 0).any() and (want.classes == -1).any()
    height, width = columns.shape
    grid = K.OccupancyGrid(0.25, 0.0, 0.0, width, height, -1.0, 1.0, 2.0)
    grid.set_counts(np.full((height, width, 2), 7, dtype=np.uint16))  # every counter is replaced
    layer.to_grid_slope(grid, S, H, slope)
    counts = grid.counts()
    assert np.array_equal(counts[:, :, 0], (want.classes == 100).astype(np.uint16)) and np.array_equal(counts[:, :, 1], (want.classes == 0).astype(np.uint16))
    assert np.array_equal(grid.occupancy(1), want.classes)
    for side in (17, 33):  # layers that are no multiple of the tile, L = 8
        square = [c for c in sc.small_cases() if c[0] == "square%d_L8" % side][0]
        small, other = layer_for(square[1]), K.OccupancyGrid(0.25, 0.0, 0.0, side, side, -1.0, 1.0, 2.0)
        small.to_grid_slope(other, *square[2], square[3])
        assert np.array_equal(other.occupancy(1), sc.expected(square).classes)
    # kicp_elev_to_grid's checks
    for bad in (K.OccupancyGrid(0.125, 0.0, 0.0, width, height, -1.0, 1.0, 2.0), K.OccupancyGrid(0.25, 0.25, 0.0, width, height, -1.0, 1.0, 2.0),
                K.OccupancyGrid(0.25, 0.0, 0.0, width, height + 1, -1.0, 1.0, 2.0)):
        with pytest.raises(K.KicpError) as e:
            layer.to_grid_slope(bad, S, H, slope)
        assert e.value.code == K.KICP_ERR_ARG
    for args in ((8, 8, slope), (S, H, (0, 6, 12, 1, 1)), (S, H, (4, 64, 12, 1, 1)), (S, H, (4, 6, 12, 1, 0))):
        with pytest.raises(K.KicpError) as e:
            layer.to_grid_slope(grid, *args)
        assert e.value.code == K.KICP_ERR_ARG
    lib, cfg, scfg = K.lib(), K.ElevationTraversabilityConfig(S, H), K.ElevationSlopeConfig(*slope)
    assert lib.kicp_elev_to_grid_slope(None, C.byref(cfg), C.byref(scfg), grid._h) == K.KICP_ERR_ARG
    assert lib.kicp_elev_to_grid_slope(layer._h, None, C.byref(scfg), grid._h) == K.KICP_ERR_ARG
    assert lib.kicp_elev_to_grid_slope(layer._h, C.byref(cfg), None, grid._h) == K.KICP_ERR_ARG
    assert lib.kicp_elev_to_grid_slope(layer._h, C.byref(cfg), C.byref(scfg), None) == K.KICP_ERR_ARG
    assert np.array_equal(grid.occupancy(1), want.classes)  # the refused calls left the grid alone


def test_the_drive_integrated_on_the_device():
    """300 x 300 cells: 361 workgroups, over a thousand waves add to the 64 shards of the counts"""
    cfg, frames, columns = sc.drive_columns()
    (S, H), slope = sc.DRIVE_PARAMS, sc.DRIVE_SLOPE
    layer = K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"])
    for pts, pose, sensor in frames:
        layer.integrate_device(K.DeviceFrame(pts), pose, sensor)
    assert np.array_equal(layer.columns(), columns)
    assert layer.slope_limit(np.tan(np.deg2rad(20.0))) == slope[3:]
    want = sr.classify(columns, S, H, slope)
    before, ground, fit, counts = layer.traversability_slope(S, H, slope, return_ground=True, return_fit=True, return_counts=True)
    assert np.array_equal(before, want.classes) and np.array_equal(ground, want.ground) and np.array_equal(fit, want.fit)
    assert counts == sr.counts(want) and sum(counts) == 90000 and counts[4] > 50
    only = want.slope & ~want.body & ~want.step
    plain = layer.traversability(S, H)
    assert np.array_equal(before[~only], plain[~only]) and (before[only] == 100).all() and (plain[only] == 0).all()
    # one more frame: nothing changes outside the last window grown by max(1, L)
    pts, pose, sensor = frames[0]
    layer.integrate(pts + np.array([0.0, 0.0, 0.4]), pose, sensor)
    after, after_fit = layer.traversability_slope(S, H, slope, return_fit=True)
    got, got_fit = K.traversability_slope_from_columns(layer.columns(), S, H, slope, return_fit=True)
    assert not np.array_equal(after, before) and np.array_equal(after, got) and np.array_equal(after_fit, got_fit)
    x0, y0, w, h = cr.grown(layer.last_window(), max(1, slope[0]), cfg["width"], cfg["height"])
    assert w * h < 90000
    pasted, pasted_fit = before.copy(), fit.copy()
    pasted[y0:y0 + h, x0:x0 + w], pasted_fit[y0:y0 + h, x0:x0 + w] = layer.traversability_slope(S, H, slope, rect=(x0, y0, w, h), return_fit=True)
    assert np.array_equal(pasted, after) and np.array_equal(pasted_fit, after_fit)


def test_argument_errors():
    layer = K.ElevationLayer(0.25, 0.0, 0.0, 16, 16, 0.0, 0.125, 2.0)
    good = (4, 6, 12, 596, 1024)
    for slope in ((0, 6, 12, 1, 1), (9, 6, 12, 1, 1), (4, 64, 12, 1, 1), (4, 6, 2, 1, 1), (4, 6, 290, 1, 1), (4, 6, 12, 65536, 1), (4, 6, 12, 1, 0), (4, 6, 12, 1, 65536)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability_slope(1, 4, slope)
        assert e.value.code == K.KICP_ERR_ARG, slope
    for slope in ((1, 0, 3, 0, 1), (8, 63, 289, 65535, 65535)):
        assert (layer.traversability_slope(1, 4, slope) == -1).all()
    for S, H in ((63, 64), (0, 0), (4, 2), (0, 65)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability_slope(S, H, good)
        assert e.value.code == K.KICP_ERR_ARG, (S, H)
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (16, 0, 1, 1), (0, 16, 1, 1), (9, 0, 8, 1), (0, 9, 1, 8)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability_slope(1, 4, good, rect=rect)
        assert e.value.code == K.KICP_ERR_ARG, rect
    lib, cfg, scfg = K.lib(), K.ElevationTraversabilityConfig(1, 4), K.ElevationSlopeConfig(*good)
    out = np.zeros(256, dtype=np.int8).ctypes.data_as(C.POINTER(C.c_byte))
    call = lib.kicp_elev_traversability_slope
    assert call(None, C.byref(cfg), C.byref(scfg), 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, None, C.byref(scfg), 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), None, 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), C.byref(scfg), 0, 0, 16, 16, None, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), C.byref(scfg), 0, 0, 16, 16, out, None, None, None, 255) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), C.byref(scfg), 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_OK
    assert (layer.traversability_slope(1, 4, good) == -1).all()  # the handle is unharmed
