"""The class ROUGH of the height columns on the GPU (kicp_elev_traversability_rough, kicp_elev_to_grid_rough: K.ElevationLayer) against
the numpy restatement of include/kicp.h's semantics (tests/elev_rough_ref.py) on the cases of tests/elev_rough_cases.py, which
tests/test_elev_rough_cases.py proves to enter their regimes.  Everything is exact: every class, ground byte, determinant, residual
and count must be equal - no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import clearance_ref as cr
import elev_rough_cases as rc
import elev_rough_ref as rr
import elev_slope_cases as sc

pytestmark = pytest.mark.gpu


def layer_for(columns, cell=0.25, slab=0.125):
    height, width = columns.shape
    layer = K.ElevationLayer(cell, 0.0, 0.0, width, height, 0.0, slab, 2.0)
    layer.set_columns(columns)
    return layer


def check_case(case, layer=None):
    name, columns, (S, H), slope, rough, rects = case
    layer = layer or layer_for(columns)
    for rect in rects:
        got, ground, fit, counts = layer.traversability_rough(S, H, slope, rough, rect=rect, return_ground=True, return_fit=True, return_counts=True)
        rc.check_result(case, rect, got, ground, fit, counts)
    # each optional output alone, and none
    rect = rects[-1]
    got, ground = layer.traversability_rough(S, H, slope, rough, rect=rect, return_ground=True)
    rc.check_result(case, rect, got, got_ground=ground)
    got, fit = layer.traversability_rough(S, H, slope, rough, rect=rect, return_fit=True)
    rc.check_result(case, rect, got, got_fit=fit)
    got, counts = layer.traversability_rough(S, H, slope, rough, rect=rect, return_counts=True)
    rc.check_result(case, rect, got, got_counts=counts)
    rc.check_result(case, rect, layer.traversability_rough(S, H, slope, rough, rect=rect))
    return layer


def test_hand_made_cases():
    for case in rc.small_cases():
        check_case(case)


@pytest.mark.parametrize("kind", ["dense", "sparse", "zero"])
def test_random_columns(kind):
    layer = None
    for case in rc.random_cases():
        if ("random_%s_" % kind) in case[0]:
            layer = check_case(case, layer)
            # wherever a cell is not ROUGH only, its value is kicp_elev_traversability_slope's; the fit begins with its triple
            want = rc.expected(case)
            only = want.rough & ~want.body & ~want.step & ~want.slope
            (got, fit), (plain, triple) = layer.traversability_rough(*case[2], case[3], case[4], return_fit=True), layer.traversability_slope(*case[2], case[3], return_fit=True)
            assert np.array_equal(got[~only], plain[~only]) and (got[only] == 100).all() and (plain[only] == 0).all()
            assert np.array_equal(fit[:, :, :3], triple)


@pytest.mark.parametrize("case", rc.radius_cases(), ids=lambda case: case[0])
def test_every_radius(case):
    """the instantiation of each L = 1 .. 8, read out and into a grid"""
    name, columns, (S, H), slope, rough, rects = case
    assert (rc.expected(case).fit[:, :, 0] > 0).any(), name  # some cell has a fit
    layer = layer_for(columns)
    for rect in rects:
        got, ground, fit, counts = layer.traversability_rough(S, H, slope, rough, rect=rect, return_ground=True, return_fit=True, return_counts=True)
        rc.check_result(case, rect, got, ground, fit, counts)
    grid = K.OccupancyGrid(0.25, 0.0, 0.0, columns.shape[1], columns.shape[0], -1.0, 1.0, 2.0)
    layer.to_grid_rough(grid, S, H, slope, rough)
    assert np.array_equal(grid.occupancy(1), rc.expected(case).classes), name


def test_all_six_counts():
    case = [c for c in rc.random_cases() if c[0] == "random_sparse_1"][0]
    got, counts = layer_for(case[1]).traversability_rough(*case[2], case[3], case[4], return_counts=True)
    assert counts == rr.counts(rc.expected(case)) and all(w > 0 for w in counts) and sum(counts) == case[1].size


def test_to_grid_rough():
    case = [c for c in rc.random_cases() if c[0] == "random_sparse_1"][0]
    name, columns, (S, H), slope, rough, _ = case
    layer = layer_for(columns)
    want = rc.expected(case)
    assert (want.rough & ~want.body & ~want.step & ~want.slope).any() and (want.classes == 0).any() and (want.classes == -1).any()
    height, width = columns.shape
    grid = K.OccupancyGrid(0.25, 0.0, 0.0, width, height, -1.0, 1.0, 2.0)
    grid.set_counts(np.full((height, width, 2), 7, dtype=np.uint16))  # every counter is replaced
    layer.to_grid_rough(grid, S, H, slope, rough)
    counts = grid.counts()
    assert np.array_equal(counts[:, :, 0], (want.classes == 100).astype(np.uint16)) and np.array_equal(counts[:, :, 1], (want.classes == 0).astype(np.uint16))
    assert np.array_equal(grid.occupancy(1), want.classes)
    for name in ("square17_L8", "square33_L8", "square33_L1", "borders", "checkerboard"):  # layers that are no multiple of the tile; the wide product
        small_case = [c for c in rc.small_cases() if c[0] == name][0]
        side_y, side_x = small_case[1].shape
        small, other = layer_for(small_case[1]), K.OccupancyGrid(0.25, 0.0, 0.0, side_x, side_y, -1.0, 1.0, 2.0)
        small.to_grid_rough(other, *small_case[2], small_case[3], small_case[4])
        assert np.array_equal(other.occupancy(1), rc.expected(small_case).classes), name
    # kicp_elev_to_grid's checks
    for bad in (K.OccupancyGrid(0.125, 0.0, 0.0, width, height, -1.0, 1.0, 2.0), K.OccupancyGrid(0.25, 0.25, 0.0, width, height, -1.0, 1.0, 2.0),
                K.OccupancyGrid(0.25, 0.0, 0.0, width, height + 1, -1.0, 1.0, 2.0)):
        with pytest.raises(K.KicpError) as e:
            layer.to_grid_rough(bad, S, H, slope, rough)
        assert e.value.code == K.KICP_ERR_ARG
    for args in ((8, 8, slope, rough), (S, H, (0, 6, 12, 1, 1), rough), (S, H, (4, 64, 12, 1, 1), rough), (S, H, slope, (65536, 1)), (S, H, slope, (1, 0)), (S, H, slope, (1, 65536))):
        with pytest.raises(K.KicpError) as e:
            layer.to_grid_rough(grid, *args)
        assert e.value.code == K.KICP_ERR_ARG
    lib, cfg, scfg, rcfg = K.lib(), K.ElevationTraversabilityConfig(S, H), K.ElevationSlopeConfig(*slope), K.ElevationRoughConfig(*rough)
    assert lib.kicp_elev_to_grid_rough(None, C.byref(cfg), C.byref(scfg), C.byref(rcfg), grid._h) == K.KICP_ERR_ARG
    assert lib.kicp_elev_to_grid_rough(layer._h, None, C.byref(scfg), C.byref(rcfg), grid._h) == K.KICP_ERR_ARG
    assert lib.kicp_elev_to_grid_rough(layer._h, C.byref(cfg), None, C.byref(rcfg), grid._h) == K.KICP_ERR_ARG
    assert lib.kicp_elev_to_grid_rough(layer._h, C.byref(cfg), C.byref(scfg), None, grid._h) == K.KICP_ERR_ARG
    assert lib.kicp_elev_to_grid_rough(layer._h, C.byref(cfg), C.byref(scfg), C.byref(rcfg), None) == K.KICP_ERR_ARG
    assert np.array_equal(grid.occupancy(1), want.classes)  # the refused calls left the grid alone


def test_the_drive_integrated_on_the_device():
    """300 x 300 cells: 361 workgroups, over a thousand waves add to the 64 shards of the counts"""
    cfg, frames, columns = sc.drive_columns()
    (S, H), slope, rough = sc.DRIVE_PARAMS, sc.DRIVE_SLOPE, rc.DRIVE_ROUGH
    layer = K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"])
    for pts, pose, sensor in frames:
        layer.integrate_device(K.DeviceFrame(pts), pose, sensor)
    assert np.array_equal(layer.columns(), columns)
    assert layer.rough_limit(cfg["slab"] * np.sqrt(0.5)) == rough
    want = rr.classify(columns, S, H, slope, rough)
    before, ground, fit, counts = layer.traversability_rough(S, H, slope, rough, return_ground=True, return_fit=True, return_counts=True)
    assert np.array_equal(before, want.classes) and np.array_equal(ground, want.ground) and np.array_equal(fit, want.fit)
    assert counts == rr.counts(want) and sum(counts) == 90000 and all(w > 0 for w in counts) and counts[5] > 50
    only = want.rough & ~want.body & ~want.step & ~want.slope
    plain, triple = layer.traversability_slope(S, H, slope, return_fit=True)
    assert np.array_equal(before[~only], plain[~only]) and (before[only] == 100).all() and (plain[only] == 0).all() and np.array_equal(fit[:, :, :3], triple)
    grid = K.OccupancyGrid(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], -1.0, 1.0, cfg["max_ray"])
    layer.to_grid_rough(grid, S, H, slope, rough)
    assert np.array_equal(grid.occupancy(1), want.classes)
    # one more frame: nothing changes outside the last window grown by max(1, L)
    pts, pose, sensor = frames[0]
    layer.integrate(pts + np.array([0.0, 0.0, 0.4]), pose, sensor)
    after, after_fit = layer.traversability_rough(S, H, slope, rough, return_fit=True)
    got, got_fit = K.traversability_rough_from_columns(layer.columns(), S, H, slope, rough, return_fit=True)
    assert not np.array_equal(after, before) and np.array_equal(after, got) and np.array_equal(after_fit, got_fit)
    x0, y0, w, h = cr.grown(layer.last_window(), max(1, slope[0]), cfg["width"], cfg["height"])
    assert w * h < 90000
    pasted, pasted_fit = before.copy(), fit.copy()
    pasted[y0:y0 + h, x0:x0 + w], pasted_fit[y0:y0 + h, x0:x0 + w] = layer.traversability_rough(S, H, slope, rough, rect=(x0, y0, w, h), return_fit=True)
    assert np.array_equal(pasted, after) and np.array_equal(pasted_fit, after_fit)


def test_argument_errors():
    layer = K.ElevationLayer(0.25, 0.0, 0.0, 16, 16, 0.0, 0.125, 2.0)
    good, fine = (4, 6, 12, 596, 1024), (1, 2)
    for slope in ((0, 6, 12, 1, 1), (9, 6, 12, 1, 1), (4, 64, 12, 1, 1), (4, 6, 2, 1, 1), (4, 6, 290, 1, 1), (4, 6, 12, 65536, 1), (4, 6, 12, 1, 0), (4, 6, 12, 1, 65536)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability_rough(1, 4, slope, fine)
        assert e.value.code == K.KICP_ERR_ARG, slope
    for rough in ((65536, 1), (1, 0), (0, 0), (1, 65536), (2 ** 32 - 1, 1)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability_rough(1, 4, good, rough)
        assert e.value.code == K.KICP_ERR_ARG, rough
    for slope, rough in (((1, 0, 3, 0, 1), (0, 1)), ((8, 63, 289, 65535, 65535), (65535, 65535))):
        assert (layer.traversability_rough(1, 4, slope, rough) == -1).all()
    for S, H in ((63, 64), (0, 0), (4, 2), (0, 65)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability_rough(S, H, good, fine)
        assert e.value.code == K.KICP_ERR_ARG, (S, H)
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (16, 0, 1, 1), (0, 16, 1, 1), (9, 0, 8, 1), (0, 9, 1, 8)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability_rough(1, 4, good, fine, rect=rect)
        assert e.value.code == K.KICP_ERR_ARG, rect
    lib, cfg, scfg, rcfg = K.lib(), K.ElevationTraversabilityConfig(1, 4), K.ElevationSlopeConfig(*good), K.ElevationRoughConfig(*fine)
    out = np.zeros(256, dtype=np.int8).ctypes.data_as(C.POINTER(C.c_byte))
    call = lib.kicp_elev_traversability_rough
    assert call(None, C.byref(cfg), C.byref(scfg), C.byref(rcfg), 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, None, C.byref(scfg), C.byref(rcfg), 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), None, C.byref(rcfg), 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), C.byref(scfg), None, 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), C.byref(scfg), C.byref(rcfg), 0, 0, 16, 16, None, None, None, None, 256) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), C.byref(scfg), C.byref(rcfg), 0, 0, 16, 16, out, None, None, None, 255) == K.KICP_ERR_ARG
    assert call(layer._h, C.byref(cfg), C.byref(scfg), C.byref(rcfg), 0, 0, 16, 16, out, None, None, None, 256) == K.KICP_OK
    assert (layer.traversability_rough(1, 4, good, fine) == -1).all()  # the handle is unharmed
