"""The fill of a grid's unknown cells from another grid on the GPU (kicp_grid_fill_unknown: K.OccupancyGrid.fill_unknown) against the
host entry and the numpy restatement of include/kicp.h's semantics (tests/elev_rough_ref.py's fill) on the cases of
tests/grid_fill_cases.py, which tests/test_grid_fill_host.py proves to enter their regimes; and end to end: a drive into a mapping
grid and a layer, the layer's classes with ROUGH into a planner's grid, the fill from the mapping grid, the frontiers of the result.
Everything is exact - no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import elev_rough_cases as rc
import elev_rough_ref as rr
import elev_slope_cases as sc
import frontier_ref as fr
import grid_fill_cases as fc
import grid_ref as gr

pytestmark = pytest.mark.gpu


def grids_for(dst, src):
    cells = dst.size // 2
    width, height = (dst.shape[1], dst.shape[0]) if dst.ndim == 3 and dst.shape[0] == dst.shape[1] == 300 else (cells, 1)
    a, b = (K.OccupancyGrid(0.25, 0.0, 0.0, width, height, -1.0, 1.0, 2.0) for _ in range(2))
    a.set_counts(dst)
    b.set_counts(src)
    return a, b, (height, width, 2)


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c[0])
def test_against_the_host_entry_and_the_restatement(case):
    name, dst, src, cfg = case
    want, words = rr.fill(dst, src, *cfg)
    a, b, shape = grids_for(dst, src)
    counts = a.fill_unknown(b, *cfg, return_counts=True)
    got = a.counts()
    host, host_words = K.fill_unknown_counts(dst, src, *cfg, return_counts=True)
    assert np.array_equal(got, want.reshape(shape)) and np.array_equal(got, host.reshape(shape)) and counts == words == host_words
    assert sum(counts[:5]) == dst.size // 2 and np.array_equal(b.counts(), src.reshape(shape))  # the source is not changed
    kept = (dst[..., 0] > 0) | (dst[..., 1] > 0)
    assert np.array_equal(got.reshape(dst.shape)[kept], dst[kept])  # kept words keep their bits
    # a second call leaves the counters equal and counts the filled cells as kept; without the counts nothing else changes
    second = a.fill_unknown(b, *cfg, return_counts=True)
    assert np.array_equal(a.counts(), got) and second[2] == second[3] == 0 and second[0] == counts[0] + counts[3] and second[1] == counts[1] + counts[2]
    a.set_counts(dst)
    assert a.fill_unknown(b, *cfg) is None and np.array_equal(a.counts(), got)


def test_all_seven_counts_at_300_x_300():
    name, dst, src, cfg = [c for c in fc.cases() if c[0] == "random_300x300"][0]
    a, b, _ = grids_for(dst, src)
    counts = a.fill_unknown(b, *cfg, return_counts=True)
    assert counts == rr.fill(dst, src, *cfg)[1] and all(w > 0 for w in counts) and sum(counts[:5]) == 90000


def test_a_fill_invalidates_the_plan_and_keeps_the_window_and_the_frames():
    occ = np.zeros((40, 50), dtype=np.int8)
    occ[:, 30:] = -1
    a, b = (K.OccupancyGrid(0.05, -1.0, -1.0, 50, 40, -1.0, 1.0, 1.0) for _ in range(2))
    a.integrate(np.array([[0.3, 0.0, 0.0]]), np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]))
    window, frames = a.last_window(), a.info()["frames"]
    a.set_counts(fr.counts_of(occ))
    b.set_counts(fr.counts_of(np.zeros((40, 50), dtype=np.int8)))
    a.potential(K.nav2_cost_table(0.05, 2, 0.05, 3.0), K.plan_weights(), [(5, 5)])
    assert a.has_plan()
    counts = a.fill_unknown(b, return_counts=True)
    assert not a.has_plan() and counts[2] == 40 * 20 and (a.occupancy(1) == 0).all()
    assert a.last_window() == window and a.info()["frames"] == frames == 1
    with pytest.raises(K.KicpError) as e:
        a.frontiers(use_plan=True)
    assert e.value.code == K.KICP_ERR_ARG and "kicp_grid_potential" in str(e.value)
    a.potential(K.nav2_cost_table(0.05, 2, 0.05, 3.0), K.plan_weights(), [(5, 5)])
    assert a.has_plan()


def test_argument_errors():
    dst, src = fc.table()
    shape = (8, 10)
    geometry = dict(cell=0.25, origin_x=0.5, origin_y=-0.5, width=10, height=8)

    def grid(**changed):
        g = dict(geometry, **changed)
        return K.OccupancyGrid(g["cell"], g["origin_x"], g["origin_y"], g["width"], g["height"], -1.0, 1.0, 2.0)

    a, b = grid(), grid()
    a.set_counts(dst)
    b.set_counts(src)
    a.potential_of_costmap(np.zeros(shape, dtype=np.uint8), K.plan_weights(), [(1, 0)])
    for cfg in ((0, 25, 65), (1, 101, 101), (1, 25, 25), (1, 30, 25), (1, 25, 102), (1, 100, 100)):
        with pytest.raises(K.KicpError) as e:
            a.fill_unknown(b, *cfg)
        assert e.value.code == K.KICP_ERR_ARG, cfg
    with pytest.raises(K.KicpError) as e:
        a.fill_unknown(a)  # dst is src
    assert e.value.code == K.KICP_ERR_ARG
    off_by_one_bit = [dict(cell=np.nextafter(0.25, 1.0)), dict(origin_x=np.nextafter(0.5, 1.0)), dict(origin_y=np.nextafter(-0.5, 0.0)), dict(width=11), dict(height=9)]
    for changed in off_by_one_bit:
        other = grid(**changed)
        for one, two in ((a, other), (other, a)):
            with pytest.raises(K.KicpError) as e:
                one.fill_unknown(two)
            assert e.value.code == K.KICP_ERR_ARG, changed
        assert not other.counts().any()
    lib, cfg, words = K.lib(), K.GridFillConfig(1, 25, 65), (C.c_ulonglong * 7)(*([9] * 7))
    assert lib.kicp_grid_fill_unknown(None, b._h, C.byref(cfg), words) == K.KICP_ERR_ARG
    assert lib.kicp_grid_fill_unknown(a._h, None, C.byref(cfg), words) == K.KICP_ERR_ARG
    assert lib.kicp_grid_fill_unknown(a._h, b._h, None, words) == K.KICP_ERR_ARG
    assert list(words) == [9] * 7 and np.array_equal(a.counts(), dst) and np.array_equal(b.counts(), src) and a.has_plan()  # nothing was written
    assert lib.kicp_grid_fill_unknown(a._h, b._h, C.byref(cfg), None) == K.KICP_OK and np.array_equal(a.counts(), rr.fill(dst, src, 1, 25, 65)[0])
    assert a.counts().shape == shape + (2,)


def test_a_drive_end_to_end():
    """the drive of tests/elev_cases.py into a mapping grid whose band holds the floor - so its returns are hits there: the band's wall -
    and into a layer of equal geometry; the layer's classes with ROUGH into a planner's grid, filled from the mapping grid"""
    cfg, frames, columns = sc.drive_columns()
    (S, H), slope, rough = sc.DRIVE_PARAMS, sc.DRIVE_SLOPE, rc.DRIVE_ROUGH
    band, fill = (-0.5, 1.5), (1, 25, 101)
    # the restatements first, on the CPU
    gcfg = gr.make_config(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], band[0], band[1], cfg["max_ray"])
    src = np.zeros((cfg["height"], cfg["width"], 2), dtype=np.uint16)
    for pts, pose, sensor in frames:
        gr.integrate(gcfg, src, pts, pose, sensor)
    want = rr.classify(columns, S, H, slope, rough)
    unfilled = np.stack([want.classes == 100, want.classes == 0], axis=-1).astype(np.uint16)
    filled, words = rr.fill(unfilled, src, *fill)
    cells_before, cells_after = int(fr.frontier_cells(gr.occupancy(unfilled)).sum()), int(fr.frontier_cells(gr.occupancy(filled)).sum())
    print("fill: counts %s; frontier cells %d unfilled, %d filled" % (words, cells_before, cells_after))
    assert words[2] > 0 and cells_after < cells_before
    # the device
    mapping = K.OccupancyGrid(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], band[0], band[1], cfg["max_ray"])
    layer = K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"])
    for pts, pose, sensor in frames:
        frame = K.DeviceFrame(pts)
        mapping.integrate_device(frame, pose, sensor)
        layer.integrate_device(frame, pose, sensor)
    assert np.array_equal(mapping.counts(), src) and np.array_equal(layer.columns(), columns)
    planner = K.OccupancyGrid(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], -1.0, 1.0, cfg["max_ray"])
    layer.to_grid_rough(planner, S, H, slope, rough)
    assert np.array_equal(planner.counts(), unfilled)
    rows_before = planner.frontiers()
    counts = planner.fill_unknown(mapping, *fill, return_counts=True)
    got = planner.counts()
    assert np.array_equal(got, filled) and counts == words and counts[2] > 0 and np.array_equal(mapping.counts(), src)
    known = want.classes != -1
    assert np.array_equal(planner.occupancy(1)[known], want.classes[known])  # every cell the layer knows keeps the layer's class
    rows_after = planner.frontiers()
    assert int(rows_before[:, 1].sum()) == cells_before and int(rows_after[:, 1].sum()) == cells_after and rows_after[:, 1].sum() < rows_before[:, 1].sum()
