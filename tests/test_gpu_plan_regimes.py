"""The occupancy grid's plan, clearance and height-column kernels in the regimes their own suites never enter (tests/plan_cases.py holds
the cases, tests/test_plan_cases.py proves on the CPU that each case enters its regime and that the answer would differ without it):

  potential   k_nav_goals with more than one workgroup of goals - 257, 600 with duplicates and impassable ones, every cell of 65 x 63 -
              and k_nav_count on 267 800 cells, where its 1 024 workgroups stride a second time; then the small map on the large
              map's handle.
  clearance   k_clear_columns and k_clear_rows at R = 254 and 253 on grids 520 cells long: column distances of 253, 254 and "none",
              sweeps saturating past 255 rows, `m > radius` where m == radius and "none" are neighbours, row scans to k = 254 with
              both halos from neighbouring segments, three strips with their run-in; 300 x 300 with scans that run the full radius.
  columns     k_elev_classify and k_elev_to_grid on layers with sides 1, 15 .. 17, 31 .. 33 and 40, and on 300 x 300 cells, where 1 444
              waves share the 64 shards of the four counts; k_elev_mark with a partly filled last wave and workgroup, and with 313
              waves on the 64 shards of its statistics.

Everything is integer and unique: np.array_equal against the Python restatements (potential_ref, clearance_ref, elev_ref), no
tolerance anywhere, and against the pure-host entries where one exists.  Round counts are printed, never asserted beyond >= 1."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import clearance_ref as cr
import elev_cases as ec
import elev_ref as er
import plan_cases as pc
import potential_ref as pr

pytestmark = pytest.mark.gpu


def grid_for(width, height):
    return K.OccupancyGrid(0.05, 0.0, 0.0, width, height, 0.0, 1.0, 1.0)


def check_potential(grid, costmap, weight, goals, max_potential, want, want_stats, host=False):
    got, stats = grid.potential_of_costmap(costmap, weight, goals, max_potential, return_stats=True)
    assert got.dtype == np.uint32 and got.shape == costmap.shape
    bad = got != want
    print("%d x %d, %d goals, max_potential %d: %d of %d potentials differ, stats %s, restatement %s" %
          (costmap.shape[1], costmap.shape[0], len(goals), max_potential, bad.sum(), bad.size, stats, want_stats))
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    assert stats[:3] == tuple(want_stats) and stats[3] >= 1
    if host:
        on_host, host_stats = K.potential_from_costmap(costmap, weight, goals, max_potential, return_stats=True)
        assert np.array_equal(on_host, got) and tuple(host_stats[:3]) == tuple(want_stats)
    return got, stats


# ---- potential ---------------------------------------------------------------------------------------------------------------------
def test_257_goals():
    """the second workgroup of k_nav_goals holds one goal, the only one of the far corner tile"""
    cm, goals = pc.map_96x70(), list(pc.goals_257())
    want, want_stats = pr.potential_dijkstra(cm, pr.IDENTITY, goals)
    got, _ = check_potential(grid_for(96, 70), cm, pr.IDENTITY, goals, pr.MAX_POTENTIAL, want, want_stats, host=True)
    assert got[66, 90] == 0


@pytest.mark.parametrize("max_potential", [pr.MAX_POTENTIAL, 60])
def test_600_goals(max_potential):
    """three workgroups, the last partly filled; 50 goals listed twice, about 30 % on impassable cells, 40 raising one tile's flag"""
    cm, goals = pc.map_96x70(), list(pc.goals_600())
    want, want_stats = pr.potential_dijkstra(cm, pr.IDENTITY, goals, max_potential)
    got, stats = check_potential(grid_for(96, 70), cm, pr.IDENTITY, goals, max_potential, want, want_stats, host=True)
    assert stats[0] == sum(1 for x, y in goals if cm[y, x] > 0)
    assert all(got[y, x] == (0 if cm[y, x] else pr.UNREACHED) for x, y in goals)


def test_every_cell_a_goal():
    """4 095 goals, 16 workgroups, the last with 255 live lanes: every passable cell is 0, every impassable one unreached"""
    cm = pc.map_65x63()
    goals = list(pc.goals_every_cell(65, 63))
    want, want_stats = pr.potential_dijkstra(cm, pr.IDENTITY, goals)
    got, stats = check_potential(grid_for(65, 63), cm, pr.IDENTITY, goals, pr.MAX_POTENTIAL, want, want_stats, host=True)
    assert np.array_equal(got, np.where(cm > 0, 0, pr.UNREACHED).astype(np.uint32)) and stats[3] >= 1


@pytest.fixture(scope="module")
def large():
    """the restatement's potentials of the 1 030 x 260 map, unclamped and clamped, computed once"""
    cm = pc.map_large()
    return cm, {m: pr.potential_dijkstra(cm, pr.IDENTITY, [pc.LARGE_GOAL], m) for m in (pr.MAX_POTENTIAL, pc.LARGE_CLAMP)}


@pytest.fixture(scope="module")
def large_grid():
    return grid_for(pc.LARGE_W, pc.LARGE_H)


@pytest.mark.parametrize("max_potential", [pr.MAX_POTENTIAL, pc.LARGE_CLAMP])
def test_the_count_strides_over_267800_cells(large, large_grid, max_potential):
    """k_nav_count's second trip: cells below and at the clamp lie at flat indices past 1 024 x 256"""
    cm, wants = large
    want, want_stats = wants[max_potential]
    assert min(pc.beyond_one_trip(want, max_potential)) > 0 or max_potential == pr.MAX_POTENTIAL
    check_potential(large_grid, cm, pr.IDENTITY, [pc.LARGE_GOAL], max_potential, want, want_stats, host=max_potential == pc.LARGE_CLAMP)


def test_the_large_map_from_counters(large_grid):
    """kicp_grid_potential at this size: the costmap comes from the counters in HBM"""
    occ, costmap = pc.occupancy_large()
    grid = large_grid
    grid.set_counts(cr.counts_of(occ))
    assert np.array_equal(grid.costmap(pc.LARGE_TABLE), costmap)
    for max_potential in (pr.MAX_POTENTIAL, pc.LARGE_CLAMP):
        want, want_stats = pr.potential_dijkstra(costmap, pc.LARGE_WEIGHT, [pc.LARGE_GOAL], max_potential)
        got, stats = grid.potential(pc.LARGE_TABLE, pc.LARGE_WEIGHT, [pc.LARGE_GOAL], max_potential, return_stats=True)
        print("from counters, max_potential %d: stats %s, restatement %s" % (max_potential, stats, want_stats))
        assert np.array_equal(got, want) and stats[:3] == want_stats and stats[3] >= 1
    assert min(pc.beyond_one_trip(want, pc.LARGE_CLAMP)) > 0


def test_the_small_call_after_the_large_one_on_one_handle(large):
    """the 1 030 x 260 field, then the 257 goals on the 96 x 70 map in the corner of an impassable 1 030 x 260 costmap, then the large
    one again: flags, counters or goals that a call left behind would show"""
    cm, wants = large
    grid = grid_for(pc.LARGE_W, pc.LARGE_H)
    check_potential(grid, cm, pr.IDENTITY, [pc.LARGE_GOAL], pc.LARGE_CLAMP, *wants[pc.LARGE_CLAMP])
    small, goals = pc.embedded_small(), list(pc.goals_257())
    want, want_stats = pr.potential_dijkstra(small, pr.IDENTITY, goals)
    got, _ = check_potential(grid, small, pr.IDENTITY, goals, pr.MAX_POTENTIAL, want, want_stats)
    assert got[66, 90] == 0 and (got[70:] == pr.UNREACHED).all()
    check_potential(grid, cm, pr.IDENTITY, [pc.LARGE_GOAL], pr.MAX_POTENTIAL, *wants[pr.MAX_POTENTIAL])


# ---- clearance and costmap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.clearance_cases()))
def test_clearance_at_the_largest_radii(name):
    occ, radius, rects = pc.clearance_cases()[name]
    H, W = occ.shape
    grid = K.OccupancyGrid(0.05, 0.0, 0.0, W, H, 0.0, 1.0, 1.0)
    grid.set_counts(cr.counts_of(occ))
    assert np.array_equal(grid.occupancy(), occ)
    table = cr.mixed_table(radius)
    for uio in (False, True):
        full = pc.clearance_of(name, uio)
        assert np.array_equal(K.clearance_from_occupancy(occ, radius, unknown_is_obstacle=uio), full)
        costs = {inflate: cr.costmap(occ, table, 0.65, uio, inflate, clear=full) for inflate in (False, True)}
        for inflate in (False, True):
            assert np.array_equal(K.costmap_from_occupancy(occ, table, unknown_is_obstacle=uio, inflate_unknown=inflate), costs[inflate])
        for rect in rects:
            x0, y0, w, h = rect or (0, 0, W, H)
            got = grid.clearance(radius, unknown_is_obstacle=uio, rect=rect)
            assert got.dtype == np.uint16 and got.shape == (h, w)
            bad = got != full[y0:y0 + h, x0:x0 + w]
            print("%s R %d rect %s uio %d: %d of %d clearances differ" % (name, radius, rect, uio, bad.sum(), bad.size))
            assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], full[y0:y0 + h, x0:x0 + w][bad][:5])
            for inflate in (False, True):
                got = grid.costmap(table, unknown_is_obstacle=uio, inflate_unknown=inflate, rect=rect)
                assert got.dtype == np.uint8 and got.shape == (h, w)
                bad = got != costs[inflate][y0:y0 + h, x0:x0 + w]
                assert not bad.any(), (rect, uio, inflate, np.argwhere(bad)[:5])


# ---- height columns ----------------------------------------------------------------------------------------------------------------
def layer_for(width, height):
    return K.ElevationLayer(0.25, 0.0, 0.0, width, height, 0.0, 0.125, 2.0)


def check_classification(layer, columns, rects, wants):
    """every rectangle with the ground bytes and the counts, and the plain call; wants: (S, H) -> er.classify's result"""
    height, width = columns.shape
    for (S, H), (cls, ground, body, _) in wants.items():
        for rect in rects:
            r = rect or (0, 0, width, height)
            got, got_ground, got_counts = layer.traversability(S, H, rect=rect, return_ground=True, return_counts=True)
            assert got.dtype == np.int8 and got.shape == (r[3], r[2])
            assert np.array_equal(got, er.restrict(cls, r)), (S, H, rect, np.argwhere(got != er.restrict(cls, r))[:5])
            assert np.array_equal(got_ground, er.restrict(ground, r)), (S, H, rect)
            want_counts = er.counts(er.restrict(cls, r), er.restrict(body, r))
            assert got_counts == want_counts, (S, H, rect, got_counts, want_counts)
            assert np.array_equal(layer.traversability(S, H, rect=rect), got)  # without the optional outputs
            on_host, host_ground, host_counts = K.traversability_from_columns(columns, S, H, rect=rect, return_ground=True, return_counts=True)
            assert np.array_equal(on_host, got) and np.array_equal(host_ground, got_ground) and tuple(host_counts) == want_counts


@pytest.mark.parametrize("width,height", pc.SMALL_LAYERS)
def test_small_layers(width, height):
    """the 16-cell tile and its 68-lane halo load on layers of one cell, one row, one column, and sides around one and two tiles;
    then k_elev_to_grid on the same shape"""
    columns = pc.small_layer_columns(width, height)
    layer = layer_for(width, height)
    layer.set_columns(columns)
    assert np.array_equal(layer.columns(), columns)
    wants = {(S, H): er.classify(columns, S, H) for S, H in ec.PARAMS}
    check_classification(layer, columns, pc.small_layer_rects(width, height), wants)
    grid = K.OccupancyGrid(0.25, 0.0, 0.0, width, height, -1.0, 1.0, 2.0)
    for S, H in ec.PARAMS[:2]:
        classes = wants[(S, H)][0]
        grid.set_counts(np.full((height, width, 2), 7, dtype=np.uint16))  # every counter is replaced
        layer.to_grid(grid, S, H)
        counts = grid.counts()
        assert np.array_equal(counts[:, :, 0], (classes == 100).astype(np.uint16)) and np.array_equal(counts[:, :, 1], (classes == 0).astype(np.uint16))
        assert np.array_equal(grid.occupancy(1), classes)


@pytest.mark.parametrize("which", ["random", "drive"])
def test_300x300_counts_where_waves_share_a_shard(which):
    """19 x 19 tiles, 1 444 waves, about 22 on each of the 64 shards: classes, ground bytes and all four counts of the full layer and
    of a rectangle, on random sparse columns (set_columns) and on the columns six frames of a drive leave (integrate)"""
    if which == "random":
        columns = pc.columns_300()
        layer = layer_for(300, 300)
        layer.set_columns(columns)
    else:
        cfg, frames, columns = pc.drive_columns()
        layer = K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"])
        for pts, pose, sensor in frames:
            layer.integrate(pts, pose, sensor)
    assert np.array_equal(layer.columns(), columns)
    wants = {(S, H): pc.classified(which, S, H) for S, H in ec.PARAMS}
    check_classification(layer, columns, [None, pc.BIG_RECT], wants)
    if which == "random":
        grid = K.OccupancyGrid(0.25, 0.0, 0.0, 300, 300, -1.0, 1.0, 2.0)
        grid.set_counts(np.full((300, 300, 2), 7, dtype=np.uint16))
        layer.to_grid(grid, 2, 8)
        assert np.array_equal(grid.occupancy(1), wants[(2, 8)][0])


def check_frame(layer, want, pts, pose, sensor):
    stats = er.integrate(ec.CFG16, want, pts, pose, sensor)
    got = layer.integrate(pts, pose, sensor)
    print("frame: n = %d, restatement %s, device %s" % (len(pts), stats, got))
    assert got == stats and layer.last_frame() == stats and sum(got[:4]) == len(pts)
    assert np.array_equal(layer.columns(), want)
    return stats


@pytest.mark.parametrize("name", sorted(pc.short_frames()))
def test_frames_that_end_inside_a_wave_or_a_workgroup(name):
    """63, 64, 65, 255, 256 and 257 points onto a fresh layer, then the same frame again: nothing is new"""
    pts, pose, sensor = pc.short_frames()[name]
    layer = K.ElevationLayer(*[ec.CFG16[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_origin", "slab", "max_ray")])
    want = np.zeros((16, 16), dtype=np.uint64)
    first = check_frame(layer, want, pts, pose, sensor)
    again = check_frame(layer, want, pts, pose, sensor)
    assert again[:4] == first[:4] and again[4:] == (0, 0) and first[4] > 0


def test_a_frame_of_20000_points():
    """313 waves on the 64 shards of the frame statistics"""
    pts, pose, sensor = pc.long_frame()
    layer = K.ElevationLayer(*[ec.CFG16[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_origin", "slab", "max_ray")])
    want = np.zeros((16, 16), dtype=np.uint64)
    stats = check_frame(layer, want, pts, pose, sensor)
    assert min(stats[1], stats[3], stats[4], stats[5]) > 0
    got = layer.integrate_device(K.DeviceFrame(pts), pose, sensor)
    assert got == stats[:4] + (0, 0) and np.array_equal(layer.columns(), want)
