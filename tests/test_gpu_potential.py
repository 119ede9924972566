"""The cost-to-go field on the GPU (kicp_grid_potential, kicp_grid_potential_of_costmap: K.OccupancyGrid.potential,
.potential_of_costmap) against the restatement of include/kicp.h's text (tests/potential_ref.py).  The field is a unique fixed point
over integers, so everything is exact: np.array_equal, no tolerance anywhere.  The round count is implementation-defined and is not
compared; one test asserts that it took more than two batches where the field has to cross about a hundred tile borders.  More than
one workgroup of goals and grids beyond the counting launch's first trip: tests/test_gpu_plan_regimes.py."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import clearance_ref as cr
import potential_ref as pr

pytestmark = pytest.mark.gpu

CASES = pr.small_cases()


def grid_for(width, height):
    return K.OccupancyGrid(0.05, 0.0, 0.0, width, height, 0.0, 1.0, 1.0)


def check(grid, costmap, weight, goals, max_potential, want, want_stats):
    got, stats = grid.potential_of_costmap(costmap, weight, goals, max_potential, return_stats=True)
    assert got.dtype == np.uint32 and got.shape == costmap.shape
    bad = got != want
    print("%d x %d, %d goals, max_potential %d: %d of %d potentials differ, stats %s" % (costmap.shape[1], costmap.shape[0], len(goals), max_potential, bad.sum(), bad.size, stats))
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    assert stats[:3] == tuple(want_stats) and stats[3] >= 1
    return got, stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_small_cases(name):
    """one tile, partial tiles, the halo at the grid's edge (31 / 32 / 33, 63 / 64 / 65), 1 x 1, 1 x 70, 70 x 1, goals in the corners and
    on a tile corner, the diagonal step across four tiles, random weights with 30 % impassable and two goals, the clamp, an enclosed
    region, goals on impassable cells"""
    costmap, weight, goals, max_potential = CASES[name]
    want, want_stats = pr.potential_dijkstra(costmap, weight, goals, max_potential)
    got, _ = check(grid_for(costmap.shape[1], costmap.shape[0]), costmap, weight, goals, max_potential, want, want_stats)
    if name == "pinned_8x6":
        assert np.array_equal(got, pr.pinned_8x6()[3])
    if name == "diagonal_across_four_tiles":
        assert got[31, 31] == (181 * 4 + 64) >> 7 and got[32, 32] == 0
    if name == "enclosed":
        assert (got[11:22, 13:24] == pr.UNREACHED).all() and got[2, 2] == 0 and got[30, 30] < pr.UNREACHED
    if name == "enclosed_goal_inside":
        assert (got[11:22, 13:24] < pr.UNREACHED).all() and (got[:10] == pr.UNREACHED).all()
    if name == "goal_impassable_alone":
        assert (got == pr.UNREACHED).all() and want_stats == (0, 0, 0)  # all goals impassable: nothing is reached, goals used = 0
    if name == "goal_impassable_beside_a_good_one":
        assert want_stats[0] == 1 and got[30, 30] == 0 and got[15, 12] == pr.UNREACHED
    if name == "random_96x70_clamped":
        assert want_stats[2] > 1000 and want_stats[1] > 1000 and got.max() == pr.UNREACHED and (got[got != pr.UNREACHED] <= 5000).all()


def test_serpentine_needs_many_rounds():
    """130 x 100 with a wall on every fourth row: the field crosses tile borders about a hundred times, one round at best per crossing.
    A lost activity flag or a batch loop that stops early leaves the far end unreached or too high."""
    costmap = pr.serpentine()
    want, want_stats = pr.potential_dijkstra(costmap, pr.IDENTITY, [(0, 0)])
    assert want_stats[1] == int((costmap > 0).sum()) and want[99, 129] > 6000  # every passable cell is reached, the far end far
    _, stats = check(grid_for(130, 100), costmap, pr.IDENTITY, [(0, 0)], pr.MAX_POTENTIAL, want, want_stats)
    assert stats[3] >= 2 * 16


@pytest.fixture(scope="module")
def large():
    """260 x 200 random weights, 30 % impassable, three goals: the restatement's potential computed once, unclamped"""
    costmap = pr.random_costmap(260, 200, 21)
    goals = [(5, 7), (250, 190), (130, 100)]
    for x, y in goals:
        costmap[y, x] = 40
    want, stats = pr.potential_dijkstra(costmap, pr.IDENTITY, goals)
    return costmap, goals, want, stats


def clamped(pot, max_potential):
    """clamping at the end is the definition"""
    return np.where(pot == pr.UNREACHED, pot, np.minimum(pot, max_potential)).astype(np.uint32)


@pytest.mark.parametrize("max_potential", [pr.MAX_POTENTIAL, 9000])
def test_260x200(large, max_potential):
    costmap, goals, want, want_stats = large
    if max_potential != pr.MAX_POTENTIAL:
        want = clamped(want, max_potential)
        want_stats = pr.stats_of(want, costmap.astype(np.int64), goals, max_potential)
        assert want_stats[2] > 5000 and want_stats[1] > 5000
    check(grid_for(260, 200), costmap, pr.IDENTITY, goals, max_potential, want, want_stats)


def test_two_calls_on_one_handle_and_the_path(large):
    """different goals, then a smaller field, then the first again on the same handle: stale flags, counters or buffers would show;
    the path over the device's potential is the path over the host's"""
    costmap, goals, want, want_stats = large
    grid = grid_for(260, 200)
    check(grid, costmap, pr.IDENTITY, goals, pr.MAX_POTENTIAL, want, want_stats)
    other = [(259, 0)]
    costmap2 = costmap.copy()
    costmap2[0, 259] = 9
    want2, stats2 = pr.potential_dijkstra(costmap2, pr.IDENTITY, other)
    got2, _ = check(grid, costmap2, pr.IDENTITY, other, pr.MAX_POTENTIAL, want2, stats2)
    want3 = clamped(want2, 700)
    check(grid, costmap2, pr.IDENTITY, other, 700, want3, pr.stats_of(want3, costmap2.astype(np.int64), other, 700))
    got, _ = check(grid, costmap, pr.IDENTITY, goals, pr.MAX_POTENTIAL, want, want_stats)
    host = K.potential_from_costmap(costmap, pr.IDENTITY, goals)
    assert np.array_equal(host, got)
    out = np.zeros_like(got)
    assert grid.potential_of_costmap(costmap, pr.IDENTITY, goals, out=out) is out and np.array_equal(out, want)  # written in place
    starts = [(int(x), int(y)) for y, x in np.argwhere(want < pr.UNREACHED)[::4001]]
    assert len(starts) >= 8
    for start in starts:
        a, b = K.potential_path(got, costmap, pr.IDENTITY, start), K.potential_path(host, costmap, pr.IDENTITY, start)
        assert np.array_equal(a, b) and [tuple(int(v) for v in c) for c in a] == pr.path(want, costmap, pr.IDENTITY, start)
        assert tuple(int(v) for v in a[-1]) in goals


def test_potential_from_the_counters_equals_potential_of_the_costmap():
    """kicp_grid_potential - the costmap never leaves HBM - against potential_of_costmap over kicp_grid_costmap's own bytes, and
    kicp_grid_costmap unchanged by the call in between"""
    occ = cr.random_occupancy(150, 97, 0.01, 31, unknown_fraction=0.03)
    occ[36:48, 55:70] = 0  # nothing within R of the first goal
    grid = grid_for(150, 97)
    grid.set_counts(cr.counts_of(occ))
    table = K.nav2_cost_table(0.05, 4, 0.05, 3.0)
    goals = [(62, 41), (149, 96), (0, 0)]
    for kw in (dict(inflate_unknown=False), dict(inflate_unknown=True, unknown_is_obstacle=False), dict(unknown_is_obstacle=True)):
        for weight in (K.plan_weights(), K.plan_weights(unknown_weight=200)):
            costmap = grid.costmap(table, **kw)
            assert np.array_equal(costmap, cr.costmap(occ, table, 0.65, kw.get("unknown_is_obstacle", False), kw.get("inflate_unknown", False)))
            got, stats = grid.potential(table, weight, goals, return_stats=True, **kw)
            via, via_stats = grid.potential_of_costmap(costmap, weight, goals, return_stats=True)
            want, want_stats = pr.potential_dijkstra(costmap, weight, goals)
            print(kw, "goals used %d, reached %d, rounds %d / %d" % (stats[0], stats[1], stats[3], via_stats[3]))
            assert np.array_equal(got, via) and np.array_equal(got, want) and stats[:3] == via_stats[:3] == want_stats
            assert np.array_equal(grid.costmap(table, **kw), costmap)
    assert want_stats[0] >= 1 and want_stats[1] > 1000
    clamped, stats = grid.potential(table, weight, goals, max_potential=3000, return_stats=True, **kw)
    want, want_stats = pr.potential_dijkstra(costmap, weight, goals, 3000)
    assert np.array_equal(clamped, want) and stats[:3] == want_stats and want_stats[2] > 0


def test_argument_errors_on_the_device():
    grid = grid_for(6, 4)
    costmap = np.zeros((4, 6), dtype=np.uint8)
    weight, table = K.plan_weights(), cr.mixed_table(2)

    def code(fn, *a, **kw):
        with pytest.raises(K.KicpError) as e:
            fn(*a, **kw)
        return e.value.code

    for goals in ([(6, 0)], [(0, 4)], [(0, 0), (7, 7)], [], [(-1, 0)]):
        assert code(grid.potential_of_costmap, costmap, weight, goals) == K.KICP_ERR_ARG, goals
        assert code(grid.potential, table, weight, goals) == K.KICP_ERR_ARG, goals
    for max_potential in (0, 0xFFFFFFFF, -1, 1 << 32):
        assert code(grid.potential_of_costmap, costmap, weight, [(0, 0)], max_potential) == K.KICP_ERR_ARG
        assert code(grid.potential, table, weight, [(0, 0)], max_potential) == K.KICP_ERR_ARG
    assert code(grid.potential_of_costmap, costmap[:3], weight, [(0, 0)]) == K.KICP_ERR_ARG
    assert code(grid.potential_of_costmap, costmap, weight[:255], [(0, 0)]) == K.KICP_ERR_ARG
    assert code(grid.potential, table[:-1], weight, [(0, 0)]) == K.KICP_ERR_ARG
    assert code(grid.potential, table, weight, [(0, 0)], min_observations=0) == K.KICP_ERR_ARG
    assert code(grid.potential, table, weight, [(0, 0)], occupied_thresh=1.5) == K.KICP_ERR_ARG
    assert code(grid.potential, np.zeros(255 * 255 + 2, dtype=np.uint8), weight, [(0, 0)]) == K.KICP_ERR_CAPACITY

    lib = K.lib()
    u8, u32, u64 = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)
    clear, plan = K.GridClearanceConfig(1, 0.65, 0, 2), K.PlanConfig(1000)
    goals, out, stats = np.array([[1, 1]], dtype=np.uint32), np.zeros(24, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    pc, pw, pt, pg, po, ps = costmap.ctypes.data_as(u8), weight.ctypes.data_as(u8), table.ctypes.data_as(u8), goals.ctypes.data_as(u32), out.ctypes.data_as(u32), stats.ctypes.data_as(u64)
    assert lib.kicp_grid_potential_of_costmap(grid._h, pc, pw, C.byref(plan), pg, 1, po, 24, ps) == K.KICP_OK
    assert lib.kicp_grid_potential_of_costmap(grid._h, pc, pw, C.byref(plan), pg, 1, po, 24, None) == K.KICP_OK  # the statistics are optional
    for args in ((None, pc, pw, C.byref(plan), pg, 1, po, 24, ps), (grid._h, None, pw, C.byref(plan), pg, 1, po, 24, ps), (grid._h, pc, None, C.byref(plan), pg, 1, po, 24, ps),
                 (grid._h, pc, pw, None, pg, 1, po, 24, ps), (grid._h, pc, pw, C.byref(plan), None, 1, po, 24, ps), (grid._h, pc, pw, C.byref(plan), pg, 1, None, 24, ps),
                 (grid._h, pc, pw, C.byref(plan), pg, 1, po, 23, ps), (grid._h, pc, pw, C.byref(plan), pg, 0, po, 24, ps)):
        assert lib.kicp_grid_potential_of_costmap(*args) == K.KICP_ERR_ARG
    assert lib.kicp_grid_potential(grid._h, C.byref(clear), pt, 6, 0, pw, C.byref(plan), pg, 1, po, 24, ps) == K.KICP_OK
    for args in ((None, C.byref(clear), pt, 6, 0, pw, C.byref(plan), pg, 1, po, 24, ps), (grid._h, None, pt, 6, 0, pw, C.byref(plan), pg, 1, po, 24, ps),
                 (grid._h, C.byref(clear), None, 6, 0, pw, C.byref(plan), pg, 1, po, 24, ps), (grid._h, C.byref(clear), pt, 5, 0, pw, C.byref(plan), pg, 1, po, 24, ps),
                 (grid._h, C.byref(clear), pt, 6, 0, None, C.byref(plan), pg, 1, po, 24, ps), (grid._h, C.byref(clear), pt, 6, 0, pw, None, pg, 1, po, 24, ps),
                 (grid._h, C.byref(clear), pt, 6, 0, pw, C.byref(plan), None, 1, po, 24, ps), (grid._h, C.byref(clear), pt, 6, 0, pw, C.byref(plan), pg, 1, None, 24, ps),
                 (grid._h, C.byref(clear), pt, 6, 0, pw, C.byref(plan), pg, 1, po, 25, ps)):
        assert lib.kicp_grid_potential(*args) == K.KICP_ERR_ARG
    want, _ = pr.potential_dijkstra(costmap, weight, [(1, 1)], 1000)
    assert np.array_equal(grid.potential_of_costmap(costmap, weight, [(1, 1)], 1000), want)  # the handle is unharmed
