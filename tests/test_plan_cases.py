"""The premises of tests/plan_cases.py, proved on the CPU with numpy and the restatements alone, so that the regime each case of
tests/test_gpu_plan_regimes.py claims is a property of its input, and so that the restatement's answer would differ if the regime
were skipped: goal 257 changes its tile and 600 goals hold duplicates, impassable cells and 40 of one tile; the large map has cells
below and at the clamp past the counting launch's first trip; the tall and the wide grid have 254^2 beside "far", sweeps that run more
than 255 rows past their source and a source exactly R rows to either side; every count shard of the 300 x 300 classifications takes
something from several waves, and the long frame's statistics from many."""
import numpy as np
import pytest

import clearance_ref as cr
import elev_cases as ec
import elev_ref as er
import plan_cases as pc
import potential_ref as pr


# ---- potential ---------------------------------------------------------------------------------------------------------------------
def test_goal_257_is_alone_in_its_workgroup_and_in_its_tile():
    cm, goals = pc.map_96x70(), pc.goals_257()
    assert cm.shape == (70, 96) and 0.25 < (cm == 0).mean() < 0.35
    assert len(goals) == pc.NAV_GOAL_LANES + 1
    corner = pc.tile_of(95, 69, 96)
    assert [pc.tile_of(x, y, 96) for x, y in goals].count(corner) == 1 and pc.tile_of(*goals[-1], 96) == corner
    assert any(cm[y, x] == 0 for x, y in goals[:-1]) and cm[goals[-1][1], goals[-1][0]] > 0
    every, stats = pr.potential_dijkstra(cm, pr.IDENTITY, goals)
    first, first_stats = pr.potential_dijkstra(cm, pr.IDENTITY, goals[:pc.NAV_GOAL_LANES])
    assert stats[0] == first_stats[0] + 1
    assert not np.array_equal(every[64:, 64:], first[64:, 64:]) and every[66, 90] == 0 and first[66, 90] > 0  # a lost second workgroup shows in that tile


def test_600_goals_hold_duplicates_impassable_cells_and_40_of_one_tile():
    cm, goals = pc.map_96x70(), pc.goals_600()
    assert len(goals) == 600 and len(goals) > 2 * pc.NAV_GOAL_LANES  # three workgroups, the last with 88 live lanes
    assert len(goals) - len(set(goals)) >= 50
    x0, y0, w, h = pc.ONE_TILE
    assert sum(1 for x, y in goals if x0 <= x < x0 + w and y0 <= y < y0 + h) >= 40 and x0 % pc.NAV_TILE == 0 and y0 % pc.NAV_TILE == 0 and w == h == pc.NAV_TILE
    impassable = sum(1 for x, y in goals if cm[y, x] == 0)
    assert 0.2 * 600 < impassable < 0.4 * 600
    want, stats = pr.potential_dijkstra(cm, pr.IDENTITY, goals)
    assert stats[0] == 600 - impassable  # duplicates count once each time they are listed
    for part in (goals[:256], goals[:512], goals[256:]):  # no two of the three workgroups make the field alone
        assert not np.array_equal(pr.potential_dijkstra(cm, pr.IDENTITY, part)[0], want)
    assert all(want[y, x] == (0 if cm[y, x] else pr.UNREACHED) or cm[y, x] == 0 for x, y in goals)
    clamped, clamped_stats = pr.potential_dijkstra(cm, pr.IDENTITY, goals, 60)
    assert clamped_stats[1] > 100 and clamped_stats[2] > 100


def test_every_cell_a_goal():
    cm = pc.map_65x63()
    goals = pc.goals_every_cell(65, 63)
    assert len(goals) == 4095 and -(-len(goals) // pc.NAV_GOAL_LANES) == 16 and len(goals) % pc.NAV_GOAL_LANES != 0
    want, stats = pr.potential_dijkstra(cm, pr.IDENTITY, goals)
    assert np.array_equal(want, np.where(cm > 0, 0, pr.UNREACHED).astype(np.uint32))
    assert stats == (int((cm > 0).sum()), int((cm > 0).sum()), 0) and (cm == 0).sum() > 1000


def test_the_large_map_has_cells_past_the_first_trip_of_the_count():
    cm = pc.map_large()
    assert cm.shape == (pc.LARGE_H, pc.LARGE_W) and cm.size == 267800 > pc.NAV_COUNT_LANES
    assert pc.LARGE_W % pc.NAV_TILE != 0 and pc.LARGE_H % pc.NAV_TILE != 0 and (-(-pc.LARGE_W // pc.NAV_TILE), -(-pc.LARGE_H // pc.NAV_TILE)) == (33, 9)
    want, stats = pr.potential_dijkstra(cm, pr.IDENTITY, [pc.LARGE_GOAL])
    assert stats == (1, 13637, 0) and pc.beyond_one_trip(want, pr.MAX_POTENTIAL)[0] > 0
    clamped, stats = pr.potential_dijkstra(cm, pr.IDENTITY, [pc.LARGE_GOAL], pc.LARGE_CLAMP)
    assert stats == (1, 5090, 8547)
    assert pc.beyond_one_trip(clamped, pc.LARGE_CLAMP) == (909, 4747)  # a single trip is wrong in both words


def test_the_large_map_from_counters():
    occ, costmap = pc.occupancy_large()
    cm = pc.map_large()
    q = pc.LARGE_WEIGHT[costmap]
    assert np.array_equal(q > 0, cm > 0)  # the same passable cells
    assert (q[3:250, 5] == 3).all() and (q[0:2] == 2).all() and (q[250:] == 7).all()
    assert set(np.unique(costmap).tolist()) == {0, 1, 254, 255}
    want, stats = pr.potential_dijkstra(costmap, pc.LARGE_WEIGHT, [pc.LARGE_GOAL], pc.LARGE_CLAMP)
    below, equal = pc.beyond_one_trip(want, pc.LARGE_CLAMP)
    assert stats[0] == 1 and below > 0 and equal > 0


def test_the_small_map_embedded_in_the_large_grid():
    cm = pc.embedded_small()
    want, stats = pr.potential_dijkstra(cm, pr.IDENTITY, pc.goals_257())
    small, small_stats = pr.potential_dijkstra(pc.map_96x70(), pr.IDENTITY, pc.goals_257())
    assert np.array_equal(want[:70, :96], small) and stats == small_stats
    assert (want[70:] == pr.UNREACHED).all() and (want[:, 96:] == pr.UNREACHED).all()
    large, _ = pr.potential_dijkstra(pc.map_large(), pr.IDENTITY, [pc.LARGE_GOAL])
    assert ((large != pr.UNREACHED) & (want == pr.UNREACHED)).sum() > 10000  # what the large call left behind must not show


# ---- clearance ---------------------------------------------------------------------------------------------------------------------
def test_the_tall_grid_at_254():
    occ = pc.tall_3x520()
    assert occ.shape == (520, 3) and np.argwhere(occ > 65).tolist() == [[0, 0], [519, 2]] and np.argwhere(occ < 0).tolist() == [[300, 1]]
    assert -(-520 // pc.CLEAR_STRIP) == 3
    full = pc.clearance_of("tall_3x520_r254", False)
    far = 254 * 254 + 1
    assert full[254, 0] == 254 * 254 and full[255, 0] == far  # a source exactly R rows below; 254^2 and "far" are neighbours
    assert full[265, 2] == 254 * 254 and full[264, 2] == far  # ... and one exactly R rows above
    assert full[253, 0] == 253 * 253 and full[254, 1] == far and full[253, 1] == 253 * 253 + 1  # the row scan's k = 1 beside k = 0
    middle = np.flatnonzero((full == far).all(axis=1))
    assert middle.min() == 255 and middle.max() == 264 and len(middle) == 10  # a run of far rows; sweeps run 264 rows past the source
    uio = pc.clearance_of("tall_3x520_r254", True)
    assert uio[300, 1] == 0 and uio[299, 0] == 2 and not (uio == far).any()  # the unknown cell as a source fills the middle
    _, _, rects = pc.clearance_cases()["tall_3x520_r254"]
    clips = set()
    for _, y0, _, h in rects[1:]:
        clips.add((y0 < 254, y0 + h + 254 > 520))
    assert clips == {(False, False), (True, False), (False, True), (True, True)}  # the run-in clipped at neither end, at one, at both


def test_the_wide_grid_is_the_transpose():
    occ = pc.wide_520x3()
    assert occ.shape == (3, 520) and np.array_equal(occ, pc.tall_3x520().T)
    for uio in (False, True):
        assert np.array_equal(pc.clearance_of("wide_520x3_r254", uio), pc.clearance_of("tall_3x520_r254", uio).T)
        assert np.array_equal(pc.clearance_of("wide_520x3_r253", uio), pc.clearance_of("tall_3x520_r253", uio).T)
    _, _, rects = pc.clearance_cases()["wide_520x3_r254"]
    assert {254, 255, 256} <= {r[0] for r in rects[1:]}
    # a rectangle that starts at 255 has its first segment's left halo in the grid and its right one past cell 510: both neighbours
    assert any(x0 >= 254 and x0 + w + 254 > 520 for x0, _, w, _ in rects[1:]) and any(x0 < 254 for x0, _, w, _ in rects[1:])


def test_253_tells_the_radius_from_the_byte():
    full = pc.clearance_of("tall_3x520_r253", False)
    far = 253 * 253 + 1
    assert full[253, 0] == 253 * 253 and full[254, 0] == far and full[266, 2] == 253 * 253 and full[265, 2] == far
    # at R = 253 a column distance of 254 is already "none": a comparison with the constant 254 in place of the radius is right
    # here and wrong at R = 254, where the cells at 254 rows differ between the two
    assert pc.clearance_of("tall_3x520_r254", False)[254, 0] != 254 * 254 + 1


def test_the_sparse_grid_has_scans_that_run_far():
    occ = pc.sparse_300()
    assert occ.shape == (300, 300) and 4 <= (occ > 65).sum() <= 30 and 4 <= (occ < 0).sum() <= 30
    far = 254 * 254 + 1
    for uio in (False, True):
        full = pc.clearance_of("sparse_300x300_r254", uio)
        assert (full[full < far] > 200 * 200).any() and (full == far).any() and (full == 0).sum() == ((occ > 65) | ((occ < 0) & uio)).sum()
    assert (pc.clearance_of("sparse_300x300_r254", False) > 100 * 100).mean() > 0.02
    assert not np.array_equal(pc.clearance_of("sparse_300x300_r254", False), pc.clearance_of("sparse_300x300_r254", True))


def test_the_costmap_of_the_cases_takes_every_branch():
    table = cr.mixed_table(254)
    occ = pc.tall_3x520()
    plain = cr.costmap(occ, table, clear=pc.clearance_of("tall_3x520_r254", False))
    inflated = cr.costmap(occ, table, inflate_unknown=True, clear=pc.clearance_of("tall_3x520_r254", False))
    assert plain[300, 1] == 255 and inflated[300, 1] == table[219 * 219 + 1] > 0
    assert (plain == 254).sum() == 2 and (plain == 253).any() and ((plain > 0) & (plain < 253)).any() and (plain == 0).any()


# ---- height columns ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", pc.SMALL_LAYERS)
def test_small_layers(width, height):
    columns = pc.small_layer_columns(width, height)
    assert columns.shape == (height, width) and columns.dtype == np.uint64
    rects = pc.small_layer_rects(width, height)
    assert rects[0] is None
    for x0, y0, w, h in rects[1:]:
        assert x0 + w == width and y0 + h == height
    if width >= 4 and height >= 5:  # the rectangle from (2, 3): its last tile on either axis reaches past the layer
        x0, y0, w, h = rects[2]
        assert x0 + pc.ELEV_TILE * -(-w // pc.ELEV_TILE) > width and y0 + pc.ELEV_TILE * -(-h // pc.ELEV_TILE) > height
    S, H = 2, 8
    classes, _, body, step = er.classify(columns, S, H)
    if width * height > 1:
        assert (classes == -1).any() and (classes == 100).any() and step.any()
    # a tile that classified alone, its halo unknown, would miss the STEP across each border of the full layer's tiles
    if width > pc.ELEV_TILE or height > pc.ELEV_TILE:
        alone = np.empty_like(classes)
        for by in range(0, height, pc.ELEV_TILE):
            for bx in range(0, width, pc.ELEV_TILE):
                alone[by:by + 16, bx:bx + 16] = er.classify(columns[by:by + 16, bx:bx + 16], S, H)[0]
        differs = np.argwhere(alone != classes)
        assert len(differs) and ({int(x) % 16 for _, x in differs} | {int(y) % 16 for y, _ in differs}) & {0, 15}
    # each corner of the layer is the higher cell of a pair
    if width >= 2 and height >= 2:
        assert classes[0, 0] == classes[0, width - 1] == classes[height - 1, 0] == classes[height - 1, width - 1] == 100
    bait = pc.wrap_bait(width, height)
    if bait:
        x, y = bait
        wrapped = pc.classify_wrapped(columns, S, H)
        assert classes[y, x] == 0 and wrapped[y, x] == 100  # reading (0, y + 1) for the cell beyond the row's end makes it a STEP
    assert (bait is not None) == ((width, height) in [(15, 17), (16, 16), (17, 15), (31, 33), (32, 32), (33, 31)])


def test_the_bait_lies_in_a_rectangle_whose_halo_column_is_the_layers_width():
    """the halo column of a tile is its corner's x + 16: it is x == width for the rectangle from (1, 1) of the layers 17 and 33 wide,
    and for the full layers 16 and 32 wide"""
    for width, height in ((17, 15), (33, 31)):
        x0, y0, w, h = pc.small_layer_rects(width, height)[1]
        assert (x0, y0) == (1, 1) and x0 + pc.ELEV_TILE * -(-w // pc.ELEV_TILE) == width and y0 <= pc.wrap_bait(width, height)[1] < y0 + h
    for width in (16, 32):
        assert width % pc.ELEV_TILE == 0


@pytest.mark.parametrize("which", ["random", "drive"])
def test_300x300_shards_are_shared(which):
    columns = pc.columns_300() if which == "random" else pc.drive_columns()[2]
    assert columns.shape == (300, 300)
    tiles = (-(-300 // pc.ELEV_TILE)) ** 2
    assert tiles == 361 and tiles * 4 == 1444 and tiles * 4 // pc.ELEV_SHARDS == 22
    for S, H in ec.PARAMS:
        classes, ground, body, _ = pc.classified(which, S, H)
        for rect in (None, pc.BIG_RECT):
            r = rect or (0, 0, 300, 300)
            counts = er.counts(er.restrict(classes, r), er.restrict(body, r))
            sums, waves = pc.shard_table(classes, body, rect)
            assert tuple(int(v) for v in sums.sum(axis=0)) == counts and sum(counts) == r[2] * r[3]
            if which == "random":
                assert min(counts) > 64, (S, H, counts)  # no single wave holds a whole count
                # every count has a shard that two waves add to - a store in place of the add loses one of them - and something in
                # the upper half of the shards, which a sum over 32 of them loses
                assert (waves.max(axis=0) >= 2).all() and (sums[32:].sum(axis=0) > 0).all()
            else:
                assert (waves[:, :2].min(axis=0) >= 2).all() and (sums[32:, :2].sum(axis=0) > 0).all()  # unknown and traversable: in every shard
    if which == "drive":
        classes, _, body, _ = pc.classified(which, 2, 8)
        counts = er.counts(classes, body)
        assert min(counts) > 64, counts
    waves_full = pc.shard_table(*[pc.classified(which, 2, 8)[k] for k in (0, 2)])[1]
    assert waves_full[:, 0].min() >= 15  # about 22 waves a shard, most of them with unknown cells


def test_short_frames_end_in_a_partly_filled_wave():
    frames = pc.short_frames()
    assert len(frames) == 2 * len(pc.FRAME_SIZES)
    for name, (pts, pose, sensor) in frames.items():
        n = len(pts)
        assert n in pc.FRAME_SIZES
        columns = np.zeros((16, 16), dtype=np.uint64)
        stats = er.integrate(ec.CFG16, columns, pts, pose, sensor)
        assert sum(stats[:4]) == n and stats[0] > 0
        if n % 64:  # the lanes of the last, partly filled wave count: without them the statistics differ
            cut = er.integrate(ec.CFG16, np.zeros((16, 16), dtype=np.uint64), pts[:n - n % 64], pose, sensor)
            assert cut != stats
    tilted = [frames["tilted_%d" % n] for n in pc.FRAME_SIZES]
    cls = er.point_classes(ec.CFG16, *tilted[-1])[0]
    assert (cls == er.SKIPPED).any() and (cls == er.OUTSIDE_COLUMN).any() and (cls == er.USED).any()


def test_the_long_frame_shares_every_shard():
    pts, pose, sensor = pc.long_frame()
    assert pts.shape == (20000, 3) and -(-20000 // 64) == 313 and 313 // pc.ELEV_SHARDS >= 4
    columns = np.zeros((16, 16), dtype=np.uint64)
    used, skipped, outside_grid, outside_column, new_bits, new_cells = er.integrate(ec.CFG16, columns, pts, pose, sensor)
    assert min(skipped, outside_column, new_bits, new_cells) > 0 and used > 10000
    cls = er.point_classes(ec.CFG16, pts, pose, sensor)[0]
    shard = (np.arange(20000) // 64) % pc.ELEV_SHARDS
    for k in (er.SKIPPED, er.OUTSIDE_COLUMN):
        per_wave = np.bincount(np.arange(20000) // 64, weights=(cls == k), minlength=313)
        waves = np.bincount(np.arange(313) % pc.ELEV_SHARDS, weights=per_wave > 0, minlength=pc.ELEV_SHARDS)
        # more waves than shards have something to add, so shards are shared whatever the order; and the upper half takes some
        assert (per_wave > 0).sum() > pc.ELEV_SHARDS and waves.max() >= 2 and ((cls == k) & (shard >= 32)).sum() > 0
