"""The occupancy grid's frame kernels and the depth view with its sweep in the regimes their own suites never enter (tests/frame_cases.py
holds the cases, tests/test_frame_cases.py proves on the CPU that each case enters its regime and that the answer would differ without it):

  grid   k_grid_mark, k_grid_rays and k_grid_apply at reach 4095, the limit - a window of 8191^2 cells, walks of 4095 steps - on
         8191 x 9 and 9 x 8191; 524 588 points, dense and sparse, whose ray list is longer than the 8 192 waves k_grid_rays is launched
         with, after a 65-point frame on the same handle; sensors whose window corner is 2^30, 2^30 + 1 and far beyond 32 bits;
         windows that are all endpoints and all rays; endpoint pairs in one plane word across two window rows; frames of 1 .. 257 points,
         every lane appending to the ray list; k_grid_readout at the counters' ends on 255 and 257 cells.
  view   k_view_render and k_view_classify at res 8 and res 1024 (clamped pixels on all six faces, ties, borders), window 3 - an
         unrolled instantiation of its own - and window 4 with min_rays - 1 against min_rays returns at corners, edges and inside;
         depths that are +inf, denormal, zero and rounding ties as floats; 1 .. 257 points, 5 000 / 3 / 70 000 queries on one handle,
         200 000 returns in one pixel.  k_view_list and k_view_sweep on buckets of 63 .. 128 points, on a 3 x 3 x 3 block that loses its
         centre, everything and a face, and on map points at exactly max_ray.

Everything is integer or bit-exact and unique: np.array_equal (images also byte for byte) against the numpy restatements (grid_ref,
view_ref), okicp.VoxelHashMap for the swept maps, and the pure-host entry where one exists - no tolerance anywhere.  Each test prints
its counts, restatement against device."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import frame_cases as fc
import grid_cases as gc
import grid_ref as gr
import view_cases as vc
import view_ref as vr
from checkers import okicp
from mapdev_ref import bucket_sorted
from test_gpu_grid import check_frames, make_grid
from test_gpu_view import check_case, make_view
from test_gpu_view_map import MAX_DISTANCE, build, check_sweep, wall, wall_view  # noqa: F401  (wall is a fixture)

pytestmark = pytest.mark.gpu


# ---- grid --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True], ids=["8191x9", "9x8191"])
def test_reach_4095(transposed):
    """the largest legal reach: 16 773 121 plane words, the last with one cell; the second frame from a sensor moved by (+3, -2) cells
    would show a plane byte the first frame's k_grid_apply failed to clear"""
    cfg, frames, cells = fc.reach_frames(transposed)
    grid, counts = check_frames(cfg, frames[:1])
    assert grid.info()["reach"] == 4095 and grid.last_frame()[3] >= 8000
    assert grid.last_window() == (0, 0, cfg["width"], cfg["height"])
    grid, counts = check_frames(cfg, frames[1:], grid, counts, device=True)
    assert counts[:, :, 1].max() == 2 and grid.last_frame()[3] >= 8000


def run_frame(grid, frame, want_counts, want_stats, device):
    pts, pose, sensor = frame
    got = grid.integrate_device(K.DeviceFrame(pts), pose, sensor) if device else grid.integrate(pts, pose, sensor)
    print("frame: n = %d, restatement %s, device %s" % (len(pts), want_stats, got))
    assert got == want_stats and grid.last_frame() == want_stats
    counts = grid.counts()
    bad = counts != want_counts
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])


@pytest.fixture(scope="module")
def big():
    """the restatement of the large frame, the 65 points and the large frame again, computed once"""
    cfg, frames = fc.big_sequence()
    after, stats = gc.reference_run(cfg, frames)
    for a in after:
        a.setflags(write=False)
    return cfg, frames, after, stats


def test_large_frame_strides_the_ray_list(big):
    """2 050 workgroups of k_grid_mark, 14 526 list entries on the 8 192 waves of k_grid_rays; then 65 points, then the large frame from
    HBM: no stale list entry is read.  On a second handle the list grows from 97 entries, with its stream drained first"""
    cfg, frames, after, stats = big
    grid = make_grid(cfg)
    for k, device in enumerate((False, False, True)):
        run_frame(grid, frames[k], after[k], stats[k], device)
    assert grid.info()["frames"] == 3
    other = make_grid(cfg)
    want = np.zeros_like(after[0])
    small = gr.integrate(cfg, want, *frames[1])
    run_frame(other, frames[1], want, small, False)
    run_frame(other, frames[0], after[1], stats[0], True)  # (nothing saturates: the two frames add up in either order)


def test_sparse_large_frame_needs_every_list_entry():
    """9 000 long rays that hardly cross: the 808 entries past the first trip of k_grid_rays carry MISS cells of their own"""
    cfg, frame = fc.sparse_big_frame()
    want = np.zeros((cfg["height"], cfg["width"], 2), dtype=np.uint16)
    stats = gr.integrate(cfg, want, *frame)
    grid = make_grid(cfg)
    run_frame(grid, frame, want, stats, False)
    assert stats[2] == fc.SPARSE_CELLS and stats[3] > 20 * fc.SPARSE_CELLS
    run_frame(grid, frame, 2 * want, stats, True)


@pytest.mark.parametrize("name", sorted(fc.far_sensors()))
def test_far_sensor(name):
    """two points are used and nothing else happens: whatever the corner - 2^30, the last legal one, or kGridFarAway - no window cell is
    inside the grid"""
    pts, pose, sensor, cell = fc.far_sensors()[name]
    start = np.random.default_rng(7).integers(0, 65536, (16, 16, 2)).astype(np.uint16)
    grid = make_grid(fc.CFG16)
    grid.set_counts(start)
    for device in (False, True):
        got = grid.integrate_device(K.DeviceFrame(pts), pose, sensor) if device else grid.integrate(pts, pose, sensor)
        print("%s: sensor cell %d, device %s" % (name, cell, got))
        assert got == (2, 0, 0, 0) and grid.last_window() == (0, 0, 0, 0)
        assert np.array_equal(grid.counts(), start)
    check_frames(fc.CFG16, [(np.array([[0.6, 0.1, 0.0]]), gc.IDENTITY, fc.SENSOR16)], grid, start)  # and the planes were left clean


@pytest.mark.parametrize("reach", [6, 60])
def test_windows_of_endpoints_and_of_rays(reach):
    """every lane of k_grid_apply adds four hits (the packed wave sum carries 256 in its low half), then four misses (in its high half)"""
    side = 2 * reach + 1
    cfg, frame = fc.window_frame(reach, "endpoints")
    grid, counts = check_frames(cfg, [frame, frame])
    assert grid.last_frame() == (side * side, 0, side * side, 0) and counts[:, :, 1].sum() == 0
    cfg, frame = fc.window_frame(reach, "rays")
    grid, counts = check_frames(cfg, [frame, frame], device=True)
    assert grid.last_frame() == (8 * reach, 0, 8 * reach, (side - 2) ** 2)
    check_frames(cfg, [fc.window_frame(reach, "endpoints")[1]], grid, counts)  # the other kind on the same handle


def test_plane_words_shared_by_two_window_rows():
    pairs = fc.shared_word_pairs()
    for at, pair in pairs:
        cfg, frame = fc.offsets_frame(6, list(pair))
        grid, counts = check_frames(cfg, [frame, frame])
        assert grid.last_frame()[:3] == (2, 0, 2) and counts[:, :, 0].sum() == 4
    cfg, frame = fc.offsets_frame(6, [p for _, pair in pairs for p in pair])
    grid, counts = check_frames(cfg, [frame, frame], device=True)
    assert grid.last_frame()[:3] == (8, 0, 8)


@pytest.mark.parametrize("n", fc.WAVE_EDGES)
def test_short_frames(n):
    """every point is used and is the first of its cell: every live lane appends to the ray list through the ballot prefix"""
    cfg, frame = fc.own_cell_frame(n)
    grid, counts = check_frames(cfg, [frame, frame])
    assert grid.last_frame()[:3] == (n, 0, n)
    check_frames(cfg, [frame], grid, counts, device=True)


@pytest.mark.parametrize("width,height", fc.READOUT_SHAPES)
def test_readout_at_the_counters_ends(width, height):
    counts = fc.readout_counts(width, height)
    grid = K.OccupancyGrid(0.25, 0.0, 0.0, width, height, 0.0, 1.0, 1.0)
    grid.set_counts(counts)
    assert np.array_equal(grid.counts(), counts)
    for m in fc.MIN_OBSERVATIONS:
        want = gr.occupancy(counts, m)
        got, on_host = grid.occupancy(m), K.occupancy_from_counts(counts, m)
        print("%d x %d, min_observations %d: %d cells known, device %d, host entry %d" % (width, height, m, (want >= 0).sum(), (got >= 0).sum(), (on_host >= 0).sum()))
        assert got.dtype == np.int8 and np.array_equal(got, want) and np.array_equal(on_host, want)


# ---- depth view ----------------------------------------------------------------------------------------------------------------------
def same_bits(image, depth):
    return image.tobytes() == depth.tobytes()  # (np.array_equal takes -0.0 for 0.0)


def test_res_8():
    case, exact = fc.res8_case()
    for c in (case, exact):
        _, image, verdicts = check_case(c)
        _, from_device, v_device = check_case(c, device=True)
        assert same_bits(image, from_device) and np.array_equal(verdicts, v_device)
    assert verdicts.tolist() == [vc.T] * 8 and np.isfinite(image).sum() == 8


@pytest.fixture(scope="module")
def res1024():
    """the restatement of the res-1024 case, computed once: (case, image, statistics, sensor, verdicts)"""
    case = fc.res1024_case()
    depth, stats, c = vr.render(case["cfg"], case["frame"], case["pose"], case["sensor"])
    verdicts = vr.verdict(case["cfg"], depth, c, case["queries"])
    depth.setflags(write=False), verdicts.setflags(write=False)
    return case, depth, stats, c, verdicts


def test_res_1024(res1024):
    """6 291 456 pixels, 304 000 returns, window 4 with min_rays 81: the whole image bit for bit, the statistics and every verdict; pixel
    1024 clamped to 1023 on all six faces, the tie rules, a border hit exactly"""
    case, depth, stats, c, want = res1024
    view = make_view(case["cfg"])
    for device in (False, True):
        got = view.render_device(K.DeviceFrame(case["frame"]), case["pose"], case["sensor"]) if device else view.render(case["frame"], case["pose"], case["sensor"])
        image = view.depth()
        bad = image.view(np.uint32) != depth.view(np.uint32)
        verdicts = view.classify(case["queries"])
        print("res 1024: restatement %s, device %s; %d of %d pixels differ; verdicts %s, device %s" %
              (stats, got, bad.sum(), bad.size, np.bincount(want, minlength=4).tolist(), np.bincount(verdicts, minlength=4).tolist()))
        assert got == stats and not bad.any() and np.array_equal(verdicts, want)
    for _, (face, u, w) in fc.directed_1024():
        assert image[face, w, u] <= np.float32(8.0)


@pytest.mark.parametrize("name,res,window,min_rays,filled", fc.patch_cases(), ids=[p[0] for p in fc.patch_cases()])
def test_patches_flip_the_verdict_at_min_rays(name, res, window, min_rays, filled):
    """view_window<3> and view_window<4> with windows clipped on one side (edges) and on two (corners)"""
    case, want = fc.patch_case(res, window, min_rays, filled)
    _, image, verdicts = check_case(case)
    print("%s: expected %s, device %s" % (name, want, verdicts.tolist()))
    assert verdicts.tolist() == want and int(np.isfinite(image).sum()) == len(case["frame"])


def test_depths_no_normal_float_holds():
    """(float)m, round to nearest even, denormals kept: 5e38 leaves its pixel empty, 1e-40 a denormal, 3e-46 +0.0, the two ties go to even"""
    case, want, pixels = fc.tiny_case()
    depth, _, _ = vr.render(case["cfg"], case["frame"], case["pose"], case["sensor"])
    for device in (False, True):
        _, image, verdicts = check_case(case, device=device)
        print("pixels: restatement %s, device %s; verdicts %s" % ({k: hex(int(depth[k].view(np.uint32))) for k in pixels},
                                                               {k: hex(int(image[k].view(np.uint32))) for k in pixels}, verdicts.tolist()))
        assert same_bits(image, depth) and verdicts.tolist() == want
        assert int(np.isfinite(image).sum()) == len(pixels) and all(image[k].tobytes() == v.tobytes() for k, v in pixels.items())


def test_points_and_queries_at_the_wave_and_workgroup_edges():
    cfg, pose, sensor, frame, queries = fc.edge_points()
    view = make_view(cfg)
    for n in fc.WAVE_EDGES:
        for device in (False, True):
            check_case(fc.view_case(cfg, frame[:n], queries[:n], pose, sensor), device=device, view=view)
    depth, _, c = vr.render(cfg, frame, pose, sensor)
    want = vr.verdict(cfg, depth, c, queries)
    for n in (5000, 3, 70000):  # the verdict buffer grows, shrinks in use and grows again: nothing stale is read
        got = view.classify(queries[:n])
        print("%d queries: restatement %s, device %s" % (n, np.bincount(want[:n], minlength=4).tolist(), np.bincount(got, minlength=4).tolist()))
        assert np.array_equal(got, want[:n])


@pytest.mark.parametrize("minimum_first", [False, True], ids=["minimum_last", "minimum_first"])
def test_200000_returns_in_one_pixel(minimum_first):
    """782 workgroups doing atomicMin on one word"""
    cfg = vr.make_config(16, 0, 1, 10.0, 0.25, 0.0)
    pts = fc.contended_frame(minimum_first)
    view, image, _ = check_case(fc.view_case(cfg, pts, [[2.0, 0.1, 0.1], [2.4, 0.12, 0.12]]), device=True)
    assert view.last_frame() == (fc.CONTENDED_N, 0) and np.isfinite(image).sum() == 1 and image[0, 8, 8] == np.float32(fc.CONTENDED_MIN)


@pytest.mark.parametrize("name", fc.BUCKET_PATTERNS)
def test_buckets_at_the_trip_edges(name, wall):
    """buckets of 63, 64, 65, 127 and 128 points (one trip with a dead lane, one full trip, a second trip of one lane, two trips):
    everything but the last point seen through, only the last, only the first, none - the early return after the in-range count"""
    case = fc.bucket_sweep_cases()[name]
    rng = np.random.default_rng(8)
    gmap, before = build(case)
    view = wall_view(wall)
    want, _, stats = check_sweep(gmap, view, vc.WALL_CFG, wall["depth"], wall["c"], before, case["vs"], case["cap"], rng)
    assert stats == (len(before), int(case["pattern"].sum()), 0 if name == "none" else 5, 0)
    again, _, stats2 = check_sweep(gmap, view, vc.WALL_CFG, wall["depth"], wall["c"], want, case["vs"], case["cap"], rng)
    assert stats2 == (len(want), 0, 0, 0) and len(again) == len(want)
    gmap.UpdateDevice(K.DeviceFrame(case["points"]), vc.IDENTITY)  # the shortened buckets take points again as the oracle's do
    omap = okicp.VoxelHashMap(case["vs"], MAX_DISTANCE, case["cap"])
    omap.AddPoints(want)
    omap.Update(case["points"], vc.IDENTITY)
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), case["vs"]), bucket_sorted(omap.Pointcloud(), case["vs"])) and gmap.check() == 0


@pytest.mark.parametrize("name", ["centre", "all", "face"])
def test_erased_voxels_and_their_neighbours(name):
    """a 3 x 3 x 3 block: only the centre erased (its 26 neighbours forget it, each through another shift), all 27 erased at once
    (neighbours erase each other concurrently), one face of 9 erased"""
    case = fc.block_cases()[name]
    rng = np.random.default_rng(9)
    gmap, before = build(case)
    view = make_view(case["cfg"])
    depth, rstats, c = vr.render(case["cfg"], case["frame"], vc.IDENTITY, vc.ORIGIN)
    assert view.render(case["frame"], vc.IDENTITY, vc.ORIGIN) == rstats
    want, _, stats = check_sweep(gmap, view, case["cfg"], depth, c, before, case["vs"], case["cap"], rng)
    assert stats[3] == case["erased"] and gmap.num_voxels() == 27 - case["erased"]
    again, _, stats2 = check_sweep(gmap, view, case["cfg"], depth, c, want, case["vs"], case["cap"], rng)
    assert stats2[1:] == (0, 0, 0)
    gmap.UpdateDevice(K.DeviceFrame(case["points"]), vc.IDENTITY)  # the erased voxels come back and are seen by their neighbours again
    omap = okicp.VoxelHashMap(case["vs"], MAX_DISTANCE, case["cap"])
    omap.AddPoints(want)
    omap.Update(case["points"], vc.IDENTITY)
    cloud = bucket_sorted(omap.Pointcloud(), case["vs"])
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), case["vs"]), cloud) and gmap.check() == 0 and gmap.num_voxels() == 27
    queries = case["points"] + rng.uniform(-0.9, 0.9, case["points"].shape)
    nn, d = gmap.GetClosestNeighbor(queries)
    nn_o, d_o = omap.GetClosestNeighbor(queries)
    assert np.array_equal(nn, nn_o) and np.array_equal(d, d_o)


@pytest.mark.parametrize("vs", [1.0, 0.3])
def test_range_cull_and_a_view_that_sees_nothing(vs):
    """map points at exactly max_ray on all six faces are listed by k_view_list and counted in range; a voxel wholly beyond max_ray is
    not touched; after a frame with a NaN pose the sweep removes and counts nothing"""
    data = fc.cull_case()
    case = dict(vs=vs, cap=20, points=data["points"])
    rng = np.random.default_rng(10)
    gmap, before = build(case)
    view = make_view(fc.CULL_CFG)
    depth, rstats, c = vr.render(fc.CULL_CFG, data["frame"], vc.IDENTITY, fc.CULL_SENSOR)
    assert view.render(data["frame"], vc.IDENTITY, fc.CULL_SENSOR) == rstats
    want, _, stats = check_sweep(gmap, view, fc.CULL_CFG, depth, c, before, vs, 20, rng)
    assert stats[0] == 6 + data["removed"] and stats[1] == data["removed"]
    far = data["points"][data["far"]][0]
    assert np.any(np.all(want == far, axis=1)) and all(np.any(np.all(want == p, axis=1)) for p in data["points"][data["at_max_ray"]])
    fresh, before = build(case)
    assert view.render(data["frame"], fc.NAN_POSE, fc.CULL_SENSOR) == (0, len(data["frame"]))
    assert not np.isfinite(view.depth()).any() and np.isnan(view.info()["sensor_world"]).all()
    got = fresh.RemoveSeenThrough(view)
    print("sweep with a view that sees nothing: %s" % (got,))
    assert got == (0, 0, 0, 0) and np.array_equal(bucket_sorted(fresh.Pointcloud(), vs), before) and fresh.check() == 0
