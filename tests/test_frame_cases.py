"""The premises of tests/frame_cases.py, proved on the CPU with numpy and the restatements alone (tests/grid_ref.py, tests/view_ref.py,
okicp.VoxelHashMap), so that the regime each case of tests/test_gpu_frame_regimes.py claims is a property of its input, and so that
the restatement's answer would differ if the regime were skipped: a walk cut at its first 64 steps, a ray list cut at 8 192 entries,
a window evaluated one size smaller, a pixel without its clamp, a conversion that flushes small floats - and, where those do not
apply, a plane word given to one row, a corner cast without its check, counters summed in 16 bits, a sweep of one trip.

The small cases also go through the stand-alone host programs of tests/test_grid_host.py and tests/test_view_host.py (programs with
their own main, built plainly and under ASan + UBSan), so that grid_host::integrate and view_host::render / classify / sweep - the
text the kernels share - are held to the restatement on them too."""
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from checkers import okicp
from mapdev_ref import bucket_sorted
import frame_cases as fc
import grid_cases as gc
import grid_ref as gr
import view_cases as vc
import view_ref as vr
from test_grid_host import _build as build_grid_host
from test_view_host import _build as build_view_host

SANITIZED = [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]]


def reference(cfg, frames):
    counts = np.zeros((cfg["height"], cfg["width"], 2), dtype=np.uint16)
    stats = [gr.integrate(cfg, counts, pts, pose, sensor) for pts, pose, sensor in frames]
    return counts, stats


def differs(cfg, frames, **wrong):
    """the variant, left alone, IS the restatement; made wrong, it gives other counters"""
    want, want_stats = reference(cfg, frames)
    same, same_stats = fc.run_variant(cfg, frames)
    assert np.array_equal(same, want) and same_stats == want_stats
    got, _ = fc.run_variant(cfg, frames, **wrong)
    return not np.array_equal(got, want)


# ---- grid --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True], ids=["8191x9", "9x8191"])
def test_reach_4095_walks_lie_in_the_grid(transposed):
    cfg, frames, cells = fc.reach_frames(transposed)
    assert cfg["reach"] == fc.MAX_REACH and (cfg["width"], cfg["height"]) == ((9, 8191) if transposed else (8191, 9))
    side = 2 * cfg["reach"] + 1
    assert side * side == 67092481 and -(-side * side // 4) == 16773121 and side * side % 4 == 1  # the last plane word holds one cell
    assert 2 * 4094 * 4095 + 4095 == 33533955 < 2 ** 32
    counts = np.zeros((cfg["height"], cfg["width"], 2), dtype=np.uint16)
    for k, (pts, pose, sensor) in enumerate(frames):
        used, offs, (sx, sy) = gr.endpoints(cfg, pts, pose, sensor)
        assert (int(sx), int(sy)) == cells[k]
        directed = [(dy, dx) if transposed else (dx, dy) for dx, dy in fc.REACH_OFFSETS]
        assert used[:7].all() and not used[7] and offs[:7].tolist() == [list(d) for d in directed[:7]]
        stats = gr.integrate(cfg, counts, pts, pose, sensor)
        print("frame %d: %s, %d distinct endpoint cells" % (k, stats, len(np.unique(offs, axis=0))))
        assert stats[3] >= 8000 and 500 < stats[0] < len(pts) and stats[1] > 500
        if k == 0:  # the walks to (+-4095, 0): 4095 steps, every one inside the grid
            for sign in (1, -1):
                ox, oy = gr.walk(*directed[0 if sign > 0 else 1])
                gx, gy = cells[0][0] + ox, cells[0][1] + oy
                assert len(ox) == 4095 and gx.min() >= 0 and gx.max() < cfg["width"] and gy.min() >= 0 and gy.max() < cfg["height"]
    assert cells[1] == (cells[0][0] + 3, cells[0][1] - 2) and counts[:, :, 1].max() == 2
    assert differs(cfg, frames, max_steps=64)


@pytest.fixture(scope="module")
def big():
    """the large frame's reference, once: (cfg, frames, counters after each of large / 65 points / large, their statistics)"""
    cfg, frames = fc.big_sequence()
    after, stats = gc.reference_run(cfg, frames)
    return cfg, frames, after, stats


def test_the_large_frame_has_more_rays_than_the_ray_kernel_has_waves(big):
    cfg, frames, after, stats = big
    pts, pose, sensor = frames[0]
    used, offs, _ = gr.endpoints(cfg, pts, pose, sensor)
    distinct = len(np.unique(offs, axis=0))
    print("large frame: n = %d, used %d, distinct endpoint cells %d, statistics %s" % (len(pts), used.sum(), distinct, stats))
    assert len(pts) == fc.BIG_N > 524288 and -(-len(pts) // fc.GRID_BLOCK) > fc.GRID_RAY_GROUPS
    assert distinct > fc.GRID_RAY_WAVES == 8192 and cfg["reach"] == 60
    assert stats[0] == stats[2] and stats[0][2] == distinct and stats[0][1] > 100000 and len(frames[1][0]) == 65
    assert after[2].max() < 65535  # nothing saturates: the order of the three frames does not matter
    # this frame is dense - all but 115 of the window's 14 641 cells are endpoints - so its rays add 5 MISS cells and a list cut short
    # would not show; the sparse frame below is the one whose answer depends on the stride
    assert stats[0][3] < 10 and not differs(cfg, frames[:1], max_rays=fc.GRID_RAY_WAVES)


def test_the_sparse_large_frame_needs_every_entry_of_its_ray_list():
    cfg, frame = fc.sparse_big_frame()
    used, offs, (sx, sy) = gr.endpoints(cfg, *frame)
    distinct = np.unique(offs, axis=0)
    counts, stats = reference(cfg, [frame])
    print("sparse large frame: n = %d, distinct endpoint cells %d, statistics %s" % (len(frame[0]), len(distinct), stats[0]))
    assert len(frame[0]) == fc.BIG_N and used.all() and (sx, sy) == (352.0, 350.0) and cfg["reach"] == 300
    assert len(distinct) == fc.SPARSE_CELLS > fc.GRID_RAY_WAVES and np.abs(distinct).max(axis=1).min() >= 200
    assert stats[0][2] == fc.SPARSE_CELLS and stats[0][3] > 20 * fc.SPARSE_CELLS
    assert differs(cfg, [frame], max_rays=fc.GRID_RAY_WAVES) and differs(cfg, [frame], max_steps=64)


def test_far_sensors_use_their_points_and_touch_nothing():
    for name, (pts, pose, sensor, cell) in fc.far_sensors().items():
        used, offs, (sx, sy) = gr.endpoints(fc.CFG16, pts, pose, sensor)
        assert int(sx) == cell and int(sy) == 8 and used.all() and offs.tolist() == [[1, 0], [0, 2]], name
        counts = np.zeros((16, 16, 2), dtype=np.uint16)
        assert gr.integrate(fc.CFG16, counts, pts, pose, sensor) == (2, 0, 0, 0) and not counts.any(), name
        frames = [(pts, pose, sensor)]
        assert differs(fc.CFG16, frames, bare_cast=True) == (name == "wraps_onto_the_grid"), name
    cells = {name: v[3] - fc.CFG16["reach"] for name, v in fc.far_sensors().items()}
    assert cells["corner_2^30"] == 2 ** 30 and cells["corner_2^30+1"] == 2 ** 30 + 1 and cells["corner_-2^30"] == -2 ** 30 == fc.FAR_AWAY
    assert cells["corner_-2^30-1"] == -2 ** 30 - 1 and abs(cells["x_1e15"]) > 2 ** 31 and abs(cells["x_-1e15"]) > 2 ** 31


@pytest.mark.parametrize("reach", [6, 60])
def test_windows_of_endpoints_and_of_rays(reach):
    side = 2 * reach + 1
    cfg, frame = fc.window_frame(reach, "endpoints")
    assert cfg["reach"] == reach and len(frame[0]) == side * side
    counts, stats = reference(cfg, [frame, frame])
    assert stats == [(side * side, 0, side * side, 0)] * 2 and counts[:, :, 1].sum() == 0 and counts[:, :, 0].sum() == 2 * side * side
    cfg, frame = fc.window_frame(reach, "rays")
    counts, stats = reference(cfg, [frame, frame])
    assert stats == [(8 * reach, 0, 8 * reach, (side - 2) ** 2)] * 2  # every interior cell is MISS
    if reach == 60:
        assert side * side // 4 >= 256 and differs(cfg, [frame], max_steps=59)


def test_endpoint_pairs_share_a_plane_word_across_two_rows():
    pairs = fc.shared_word_pairs()
    assert [at % 4 for at, _ in pairs] == [0, 1, 2, 3]
    for at, ((ax, ay), (bx, by)) in pairs:
        first, second = (ay + 6) * 13 + ax + 6, (by + 6) * 13 + bx + 6
        assert (first, second) == (at, at + 1) and by == ay + 1 and (first // 4 == second // 4) == (at % 4 != 3)
        cfg, frame = fc.offsets_frame(6, [(ax, ay), (bx, by)])
        counts, stats = reference(cfg, [frame])
        assert stats[0][:3] == (2, 0, 2) and counts[8 + ay, 8 + ax, 0] == 1 and counts[8 + by, 8 + bx, 0] == 1
        assert differs(cfg, [frame], word_rows=True)  # (the rays' cells straddle rows too)
        assert fc.run_variant(cfg, [frame], word_rows=True)[1][0][2] == (1 if at % 4 != 3 else 2)  # the second endpoint is lost with its word's row
    cfg, frame = fc.offsets_frame(6, [p for _, pair in pairs for p in pair])
    assert reference(cfg, [frame])[1][0][:3] == (8, 0, 8) and differs(cfg, [frame], word_rows=True)


@pytest.mark.parametrize("n", fc.WAVE_EDGES)
def test_short_frames_make_a_ray_per_point(n):
    cfg, frame = fc.own_cell_frame(n)
    used, offs, _ = gr.endpoints(cfg, *frame)
    assert len(frame[0]) == n and used.all() and len(np.unique(offs, axis=0)) == n and np.abs(offs).max(axis=1).min() >= 1
    counts, stats = reference(cfg, [frame, frame])
    assert stats[0] == stats[1] and stats[0][:3] == (n, 0, n) and counts[:, :, 0].sum() == 2 * n
    assert differs(cfg, [frame], max_rays=n - 1)  # the last entry of the list matters


@pytest.mark.parametrize("width,height", fc.READOUT_SHAPES)
def test_readout_at_the_counters_ends(width, height):
    counts = fc.readout_counts(width, height)
    assert counts.shape == (height, width, 2) and width * height in (255, 257)
    flat = counts.reshape(-1, 2).tolist()
    assert flat[:5] == [list(p) for p in fc.END_PAIRS] and flat[-1] == list(fc.END_PAIRS[0])
    seen = counts.astype(np.int64).sum(axis=2)
    assert seen.max() == 131070 and (seen == 65535).any() and (seen == 65536).any()
    for m in fc.MIN_OBSERVATIONS:
        want = gr.occupancy(counts, m)
        assert np.array_equal(K.occupancy_from_counts(counts, m), want)
        known = int((want >= 0).sum())
        print("%d x %d, min_observations %d: %d cells known" % (width, height, m, known))
        assert (known > 0) == (m <= 131070) and want.reshape(-1)[0] == (50 if m <= 131070 else -1)
        if m <= 131070:
            assert not np.array_equal(fc.occupancy_16bit_variant(counts, m), want)


@pytest.fixture(scope="module")
def grid_host_cases():
    cases = [(fc.CFG16, [f[:3]] * 2) for f in fc.far_sensors().values()]
    for reach in (6, 60):
        for which in ("endpoints", "rays"):
            cfg, frame = fc.window_frame(reach, which)
            cases.append((cfg, [frame, frame]))
    pairs = fc.shared_word_pairs()
    cases += [fc.offsets_frame(6, list(pair)) for _, pair in pairs] + [fc.offsets_frame(6, [p for _, pair in pairs for p in pair])]
    cases = [(c[0], c[1] if isinstance(c[1], list) else [c[1]]) for c in cases]
    for n in fc.WAVE_EDGES:
        cfg, frame = fc.own_cell_frame(n)
        cases.append((cfg, [frame, frame]))
    return [(cfg, frames) + tuple(gc.reference_run(cfg, frames)) for cfg, frames in cases]


@pytest.mark.parametrize("flags", SANITIZED, ids=["plain", "asan_ubsan"])
def test_grid_host_program_on_the_small_cases(tmp_path, grid_host_cases, flags):
    """grid_host::integrate (tests/cpp/grid_host_test.cpp, a program of its own) on the far sensors, the full windows, the shared words
    and the short frames; the reach-4095 and the 524 588-point cases are left to the kernels (two planes of 67 MB per frame)"""
    exe = build_grid_host(tmp_path, "grid_host_test", flags)
    for k, (cfg, frames, after, stats) in enumerate(grid_host_cases):
        src, dst = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        gc.write_frames(src, cfg, frames)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (k, (out.stdout + out.stderr)[-2000:])
        assert [tuple(int(v) for v in ln.split()[1:]) for ln in out.stdout.splitlines() if ln.startswith("frame ")] == stats, k
        cells = cfg["width"] * cfg["height"]
        raw = open(dst, "rb").read()
        assert np.array_equal(np.frombuffer(raw[:4 * cells], dtype=np.uint16).reshape(cfg["height"], cfg["width"], 2), after[-1]), k
        assert np.array_equal(np.frombuffer(raw[4 * cells:], dtype=np.int8).reshape(cfg["height"], cfg["width"]), gr.occupancy(after[-1])), k


# ---- depth view ----------------------------------------------------------------------------------------------------------------------
def rendered(case):
    depth, stats, c = vr.render(case["cfg"], case["frame"], case["pose"], case["sensor"])
    return depth, stats, c, vr.verdict(case["cfg"], depth, c, case["queries"])


def smaller_window(case, depth, c):
    return vr.verdict(dict(case["cfg"], window=case["cfg"]["window"] - 1), depth, c, case["queries"])


def test_res_8():
    case, exact = fc.res8_case()
    depth, stats, c, v = rendered(case)
    print("res 8: %s, %d finite pixels, verdicts %s" % (stats, np.isfinite(depth).sum(), np.bincount(v, minlength=4).tolist()))
    assert depth.shape == (6, 8, 8) and stats[1] > 20 and np.isfinite(depth).sum() > 150 and all((v == k).sum() > 20 for k in (0, 2, 3))
    depth, stats, c, v = rendered(exact)
    assert stats == (8, 0) and v.tolist() == [vc.T] * 8 and {tuple(p) for p in np.argwhere(np.isfinite(depth)).tolist()} == {(f, w, u) for f in (0, 1) for w in (0, 7) for u in (0, 7)}
    assert not np.array_equal(fc.render_unclamped_variant(exact["cfg"], exact["frame"], exact["pose"], exact["sensor"]), depth)


@pytest.fixture(scope="module")
def res1024():
    case = fc.res1024_case()
    return (case,) + rendered(case)


def test_res_1024(res1024):
    case, depth, stats, c, v = res1024
    cfg = case["cfg"]
    assert (cfg["res"], cfg["window"], cfg["min_rays"]) == (1024, 4, 81) and len(case["queries"]) == 20000 and len(case["frame"]) > 300000
    print("res 1024: %s, %d finite pixels, verdicts %s" % (stats, np.isfinite(depth).sum(), np.bincount(v, minlength=4).tolist()))
    assert stats[1] > 30000 and np.isfinite(depth).sum() > 200000
    assert (v == 3).sum() > 200 and (v == 2).sum() > 1000 and (v == 0).sum() > 1000
    directed = fc.directed_1024()
    ok, m, face, u, w = vr.project(cfg, np.array([p for p, _ in directed]))
    assert ok.all() and [(int(f), int(a), int(b)) for f, a, b in zip(face, u, w)] == [want for _, want in directed]
    assert {f for _, (f, a, b) in directed if a == 1023 and b == 1023} == set(range(6))
    assert all(np.isfinite(depth[f, b, a]) for _, (f, a, b) in directed)
    assert not np.array_equal(fc.render_unclamped_variant(cfg, case["frame"], case["pose"], case["sensor"]), depth)  # the clamp is needed
    full = dict(cfg, min_rays=1)
    assert not np.array_equal(vr.verdict(full, depth, c, case["queries"]), v)  # min_rays 81 decides: outside the patch no window is full


@pytest.mark.parametrize("name,res,window,min_rays,filled", fc.patch_cases(), ids=[p[0] for p in fc.patch_cases()])
def test_patches_flip_the_verdict_at_min_rays(name, res, window, min_rays, filled):
    case, want = fc.patch_case(res, window, min_rays, filled)
    places = fc.patch_places(res, window)
    sizes = {place: len(fc.window_pixels(res, window, u, w)) for place, (u, w) in places.items()}
    side, clipped = 2 * window + 1, window + 1
    assert sizes["inside"] == side * side and (len(places) == 9 or (res, window) == (16, 4))
    if len(places) == 9:  # clipped on one side at an edge, on two sides in a corner
        assert sizes["edge_left"] == sizes["edge_high"] == side * clipped and sizes["corner_00"] == sizes["corner_11"] == clipped * clipped
    depth, stats, c, v = rendered(case)
    assert stats == (len(case["frame"]), 0) and int(np.isfinite(depth).sum()) == len(case["frame"]) == sum(min(filled, s) for s in sizes.values())
    ok, m, face, u, w = vr.project(case["cfg"], case["queries"])
    assert ok.all() and (face == 0).all() and list(zip(u.tolist(), w.tolist())) == list(places.values())
    assert v.tolist() == want
    if filled == min_rays:
        assert vc.T in want and not np.array_equal(smaller_window(case, depth, c), v)  # one size smaller sees fewer returns
        below, _ = fc.patch_case(res, window, min_rays, filled - 1)
        assert vc.T not in rendered(below)[3].tolist()  # and one return fewer flips every verdict


def test_depths_no_normal_float_holds():
    case, want, pixels = fc.tiny_case()
    depth, stats, c, v = rendered(case)
    assert stats == (5, 0) and v.tolist() == want
    finite = {tuple(p): depth[tuple(p)] for p in np.argwhere(np.isfinite(depth)).tolist()}
    assert finite.keys() == pixels.keys() and all(finite[k].tobytes() == pixels[k].tobytes() for k in pixels)
    assert depth[1, 8, 8].view(np.uint32) == 71362 and depth[2, 8, 8].view(np.uint32) == 0  # a denormal; +0.0
    first = dict(case, frame=case["frame"][:3])
    d3, s3, _, _ = rendered(first)
    assert s3 == (3, 0) and np.isfinite(d3).sum() == 2
    flushed = fc.flushed_variant(depth)
    assert not np.array_equal(vr.verdict(case["cfg"], flushed, c, case["queries"]), v)


def test_edge_counts_and_the_contended_pixel():
    cfg, pose, sensor, frame, queries = fc.edge_points()
    assert len(frame) == max(fc.WAVE_EDGES) and len(queries) == 70000
    depth, stats, c = vr.render(cfg, frame, pose, sensor)
    assert stats[0] > 150 and stats[1] > 10
    v = vr.verdict(cfg, depth, c, queries)
    assert all((v[:n] == k).any() for n in (3, 5000, 70000) for k in ((2,) if n == 3 else (0, 2, 3)))
    one = vr.make_config(16, 0, 1, 10.0, 0.25, 0.0)
    for first in (True, False):
        pts = fc.contended_frame(first)
        assert len(pts) == 200000 and -(-len(pts) // fc.VIEW_BLOCK) == 782 and pts[:, 0].min() == fc.CONTENDED_MIN == pts[0 if first else -1, 0]
        depth, stats, _ = vr.render(one, pts, vc.IDENTITY, vc.ORIGIN)
        assert stats == (200000, 0) and np.isfinite(depth).sum() == 1 and depth[0, 8, 8] == np.float32(fc.CONTENDED_MIN)


@pytest.fixture(scope="module")
def wall():
    depth, stats, c = vr.render(vc.WALL_CFG, vc.wall(), vc.IDENTITY, vc.ORIGIN)
    return depth, c


@pytest.mark.parametrize("name", fc.BUCKET_PATTERNS)
def test_buckets_at_the_trip_edges(name, wall):
    case = fc.bucket_sweep_cases()[name]
    depth, c = wall
    omap = okicp.VoxelHashMap(1.0, 100.0, fc.CAP128)
    omap.AddPoints(case["points"])
    assert omap.num_points() == len(case["points"]) == sum(fc.BUCKET_LENGTHS)  # every point was accepted, in insertion order
    before = bucket_sorted(omap.Pointcloud(), 1.0)
    held = np.unique(np.floor(before), axis=0, return_counts=True)[1]
    assert sorted(held.tolist()) == fc.BUCKET_LENGTHS
    v = vr.verdict(vc.WALL_CFG, depth, c, case["points"])
    assert np.array_equal((v & vr.SEEN_THROUGH) != 0, case["pattern"]) and (v & vr.IN_RANGE).all()
    keep, stats = vr.sweep(vc.WALL_CFG, depth, c, before, 1.0)
    gone = int(case["pattern"].sum())
    assert stats == (len(before), gone, 0 if name == "none" else 5, 0) and gone == {"all_but_last": sum(fc.BUCKET_LENGTHS) - 5, "none": 0}.get(name, 5)
    one_trip = fc.one_trip_variant(vc.WALL_CFG, depth, c, before, 1.0)
    assert np.array_equal(one_trip, keep) == (name in ("only_first", "none"))


@pytest.mark.parametrize("name", ["centre", "all", "face"])
def test_block_cases_erase_what_they_claim(name):
    case = fc.block_cases()[name]
    omap = okicp.VoxelHashMap(case["vs"], 100.0, case["cap"])
    omap.AddPoints(case["points"])
    assert omap.num_points() == len(case["points"])
    before = bucket_sorted(omap.Pointcloud(), case["vs"])
    voxels = np.unique(np.floor(before), axis=0)
    assert len(voxels) == 27 and (voxels.max(axis=0) - voxels.min(axis=0)).tolist() == [2, 2, 2]
    depth, _, c = vr.render(case["cfg"], case["frame"], vc.IDENTITY, vc.ORIGIN)
    keep, stats = vr.sweep(case["cfg"], depth, c, before, case["vs"])
    print("%s: %s" % (name, stats))
    assert stats[3] == case["erased"] == stats[2] and stats[0] == len(before)
    if name == "centre":
        assert np.isfinite(depth).sum() == 1 and np.isfinite(depth[0, 32, 32])
        assert np.array_equal(np.unique(np.floor(before[~keep]), axis=0), [[10.0, 0.0, 0.0]]) and stats[1] == 4  # every neighbour keeps every point
    elif name == "face":
        assert (np.floor(before[~keep])[:, 0] == 9.0).all() and stats[1] == 27


@pytest.mark.parametrize("vs", [1.0, 0.3])
def test_points_at_exactly_max_ray_are_in_range(vs):
    case = fc.cull_case()
    cfg, c = fc.CULL_CFG, fc.CULL_SENSOR
    assert np.all(np.floor(c / vs) * vs != c)  # off the lattice
    m = np.abs(case["points"] - c).max(axis=1)
    assert (m[case["at_max_ray"]] == cfg["max_ray"]).all() and (m[case["beyond"]] > cfg["max_ray"]).all() and (m[case["beyond"]] < cfg["max_ray"] + 1e-9).all()
    far = case["points"][case["far"]][0]
    box = np.floor(far / vs) * vs
    assert np.maximum(box - c, c - (box + vs)).max() > cfg["max_ray"] + 0.002 * vs  # that voxel's box lies wholly beyond
    depth, _, cw = vr.render(cfg, case["frame"], vc.IDENTITY, c)
    assert np.array_equal(cw, c)
    v = vr.verdict(cfg, depth, cw, case["points"])
    assert (v[case["at_max_ray"]] == vc.K).all() and (v[case["beyond"]] == vc.O).all() and v[case["far"]][0] == vc.O and (v == vc.T).sum() == case["removed"]
    keep, stats = vr.sweep(cfg, depth, cw, bucket_sorted(case["points"], vs), vs)
    assert stats[0] == 6 + case["removed"] and stats[1] == case["removed"]
    blind, bstats, bc = vr.render(cfg, case["frame"], fc.NAN_POSE, c)
    assert bstats == (0, len(case["frame"])) and np.isnan(bc).all() and vr.sweep(cfg, blind, bc, case["points"], vs)[1] == (0, 0, 0, 0)


@pytest.fixture(scope="module")
def view_host_cases():
    """(cfg, vs, cap, map points, frame, pose, sensor, queries) per case small enough for the host program"""
    rng = np.random.default_rng(18)
    cases = []

    def add(case, map_points=None, vs=0.5, cap=20):
        pts = case["queries"][np.all(np.abs(case["queries"]) < 50.0, axis=1)] if map_points is None else map_points
        cases.append((case["cfg"], vs, cap, pts, case["frame"], case["pose"], case["sensor"], case["queries"]))

    for case in fc.res8_case():
        add(case)
    add(fc.tiny_case()[0], map_points=rng.uniform(-3, 3, (50, 3)))
    for name, res, window, min_rays, filled in fc.patch_cases():
        add(fc.patch_case(res, window, min_rays, filled)[0])
    cfg, pose, sensor, frame, queries = fc.edge_points()
    for n in fc.WAVE_EDGES:
        add(fc.view_case(cfg, frame[:n], queries[:n], pose, sensor))
    for case in fc.bucket_sweep_cases().values():
        cases.append((vc.WALL_CFG, case["vs"], case["cap"], case["points"], vc.wall(), vc.IDENTITY, vc.ORIGIN, case["points"]))
    for case in fc.block_cases().values():
        cases.append((case["cfg"], case["vs"], case["cap"], case["points"], case["frame"], vc.IDENTITY, vc.ORIGIN, case["points"]))
    cull = fc.cull_case()
    for vs in (1.0, 0.3):
        cases.append((fc.CULL_CFG, vs, 20, cull["points"], cull["frame"], vc.IDENTITY, fc.CULL_SENSOR, cull["points"]))
        cases.append((fc.CULL_CFG, vs, 20, cull["points"], cull["frame"], fc.NAN_POSE, fc.CULL_SENSOR, cull["points"]))
    return cases


@pytest.mark.parametrize("flags", SANITIZED, ids=["plain", "asan_ubsan"])
def test_view_host_program_on_the_small_cases(tmp_path, view_host_cases, flags):
    """view_host::render / classify / sweep (tests/cpp/view_host_test.cpp, a program of its own) on every case but the res-1024 image,
    the 70 000 queries and the contended pixel, which are left to the kernels"""
    exe = build_view_host(tmp_path, "view_host_test", flags)
    erased = 0
    for k, (cfg, vs, cap, map_points, frame, pose, sensor, queries) in enumerate(view_host_cases):
        src, dst = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        vc.write_host_case(src, cfg, vs, 100.0, cap, map_points, frame, pose, sensor, queries)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (k, (out.stdout + out.stderr)[-2000:])
        lines = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out.stdout.splitlines()}
        omap = okicp.VoxelHashMap(vs, 100.0, cap)
        omap.AddPoints(map_points)
        before = bucket_sorted(omap.Pointcloud(), vs)
        depth, rstats, c = vr.render(cfg, frame, pose, sensor)
        keep, sstats = vr.sweep(cfg, depth, c, before, vs)
        assert lines["render"] == rstats and lines["sweep"] == sstats and lines["check"] == (0, 0), k
        res = cfg["res"]
        raw = open(dst, "rb").read()
        at = 24 * res * res
        assert np.frombuffer(raw[:at], dtype=np.uint32).tobytes() == depth.tobytes(), k  # bit for bit: -0.0 or a flushed denormal would show
        assert np.array_equal(np.frombuffer(raw[at:at + len(queries)], dtype=np.uint8), vr.verdict(cfg, depth, c, queries)), k
        cloud = np.frombuffer(raw[at + len(queries):], dtype=np.float64).reshape(-1, 3)
        assert np.array_equal(bucket_sorted(cloud, vs), before[keep]), k
        erased += sstats[3]
    assert erased >= 1 + 27 + 9
