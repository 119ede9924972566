"""Inputs shared by the depth view's tests (tests/test_view_host.py on the CPU, tests/test_gpu_view.py and tests/test_gpu_view_map.py on
the GPU): hand-built frames and queries with their expected verdicts written out, maps built to lose chosen points, and the pinned
8-frame drive with a person walking through - so that the stand-alone host program and the kernels are held to the restatement
(tests/view_ref.py) on the same data."""
import numpy as np

import view_ref as vr
from kinematic_icp_amd import synthetic as syn

IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
ORIGIN = np.zeros(3)
T, K, O = 3, 2, 0  # a verdict: seen Through (and in range), Kept in range, Out of range


def _case(cfg, frame, queries, pose=IDENTITY, sensor=ORIGIN, verdicts=None, pixels=None, stats=None):
    """verdicts: the expected byte per query, written out by hand; pixels: {(face, w_, u): depth} - every other pixel is empty;
    stats: (used, skipped)"""
    return dict(cfg=cfg, frame=np.asarray(frame, dtype=np.float64).reshape(-1, 3), queries=np.asarray(queries, dtype=np.float64).reshape(-1, 3),
                pose=np.asarray(pose, dtype=np.float64), sensor=np.asarray(sensor, dtype=np.float64), verdicts=verdicts, pixels=pixels, stats=stats)


def unit_cases():
    """name -> case; res 16, so a pixel is 1/8 wide in a / m"""
    cases = {}
    one = vr.make_config(16, 0, 1, 10.0, 0.25, 0.0)
    nan, inf = np.nan, np.inf
    # one point per face and sign; (a, b) = (1, 2) / 5 -> u = floor(1.2 * 8) = 9, w_ = floor(1.4 * 8) = 11.  Queries at half the depth
    # are seen through, at 1.5 times the depth (still within max_ray) kept
    faces = np.array([[5, 1, 2], [-5, 1, 2], [1, 5, 2], [1, -5, 2], [1, 2, 5], [1, 2, -5]], dtype=np.float64)
    cases["faces"] = _case(one, faces, np.concatenate([0.5 * faces, 1.5 * faces]), verdicts=[T] * 6 + [K] * 6, stats=(6, 0),
                           pixels={(f, 11, 9): 5.0 for f in range(6)})
    # ties go to the first axis in the order x, y, z: |vx| == |vy| to x, |vy| == |vz| to y; the sign is that component's
    ties = np.array([[3, 3, 1], [3, -3, 3], [-2, 2, 2], [1, 4, -4], [-1, -4, 4]], dtype=np.float64)
    cases["ties"] = _case(one, ties, 0.5 * ties, verdicts=[T] * 5, stats=(5, 0),
                          pixels={(0, 10, 15): 3.0, (0, 15, 0): 3.0, (1, 15, 15): 2.0, (2, 0, 10): 4.0, (3, 15, 6): 4.0})
    # a / m == +1 lands in pixel res - 1 (the clamp), == -1 in pixel 0; a pixel border hit exactly: a / m = 0.25 -> 1.25 * 8 = 10.0
    clamp = np.array([[4, 4, 0], [4, -4, -4], [8, 2, -2]], dtype=np.float64)
    cases["clamp_and_border"] = _case(one, clamp, 0.5 * clamp, verdicts=[T] * 3, stats=(3, 0), pixels={(0, 8, 15): 4.0, (0, 0, 0): 4.0, (0, 6, 10): 8.0})
    # a point at the sensor (m == 0), exactly at max_ray (used) and one ulp beyond (skipped); the same three as queries
    sensor = np.array([0.5, -0.25, 0.125])
    edge = np.array([[0.5, -0.25, 0.125], [10.5, -0.25, 0.125], [10.500000000000002, -0.25, 0.125]])
    cases["range_edges"] = _case(one, edge, edge, sensor=sensor, verdicts=[O, K, O], stats=(1, 2), pixels={(0, 8, 8): 10.0})
    # coordinates that are not finite are skipped; so is a point whose world coordinate overflows
    bad = np.array([[nan, 1, 1], [1, inf, 1], [1, 1, -inf], [1.7e308, 0, 0], [2, 0, 0]], dtype=np.float64)
    cases["not_finite_points"] = _case(one, bad, [[1, 0, 0], [nan, 0, 0], [inf, 0, 0]], pose=np.array([0, 0, 0, 1, 1.7e308, 0, 0]), sensor=ORIGIN,
                                       verdicts=[O, O, O], stats=(0, 5), pixels={})
    cases["not_finite_pose"] = _case(one, [[2, 0, 0]], [[1, 0, 0]], pose=np.array([0, 0, 0, 1, nan, 0, 0]), verdicts=[O], stats=(0, 1), pixels={})
    cases["not_finite_sensor"] = _case(one, [[2, 0, 0]], [[1, 0, 0]], sensor=np.array([0, inf, 0]), verdicts=[O], stats=(0, 1), pixels={})
    # two points in one pixel: the nearer wins, whatever their order
    cases["min_wins"] = _case(one, [[7, 0.14, 0.14], [5, 0.1, 0.1], [6, 0.12, 0.12]], [[5.5, 0.11, 0.11], [4.5, 0.09, 0.09]], verdicts=[K, T], stats=(3, 0),
                              pixels={(0, 8, 8): 5.0})
    # a depth float cannot hold: (float)10.000000001 == 10.0f.  With both margins zero a query at 10.0000000005 lies in front of the return
    # in fp64, but not in front of the pixel: kept.  10 - 1e-9 is seen through
    exact = vr.make_config(16, 0, 1, 20.0, 0.0, 0.0)
    cases["float_depth_decides"] = _case(exact, [[10.000000001, 0.1, 0.1]], [[10.0000000005, 0.1, 0.1], [9.999999999, 0.1, 0.1], [10.0, 0.1, 0.1]],
                                         verdicts=[K, T, K], stats=(1, 0), pixels={(0, 8, 8): 10.0})
    # m + margin == D exactly is kept (strict <): 7.75 + 0.25 == 8
    cases["margin_exact"] = _case(one, [[8, 0.1, 0.1]], [[7.75, 0.1, 0.1], [7.749999999999999, 0.1, 0.1]], verdicts=[K, T], stats=(1, 0), pixels={(0, 8, 8): 8.0})
    # N == min_rays - 1 against N == min_rays: window 1, min_rays 3; pixels (8, 8), (9, 8), (10, 9) of face 0 hold returns.  A query in
    # pixel (9, 9) sees all three, one in pixel (7, 8) only the first two
    three = vr.make_config(16, 1, 3, 10.0, 0.25, 0.0)
    rays = [[8, 0.5, 0.5], [8, 1.5, 0.5], [8, 2.5, 1.5]]
    cases["min_rays"] = _case(three, rays, [[4, 0.75, 0.75], [4, -0.25, 0.25]], verdicts=[T, K], stats=(3, 0),
                              pixels={(0, 8, 8): 8.0, (0, 8, 9): 8.0, (0, 9, 10): 8.0})
    # The window is clipped at the face's edge and corner.  The only returns lie on the +y face right across the edge / the corner from
    # the query's pixel on the +x face: nothing is seen there (N = 0), the query is kept; a return in the query's own face, inside
    # the window, sees through it
    wide = vr.make_config(16, 2, 1, 10.0, 0.25, 0.0)
    cases["window_clipped"] = _case(wide, [[7.9, 8, 0.5], [7.9, 8, 7.9], [8, -7.5, 7.5]], [[4, 3.9, 0.25], [4, 3.9, 3.9], [4, -3.9, 3.9]], verdicts=[K, K, T],
                                    stats=(3, 0), pixels={(2, 8, 15): 8.0, (2, 15, 15): 8.0, (0, 15, 0): 8.0})
    # an empty image, and a face without returns
    cases["empty_image"] = _case(wide, np.zeros((0, 3)), [[4, 0, 0], [0, 0, -3], [11, 0, 0]], verdicts=[K, K, O], stats=(0, 0), pixels={})
    cases["face_without_returns"] = _case(wide, [[8, 0, 0]], [[-4, 0, 0], [0, 4, 0], [4, 0, 0]], verdicts=[K, K, T], stats=(1, 0), pixels={(0, 8, 8): 8.0})
    # 4 096 points in three pixels: more than one wave contends for each
    rng = np.random.default_rng(5)
    d = rng.uniform(3.0, 9.0, 4096)
    dirs = np.array([[1, 0.05, 0.05], [0.05, -1, 0.05], [0.3, 0.3, 1]])[rng.integers(0, 3, 4096)]
    cases["contended"] = _case(one, d[:, None] * dirs, [[1, 0.05, 0.05], [0.4, -8, 0.4], [2.7, 2.7, 9]], stats=(4096, 0))
    # a tilted pose and a sensor off the base origin; random points, some beyond max_ray
    pose = np.concatenate([_unit([0.03, -0.05, 0.6, 0.8]), [2.5, -1.25, 0.3]])
    pts = rng.uniform(-9, 9, (500, 3))
    cases["tilted"] = _case(vr.make_config(32, 1, 2, 8.0, 0.1, 0.02), pts, rng.uniform(-7, 7, (400, 3)) + pose[4:], pose=pose, sensor=np.array([0.2, 0.0, 0.5]))
    return cases


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


# ---- maps built to lose chosen points ---------------------------------------------------------------------------------------------
# The frame is a wall: the plane x = 10.5 over |y|, |z| <= 3 every 0.05 m, seen from the origin at the identity pose.  Every pixel it covers
# holds exactly 10.5, so with margins 0.2 + 0.02 m a map point at depth x (|y|, |z| < x) is seen through iff x + 0.2 + 0.02 x < 10.5,
# i.e. x < 10.098: x = 10.02 goes, x >= 10.3 stays.  Voxels are 1 m: voxel (10, j, k) straddles that line.
WALL_CFG = vr.make_config(64, 1, 2, 30.0, 0.2, 0.02)
GONE_X, KEPT_X = 10.02, (10.3, 10.42, 10.6, 10.8)


def wall():
    g = np.arange(-60, 61) * 0.05
    y, z = np.meshgrid(g, g, indexing="ij")
    return np.stack([np.full(y.size, 10.5), y.ravel(), z.ravel()], axis=1)


def lattice(cap, vs=1.0):
    """offsets in [0, vs)^2 farther apart than the map's resolution vs / sqrt(cap): AddPoints accepts them all in one voxel"""
    step = 1.03 * vs / np.sqrt(cap)
    g = 0.02 + step * np.arange(int((0.96 * vs) / step) + 1)
    y, z = np.meshgrid(g, g, indexing="ij")
    return np.stack([y.ravel(), z.ravel()], axis=1)


def bucket(pattern, j=0, k=0, cap=20):
    """one voxel (10, j, k): point i is seen through where pattern[i], else kept; in insertion order"""
    lat = lattice(cap)
    kept_layers = [x for x in KEPT_X]
    pts, used = [], {}
    for i, gone in enumerate(pattern):
        layer = GONE_X if gone else kept_layers[0]
        n = used.get(layer, 0)
        if n >= len(lat):  # the layer is full: the next kept layer
            kept_layers.pop(0)
            layer, n = kept_layers[0], used.get(kept_layers[0], 0)
        used[layer] = n + 1
        pts.append([layer, j + lat[n, 0], k + lat[n, 1]])
    return np.array(pts)


def sweep_cases():
    """name -> dict(vs, cap, points (insertion order), pattern (True: seen through))"""
    cases = {}

    def add(name, cap, parts, extra=None):
        pts = np.concatenate([p for p, _ in parts] + ([extra] if extra is not None else []))
        pat = np.concatenate([np.asarray(g, dtype=bool) for _, g in parts] + ([np.zeros(len(extra), dtype=bool)] if extra is not None else []))
        cases[name] = dict(vs=1.0, cap=cap, points=pts, pattern=pat)

    def part(pattern, j, k, cap=20):
        return bucket(pattern, j, k, cap), pattern

    five = [False] * 5
    add("first_middle_last", 20, [part([True] + five[1:], 0, 0), part(five[:2] + [True] + five[3:], 1, 0), part(five[:4] + [True], -1, 0), part(five, 0, 1)])
    # a full bucket loses everything: the voxel is erased, its neighbours (kept points, and one out of range at x = 40) stay
    add("full_bucket_erased", 20, [part([True] * 20, 0, 0), part(five, 1, 0), part(five, 0, -1), part([True, False, True], -1, -1)],
        extra=np.array([[40.5, 0.5, 0.5], [-5.0, 0.2, 0.2], [11.5, 0.5, 0.5]]))
    alt = [(i % 2) == 0 for i in range(150)]
    add("cap150_alternating", 150, [part(alt, 0, 0, 150), part([not g for g in alt[:130]], 0, 1, 150), part([True] * 70, 1, 1, 150)])
    add("cap300_count_bits", 300, [part([(i % 3) == 0 for i in range(300)], 0, 0, 300), part([True] * 257, 1, 0, 300)])
    return cases


# ---- the pinned drive ---------------------------------------------------------------------------------------------------------------
DRIVE_CFG = vr.make_config(128, 2, 2, 60.0, 0.2, 0.02)
DRIVE_VS, DRIVE_CAP, DRIVE_MAX_RANGE = 0.5, 20, 100.0
PERSON_RADIUS, PERSON_HEIGHT, PERSON_POINTS = 0.25, 1.7, 150


def drive():
    """cfg1's scene, 8 poses 0.5 m apart, 20 x 1000 beams, and a person (a cylinder) who crosses the aisle 3.5 m ahead, 0.8 m per frame: the
    beams the cylinder blocks are dropped, 150 points on its sensor-facing half are added.
    -> list of dict(frame (base frame), pose, sensor (base frame), person (world points of this frame's person))"""
    cfg = syn.CONFIGS["cfg1"]
    rng = np.random.Generator(np.random.PCG64(cfg.seed))
    scene = syn.make_scene(rng, **cfg.scene_kw)
    dirs = syn.beam_directions(20, 1000, cfg.elev_deg)
    sensor = np.array([0.0, 0.0, cfg.sensor_height])
    frames = []
    for k in range(8):
        pose = syn.planar_pose(-3.0 + 0.5 * k, 0.2, np.deg2rad(2.0 * k - 5.0))
        scan = syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng)
        centre = np.array([pose[4] + 3.5, -2.8 + 0.8 * k])
        c = vr.sensor_world(pose, sensor)
        world = vr.transform(pose, scan)
        # beams blocked by the cylinder: the ray passes within its radius in the plane, nearer than the return, below its top there
        v = world - c
        t = ((centre[0] - c[0]) * v[:, 0] + (centre[1] - c[1]) * v[:, 1]) / (v[:, 0] ** 2 + v[:, 1] ** 2)
        foot = c[:2] + t[:, None] * v[:, :2]
        blocked = (t > 0) & (t < 1) & (np.linalg.norm(foot - centre, axis=1) < PERSON_RADIUS) & (c[2] + t * v[:, 2] < PERSON_HEIGHT)
        towards = np.arctan2(c[1] - centre[1], c[0] - centre[0])
        ang = towards + rng.uniform(-1.3, 1.3, PERSON_POINTS)
        person = np.stack([centre[0] + PERSON_RADIUS * np.cos(ang), centre[1] + PERSON_RADIUS * np.sin(ang), rng.uniform(0.05, PERSON_HEIGHT, PERSON_POINTS)], axis=1)
        person_base = vr.transform(syn.pose_inverse(pose), person)
        frame = np.ascontiguousarray(np.concatenate([scan[~blocked], person_base]))
        # the person's points as the map files them: through the same transform the map update applies
        frames.append(dict(frame=frame, pose=pose, sensor=sensor, person=vr.transform(pose, person_base), n_scan=int((~blocked).sum())))
    return frames


def person_count(cloud, frames, which):
    """how many of the cloud's points are person points of the frames `which`"""
    if len(cloud) == 0:
        return 0
    rows = {r.tobytes() for k in which for r in frames[k]["person"]}
    return sum(1 for r in np.ascontiguousarray(cloud) if r.tobytes() in rows)


_DRIVE = {}


def reference_drive():
    """The drive by the restatement over okicp.VoxelHashMap, frame by frame: render, sweep, Update - computed once per process.
    -> dict(frames, steps = per frame dict(depth, c, render_stats, sweep_stats, after_sweep, after_update), final (the map after the last
    Update, bucket-sorted), plain (the same drive without the sweep), self_keep (keep mask of `final` swept with the LAST frame's own view))"""
    if _DRIVE:
        return _DRIVE
    from checkers import okicp
    from mapdev_ref import bucket_sorted
    frames = drive()
    vs = DRIVE_VS
    cloud, plain = np.zeros((0, 3)), okicp.VoxelHashMap(vs, DRIVE_MAX_RANGE, DRIVE_CAP)
    steps = []
    for fr in frames:
        depth, rstats, c = vr.render(DRIVE_CFG, fr["frame"], fr["pose"], fr["sensor"])
        keep, sstats = vr.sweep(DRIVE_CFG, depth, c, cloud, vs)
        after_sweep = cloud[keep]
        omap = okicp.VoxelHashMap(vs, DRIVE_MAX_RANGE, DRIVE_CAP)  # rebuilt from the survivors: every bucket's order is kept
        omap.AddPoints(after_sweep)
        assert omap.num_points() == len(after_sweep)
        omap.Update(fr["frame"], fr["pose"])
        plain.Update(fr["frame"], fr["pose"])
        removed = cloud[~keep]
        cloud = bucket_sorted(omap.Pointcloud(), vs)
        steps.append(dict(depth=depth, c=c, render_stats=rstats, sweep_stats=sstats, after_sweep=after_sweep, after_update=cloud, removed=removed))
    self_keep, _ = vr.sweep(DRIVE_CFG, steps[-1]["depth"], steps[-1]["c"], cloud, vs)
    _DRIVE.update(frames=frames, steps=steps, final=cloud, plain=bucket_sorted(plain.Pointcloud(), vs), self_keep=self_keep)
    return _DRIVE


def write_host_case(path, cfg, vs, max_distance, cap, map_points, frame, pose, sensor, queries):
    """the input file of tests/cpp/view_host_test.cpp"""
    with open(path, "wb") as f:
        np.array([cfg["res"], cfg["window"], cfg["min_rays"], cfg["max_ray"], cfg["margin"], cfg["margin_per_metre"], vs, max_distance, cap, len(map_points),
                  len(frame), len(queries)], dtype=np.float64).tofile(f)
        np.concatenate([np.asarray(pose, dtype=np.float64), np.asarray(sensor, dtype=np.float64)]).tofile(f)
        for a in (map_points, frame, queries):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
