"""The 2-D occupancy grid on the GPU (kicp_grid_*: K.OccupancyGrid) against the numpy restatement of include/kicp.h's semantics
(tests/grid_ref.py).  Everything is exact: after EVERY frame the counters and the four frame statistics must be np.array_equal to
the restatement's - no tolerance anywhere."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import grid_cases as gc
import grid_ref as gr
from kinematic_icp_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def make_grid(cfg):
    return K.OccupancyGrid(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_min"], cfg["z_max"], cfg["max_ray"])


def check_frames(cfg, frames, grid=None, start=None, device=False):
    """integrate `frames` one by one; after each the counters and the statistics equal the restatement's -> (grid, counts)"""
    grid = grid or make_grid(cfg)
    want = np.zeros((cfg["height"], cfg["width"], 2), dtype=np.uint16) if start is None else start.copy()
    for pts, pose, sensor in frames:
        stats = gr.integrate(cfg, want, pts, pose, sensor)
        got = grid.integrate_device(K.DeviceFrame(pts), pose, sensor) if device else grid.integrate(pts, pose, sensor)
        print("frame: n = %d, restatement %s, device %s" % (len(pts), stats, got))
        assert got == stats and grid.last_frame() == stats
        assert np.array_equal(grid.counts(), want)
    return grid, want


# a 16 x 16 grid of 0.25 m cells (exact in binary) from (-2, -2); the sensor in cell (8, 8); reach = ceil(1.5 / 0.25) = 6 cells
CFG16 = gr.make_config(0.25, -2.0, -2.0, 16, 16, -1.0, 1.0, 1.5)
SENSOR16 = np.array([0.1, 0.1, 0.0])
ONE_POINT = {
    "octant_0": (1.3, 0.6), "octant_1": (0.6, 1.3), "octant_2": (-0.6, 1.3), "octant_3": (-1.3, 0.6), "octant_4": (-1.3, -0.6), "octant_5": (-0.6, -1.3),
    "octant_6": (0.6, -1.3), "octant_7": (1.3, -0.6), "axis_px": (1.4, 0.1), "axis_nx": (-1.2, 0.1), "axis_py": (0.1, 1.4), "axis_ny": (0.1, -1.2),
    "diagonal": (1.1, 1.1), "own_cell": (0.2, 0.05), "on_a_cell_border": (0.75, -0.5), "at_reach": (1.6, 0.3), "beyond_reach": (1.85, 0.3),
}


@pytest.mark.parametrize("name", sorted(ONE_POINT))
def test_one_point(name):
    x, y = ONE_POINT[name]
    pts = np.array([[x, y, 0.2]])
    used, offs, (sx, sy) = gr.endpoints(CFG16, pts, gc.IDENTITY, SENSOR16)
    assert (sx, sy) == (8.0, 8.0) and CFG16["reach"] == 6
    if name == "beyond_reach":
        assert not used[0]  # 7 cells away: no hit, no ray
    else:
        assert used[0]
        m = int(np.abs(offs[0]).max())
        assert m == {"own_cell": 0, "at_reach": 6}.get(name, m)
        if name == "on_a_cell_border":
            assert offs[0].tolist() == [3, -2]  # 0.75 / 0.25 is exactly 11 - 8; -0.5 exactly 6 - 8: the border belongs to the upper cell
    grid, counts = check_frames(CFG16, [(pts, gc.IDENTITY, SENSOR16)])
    assert counts[:, :, 0].sum() == (0 if name == "beyond_reach" else 1)


def test_rays_that_leave_enter_cross_and_miss_the_grid():
    # 33 x 17 cells of 0.25 m from (0, 0): 8.25 m x 4.25 m; reach 48 cells
    cfg = gr.make_config(0.25, 0.0, 0.0, 33, 17, -1.0, 1.0, 12.0)
    cases = {
        "sensor_inside_endpoints_outside": (np.array([4.1, 2.1, 0.0]), [[9.3, 3.0, 0], [-1.2, 2.2, 0], [4.0, 6.6, 0], [3.3, -2.0, 0], [11.0, 7.0, 0]]),
        "sensor_outside_endpoints_inside": (np.array([-2.1, -1.3, 0.0]), [[1.0, 1.0, 0], [8.1, 4.1, 0], [4.4, 0.1, 0]]),
        "both_outside_ray_crosses": (np.array([-1.1, 2.1, 0.0]), [[8.9, 2.6, 0], [3.0, -0.6, 0], [2.0, 5.1, 0]]),
        "both_outside_ray_misses": (np.array([-1.1, -0.6, 0.0]), [[-0.4, 4.9, 0], [7.0, -0.9, 0], [-3.0, -3.0, 0]]),
    }
    for name, (sensor, pts) in cases.items():
        grid, counts = check_frames(cfg, [(np.array(pts, dtype=np.float64), gc.IDENTITY, sensor)])
        if name == "both_outside_ray_misses":
            assert not counts.any() and grid.last_frame() == (3, 0, 0, 0)
        elif name == "both_outside_ray_crosses":
            assert counts[:, :, 0].sum() == 0 and counts[:, :, 1].sum() > 20
        elif name == "sensor_inside_endpoints_outside":
            assert counts[:, :, 0].sum() == 0 and counts[:, :, 1].sum() > 20
        else:
            assert counts[:, :, 0].sum() == 3 and grid.last_frame()[3] > 10


def test_many_points_in_three_cells_count_once_per_frame():
    rng = np.random.default_rng(5)
    cells = np.array([[1.0, 0.5], [-0.75, 1.0], [0.25, -1.25]])  # lower corners of three cells of CFG16
    pts = np.concatenate([cells[rng.integers(0, 3, 4096)] + rng.uniform(0.01, 0.24, (4096, 2)), rng.uniform(-0.9, 0.9, (4096, 1))], axis=1)
    frames = [(pts, gc.IDENTITY, SENSOR16)] * 5
    grid, counts = check_frames(CFG16, frames[:1])
    assert sorted(counts[:, :, 0][counts[:, :, 0] > 0].tolist()) == [1, 1, 1] and grid.last_frame()[:3] == (4096, 0, 3)
    grid, counts = check_frames(CFG16, frames[1:], grid, counts)
    assert sorted(counts[:, :, 0][counts[:, :, 0] > 0].tolist()) == [5, 5, 5]
    assert grid.info()["frames"] == 5


def test_a_ray_through_another_endpoint_is_a_hit_there():
    pts = np.array([[0.6, 0.1, 0.0], [1.3, 0.1, 0.0]])  # both along +x from the sensor: the far point's ray crosses the near point's cell
    grid, counts = check_frames(CFG16, [(pts, gc.IDENTITY, SENSOR16)])
    assert counts[8, 10].tolist() == [1, 0] and counts[8, 13].tolist() == [1, 0] and counts[8, 9].tolist() == [0, 1]


def test_skipped_points():
    cfg = gr.make_config(0.25, -2.0, -2.0, 16, 16, 0.0, 0.5, 1.5)
    pts = np.array([[0.6, 0.6, -0.001], [0.6, 0.6, 0.6], [0.9, 0.2, 0.0], [0.2, 0.9, 0.5], [np.nan, 0.3, 0.1], [0.3, np.inf, 0.1], [0.3, 0.3, -np.inf],
                    [0.3, 0.3, np.nan], [-0.7, -0.4, 0.25], [1.0e300, 0.0, 0.1], [5.0, 5.0, 0.1]])
    grid, counts = check_frames(cfg, [(pts, gc.IDENTITY, SENSOR16)])
    assert grid.last_frame()[:2] == (2, 9)  # p.z == z_min is used, p.z == z_max is not
    assert counts[8, 11, 0] == 1 and counts[11, 8, 0] == 0 and counts[6, 5, 0] == 1
    before = grid.counts()
    assert grid.integrate(np.zeros((0, 3)), gc.IDENTITY, SENSOR16) == (0, 0, 0, 0)  # n == 0: nothing changes, the frame is counted
    assert np.array_equal(grid.counts(), before) and grid.info()["frames"] == 2
    nan_pose = np.array([0.0, 0.0, 0.0, 1.0, np.nan, 0.0, 0.0])
    check_frames(cfg, [(pts, nan_pose, SENSOR16), (pts, gc.IDENTITY, np.array([np.nan, 0.0, 0.0]))], grid, before)
    assert grid.last_frame() == (0, 11, 0, 0)


def test_random_frames_host_and_device_entry():
    cfg, frames = gc.random_drive()
    grid, counts = check_frames(cfg, frames)
    assert counts[:, :, 0].sum() > 1000 and counts[:, :, 1].max() >= 3 and counts[0].any() and counts[-1].any()  # clipped windows reached the border rows
    grid_dev, counts_dev = check_frames(cfg, frames, device=True)
    assert np.array_equal(counts_dev, counts)


@pytest.fixture(scope="module")
def cfg1_frame():
    """20 000 points of one scan in synthetic.py's cfg1 scene (20 beams x 1000 azimuths), base frame"""
    cfg = syn.CONFIGS["cfg1"]
    rng = np.random.Generator(np.random.PCG64(cfg.seed))
    scene = syn.make_scene(rng, **cfg.scene_kw)
    pose = gc.tilted_pose(1.2, -0.7, 0.9, np.deg2rad(1.5), np.deg2rad(-2.0))
    pts = syn.make_scan(scene, pose, syn.beam_directions(20, 1000, cfg.elev_deg), cfg.sensor_height, rng)
    assert pts.shape == (20000, 3)
    return np.ascontiguousarray(pts), pose, np.array([0.0, 0.0, cfg.sensor_height])


@pytest.mark.parametrize("cell", [0.25, 0.05])
def test_cfg1_frame(cfg1_frame, cell):
    side = int(round(70.0 / cell))
    cfg = gr.make_config(cell, -35.0, -35.0, side, side, 0.2, 2.2, 45.0)
    grid, counts = check_frames(cfg, [cfg1_frame])
    used, skipped, hit, miss = grid.last_frame()
    assert used > 3000 and skipped > 0 and miss > 5 * hit


def test_saturation():
    start = np.zeros((16, 16, 2), dtype=np.uint16)
    start[8, 11], start[8, 12], start[8, 9], start[8, 10] = (65535, 3), (65534, 0), (3, 65535), (0, 65534)
    grid = make_grid(CFG16)
    grid.set_counts(start)
    assert np.array_equal(grid.counts(), start)
    pts = np.array([[0.8, 0.1, 0.0], [1.1, 0.1, 0.0]])  # hits cells (11, 8) and (12, 8); the rays miss (8, 8), (9, 8), (10, 8)
    frame = (pts, gc.IDENTITY, SENSOR16)
    grid, counts = check_frames(CFG16, [frame], grid, start)
    assert counts[8, 11].tolist() == [65535, 3] and counts[8, 12].tolist() == [65535, 0]
    assert counts[8, 9].tolist() == [3, 65535] and counts[8, 10].tolist() == [0, 65535]
    grid, counts = check_frames(CFG16, [frame], grid, counts)  # once more: nothing wraps
    assert counts[8, 12].tolist() == [65535, 0] and counts[8, 10].tolist() == [0, 65535] and counts[8, 8].tolist() == [0, 2]


def test_readout_files_and_clear(tmp_path):
    cfg, frames = gc.random_drive()
    grid = make_grid(cfg)
    for pts, pose, sensor in frames[:4]:
        grid.integrate(pts, pose, sensor)
    counts = grid.counts()
    for min_observations in (1, 3):
        occ = grid.occupancy(min_observations)
        assert occ.dtype == np.int8 and occ.shape == (cfg["height"], cfg["width"])
        assert np.array_equal(occ, K.occupancy_from_counts(counts, min_observations)) and np.array_equal(occ, gr.occupancy(counts, min_observations))
    assert (occ == -1).any() and (occ == 0).any() and (occ == 100).any()
    a, b = str(tmp_path / "from_grid"), str(tmp_path / "from_host")
    grid.save_map(a, min_observations=3, occupied_thresh=0.6, free_thresh=0.2)
    K.write_map(b, occ, cfg["cell"], cfg["origin_x"], cfg["origin_y"], 0.6, 0.2)
    assert open(a + ".pgm", "rb").read() == open(b + ".pgm", "rb").read() == gr.map_files(a, occ, cfg["cell"], cfg["origin_x"], cfg["origin_y"], 0.6, 0.2)[0]
    assert open(a + ".yaml").read() == gr.map_files(a, occ, cfg["cell"], cfg["origin_x"], cfg["origin_y"], 0.6, 0.2)[1]
    assert open(a + ".yaml").read().replace("from_grid", "from_host") == open(b + ".yaml").read()
    info = grid.info()
    assert (info["frames"], info["reach"], info["width"], info["height"], info["cell"], info["max_ray"]) == (4, 60, 200, 160, 0.1, 6.0)
    grid.clear()
    assert not grid.counts().any() and grid.info()["frames"] == 0 and (grid.occupancy() == -1).all()
    check_frames(cfg, frames[4:], grid)  # usable after clear


def test_capacity_and_argument_errors(tmp_path):
    def code(**kw):
        args = dict(cell=0.25, origin_x=0.0, origin_y=0.0, width=16, height=16, z_min=0.0, z_max=1.0, max_ray=2.0)
        args.update(kw)
        with pytest.raises(K.KicpError) as e:
            K.OccupancyGrid(**args)
        return e.value.code, str(e.value)

    c, msg = code(width=16385, height=16384)  # 2^28 + 2^14 cells
    assert c == K.KICP_ERR_CAPACITY and "268451840" in msg
    c, msg = code(cell=0.25, max_ray=1023.9)  # reach 4096
    assert c == K.KICP_ERR_CAPACITY and "4096" in msg
    K.OccupancyGrid(0.25, 0.0, 0.0, 4, 4, 0.0, 1.0, 1023.75)  # reach 4095 is the limit
    for bad in (dict(cell=0.0), dict(cell=-0.1), dict(cell=np.nan), dict(cell=np.inf), dict(max_ray=0.0), dict(max_ray=np.inf), dict(origin_x=np.nan),
                dict(origin_y=np.inf), dict(z_min=1.0), dict(z_min=2.0), dict(z_min=np.nan), dict(width=0), dict(height=0)):
        assert code(**bad)[0] == K.KICP_ERR_ARG, bad
    import ctypes as C
    lib = K.lib()
    h = C.c_void_p()
    assert lib.kicp_grid_create(None, 0, C.byref(h)) == K.KICP_ERR_ARG
    assert lib.kicp_grid_create(C.byref(K.GridConfig(0.25, 0, 0, 4, 4, 0.0, 1.0, 1.0)), 0, None) == K.KICP_ERR_ARG
    grid = make_grid(CFG16)
    buf = np.zeros(16 * 16 * 2 + 2, dtype=np.uint16)
    u16, i8 = C.POINTER(C.c_ushort), C.POINTER(C.c_byte)
    assert lib.kicp_grid_counts(grid._h, buf.ctypes.data_as(u16), 257) == K.KICP_ERR_ARG
    assert lib.kicp_grid_counts(grid._h, None, 256) == K.KICP_ERR_ARG
    assert lib.kicp_grid_set_counts(grid._h, buf.ctypes.data_as(u16), 255) == K.KICP_ERR_ARG
    assert lib.kicp_grid_occupancy(grid._h, 1, buf.ctypes.data_as(i8), 255) == K.KICP_ERR_ARG
    assert lib.kicp_grid_occupancy(grid._h, 0, buf.ctypes.data_as(i8), 256) == K.KICP_ERR_ARG
    assert lib.kicp_grid_integrate(grid._h, None, 3, gc.IDENTITY.ctypes.data_as(K._dp), SENSOR16.ctypes.data_as(K._dp), None) == K.KICP_ERR_ARG
    assert lib.kicp_grid_integrate(None, None, 0, gc.IDENTITY.ctypes.data_as(K._dp), SENSOR16.ctypes.data_as(K._dp), None) == K.KICP_ERR_ARG
    assert lib.kicp_grid_integrate_device(grid._h, None, 0, None, SENSOR16.ctypes.data_as(K._dp), None) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clear(None) == K.KICP_ERR_ARG and lib.kicp_grid_info(None, None, None, None) == K.KICP_ERR_ARG
    with pytest.raises(K.KicpError) as e:
        grid.save_map(str(tmp_path / "m"), occupied_thresh=0.2, free_thresh=0.25)
    assert e.value.code == K.KICP_ERR_ARG
    with pytest.raises(K.KicpError) as e:
        grid.save_map(str(tmp_path / "missing" / "m"))
    assert e.value.code == K.KICP_ERR_ARG and "cannot write" in str(e.value)
    assert grid.info()["frames"] == 0 and not grid.counts().any()  # the handle is unharmed
