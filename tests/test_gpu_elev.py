"""The height columns on the GPU (kicp_elev_*: K.ElevationLayer) against the numpy restatement of include/kicp.h's semantics
(tests/elev_ref.py).  Everything is exact: after EVERY frame the columns and the six frame statistics must be np.array_equal to the
restatement's, and every class, ground byte and count of the traversability likewise - no tolerance anywhere.  Layer sides around
one and two tiles, counts where waves share a shard (300 x 300) and frames around a wave's and a workgroup's size:
tests/test_gpu_plan_regimes.py."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import clearance_ref as cr
import elev_cases as ec
import elev_ref as er

pytestmark = pytest.mark.gpu


def make_layer(cfg, device=0):
    return K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"], device=device)


def check_frames(cfg, frames, layer=None, start=None, device=False):
    """integrate `frames` one by one; after each the columns, the statistics and the window equal the restatement's -> (layer, columns)"""
    layer = layer or make_layer(cfg)
    want = np.zeros((cfg["height"], cfg["width"]), dtype=np.uint64) if start is None else start.copy()
    for pts, pose, sensor in frames:
        stats = er.integrate(cfg, want, pts, pose, sensor)
        got = layer.integrate_device(K.DeviceFrame(pts), pose, sensor) if device else layer.integrate(pts, pose, sensor)
        print("frame: n = %d, restatement %s, device %s" % (len(pts), stats, got))
        assert got == stats and layer.last_frame() == stats and sum(got[:4]) == len(pts)
        assert np.array_equal(layer.columns(), want)
        assert layer.last_window() == er.window(cfg, pose, sensor)
    return layer, want


@pytest.mark.parametrize("name", sorted(ec.ONE_POINT))
def test_one_point(name):
    point, cls, where = ec.ONE_POINT[name]
    pts = np.array([point], dtype=np.float64)
    got_cls, cx, cy, s = er.point_classes(ec.CFG16, pts, ec.IDENTITY, ec.SENSOR16)
    assert got_cls[0] == cls and ec.CFG16["reach"] == 6
    layer, columns = check_frames(ec.CFG16, [(pts, ec.IDENTITY, ec.SENSOR16)])
    if where is None:
        assert not columns.any() and layer.last_frame()[4:] == (0, 0)
    else:
        ix, iy, slab = where
        assert (int(cx[0]), int(cy[0]), int(s[0])) == where and int(columns[iy, ix]) == 1 << slab and np.count_nonzero(columns) == 1
        assert layer.last_frame() == (1, 0, 0, 0, 1, 1)


def test_inside_reach_but_outside_the_grid_and_nothing_finite():
    layer, columns = check_frames(ec.CFG16, [(ec.INSIDE_REACH_OUTSIDE_GRID, ec.IDENTITY, ec.SENSOR16_EAST)])
    assert layer.last_frame() == (0, 0, 1, 0, 0, 0) and not columns.any()
    pts = ec.contended_three(64)
    nan_pose = np.array([0.0, 0.0, 0.0, 1.0, np.nan, 0.0, 0.0])
    check_frames(ec.CFG16, [(pts, nan_pose, ec.SENSOR16), (pts, ec.IDENTITY, np.array([np.nan, 0.0, 0.0]))], layer)
    assert layer.last_frame() == (0, 64, 0, 0, 0, 0) and layer.last_window() == (0, 0, 0, 0)  # a NaN sensor cell skips everything
    nan_z = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, np.nan])  # the plane is finite, the height is not: a non-finite world coordinate
    check_frames(ec.CFG16, [(pts, nan_z, ec.SENSOR16)], layer)
    assert layer.last_frame() == (0, 64, 0, 0, 0, 0) and layer.last_window() == (2, 2, 13, 13)
    assert layer.integrate(np.zeros((0, 3)), ec.IDENTITY, ec.SENSOR16) == (0, 0, 0, 0, 0, 0)  # n == 0: nothing changes, the frame is counted
    assert layer.info()["frames"] == 5 and not layer.columns().any()


def test_contended_bits():
    frame = (ec.contended_three(), ec.IDENTITY, ec.SENSOR16)
    layer, columns = check_frames(ec.CFG16, [frame])
    assert layer.last_frame() == (4096, 0, 0, 0, 3, 3) and sorted(int(c) for c in columns[columns != 0]) == [1 << 4, 1 << 8, 1 << 12]
    layer, again = check_frames(ec.CFG16, [frame], layer, columns, device=True)  # the same frame again: nothing is new
    assert layer.last_frame() == (4096, 0, 0, 0, 0, 0) and np.array_equal(again, columns)
    layer, columns = check_frames(ec.CFG16, [(ec.contended_one_cell(), ec.IDENTITY, ec.SENSOR16)], layer, columns)
    assert layer.last_frame() == (4096, 0, 0, 0, 64, 1) and int(columns[10, 10]) == ec.FULL
    fresh, _ = check_frames(ec.CFG16, [(ec.contended_one_cell(), ec.IDENTITY, ec.SENSOR16)], device=True)
    assert fresh.last_frame() == (4096, 0, 0, 0, 64, 1)


def test_roll_and_pitch_host_and_device_entry():
    frame = ec.tilted_frame()
    cls, _, _, s = er.point_classes(ec.CFG16, *frame)
    assert len(set(s[cls == er.USED].tolist())) > 15 and (cls == er.OUTSIDE_COLUMN).any() and (cls == er.SKIPPED).any()
    flat = er.point_classes(ec.CFG16, frame[0], ec.IDENTITY, frame[2])[3]
    assert not np.array_equal(flat, s)  # wz depends on x and y
    layer, columns = check_frames(ec.CFG16, [frame])
    layer_dev, columns_dev = check_frames(ec.CFG16, [frame], device=True)
    assert np.array_equal(columns_dev, columns)


@pytest.fixture(scope="module")
def drive():
    cfg, frames = ec.random_drive()
    return cfg, frames


def test_random_drive_host_and_device_entry(drive):
    cfg, frames = drive
    layer, columns = check_frames(cfg, frames)
    stats = layer.last_frame()
    assert np.count_nonzero(columns) > 3000 and columns[0].any() and stats[0] > 1000  # the clipped window reached the border row
    layer_dev, columns_dev = check_frames(cfg, frames, device=True)
    assert np.array_equal(columns_dev, columns)
    # a frame changes classes only inside its window grown by one cell
    before = layer.traversability(2, 24)
    pts, pose, sensor = frames[0]
    layer.integrate(pts + np.array([0.0, 0.0, 0.4]), pose, sensor)
    after = layer.traversability(2, 24)
    assert not np.array_equal(after, before) and np.array_equal(after, K.traversability_from_columns(layer.columns(), 2, 24))
    x0, y0, w, h = cr.grown(layer.last_window(), 1, cfg["width"], cfg["height"])
    pasted = before.copy()
    pasted[y0:y0 + h, x0:x0 + w] = layer.traversability(2, 24, rect=(x0, y0, w, h))
    assert np.array_equal(pasted, after)
    layer.clear()
    assert not layer.columns().any() and layer.info()["frames"] == 0 and layer.last_window() == (0, 0, 0, 0) and (layer.traversability(2, 24) == -1).all()
    check_frames(cfg, frames[4:], layer)  # usable after clear


@pytest.fixture(scope="module")
def layer70():
    return make_layer(er.make_config(0.25, 0.0, 0.0, ec.W70, ec.H45, 0.0, 0.125, 2.0))


def check_classification(layer, columns):
    layer.set_columns(columns)
    assert np.array_equal(layer.columns(), columns)
    for S, H in ec.PARAMS:
        cls, ground, body, _ = er.classify(columns, S, H)
        for rect in ec.RECTS:
            r = rect or (0, 0, ec.W70, ec.H45)
            got, got_ground, got_counts = layer.traversability(S, H, rect=rect, return_ground=True, return_counts=True)
            assert got.dtype == np.int8 and got.shape == (r[3], r[2])
            assert np.array_equal(got, er.restrict(cls, r)), (S, H, rect)  # a rectangle's result is the full result restricted to it
            assert np.array_equal(got_ground, er.restrict(ground, r)), (S, H, rect)
            assert got_counts == er.counts(er.restrict(cls, r), er.restrict(body, r)), (S, H, rect)
        assert np.array_equal(layer.traversability(S, H), cls)  # without the optional outputs
        assert np.array_equal(K.traversability_from_columns(columns, S, H), cls)


def test_classification_of_handmade_columns(layer70):
    check_classification(layer70, ec.handmade_columns())


@pytest.mark.parametrize("kind", ["dense", "sparse", "zero"])
def test_classification_of_random_columns(layer70, kind):
    check_classification(layer70, ec.random_columns(kind))


def test_to_grid(layer70):
    columns = ec.random_columns("sparse")
    columns[ec.handmade_columns() != 0] = ec.handmade_columns()[ec.handmade_columns() != 0]
    layer70.set_columns(columns)
    grid = K.OccupancyGrid(0.25, 0.0, 0.0, ec.W70, ec.H45, -1.0, 1.0, 2.0)
    grid.set_counts(np.full((ec.H45, ec.W70, 2), 7, dtype=np.uint16))  # every counter is replaced
    for S, H in ((2, 8), (0, 64)):
        classes = layer70.traversability(S, H)
        layer70.to_grid(grid, S, H)
        counts = grid.counts()
        assert np.array_equal(counts[:, :, 0], (classes == 100).astype(np.uint16)) and np.array_equal(counts[:, :, 1], (classes == 0).astype(np.uint16))
        assert np.array_equal(grid.occupancy(1), classes)
        table = K.nav2_cost_table(0.25, 5, 0.4, 3.0)
        for kw in (dict(), dict(unknown_is_obstacle=True, inflate_unknown=True)):
            assert np.array_equal(grid.costmap(table, **kw), K.costmap_from_occupancy(classes, table, **kw))
    assert (classes == -1).any() and (classes == 0).any() and (classes == 100).any()
    cfg = K.ElevationTraversabilityConfig(2, 8)
    for other in (K.OccupancyGrid(0.125, 0.0, 0.0, ec.W70, ec.H45, -1.0, 1.0, 2.0), K.OccupancyGrid(0.25, 0.25, 0.0, ec.W70, ec.H45, -1.0, 1.0, 2.0),
                  K.OccupancyGrid(0.25, 0.0, 0.0, ec.W70, ec.H45 + 1, -1.0, 1.0, 2.0), K.OccupancyGrid(0.25, 0.0, 0.0, ec.H45, ec.W70, -1.0, 1.0, 2.0)):
        with pytest.raises(K.KicpError) as e:
            layer70.to_grid(other, 2, 8)
        assert e.value.code == K.KICP_ERR_ARG
    lib = K.lib()
    assert lib.kicp_elev_to_grid(None, C.byref(cfg), grid._h) == K.KICP_ERR_ARG and lib.kicp_elev_to_grid(layer70._h, None, grid._h) == K.KICP_ERR_ARG
    assert lib.kicp_elev_to_grid(layer70._h, C.byref(cfg), None) == K.KICP_ERR_ARG
    with pytest.raises(K.KicpError) as e:
        layer70.to_grid(grid, 8, 8)
    assert e.value.code == K.KICP_ERR_ARG
    assert np.array_equal(grid.occupancy(1), classes)  # the refused calls left the grid alone


def test_to_grid_refuses_a_grid_on_another_device(layer70):
    if K.device_count() < 2:
        pytest.skip("one GPU is visible here")
    other = K.OccupancyGrid(0.25, 0.0, 0.0, ec.W70, ec.H45, -1.0, 1.0, 2.0, device=1)
    with pytest.raises(K.KicpError) as e:
        layer70.to_grid(other, 2, 8)
    assert e.value.code == K.KICP_ERR_ARG and "device" in str(e.value)


def test_capacity_and_argument_errors():
    def code(**kw):
        args = dict(cell=0.25, origin_x=0.0, origin_y=0.0, width=16, height=16, z_origin=0.0, slab=0.125, max_ray=2.0)
        args.update(kw)
        with pytest.raises(K.KicpError) as e:
            K.ElevationLayer(**args)
        return e.value.code, str(e.value)

    c, msg = code(width=16385, height=16384)  # 2^28 + 2^14 cells
    assert c == K.KICP_ERR_CAPACITY and "268451840" in msg
    c, msg = code(cell=0.25, max_ray=1023.9)  # reach 4096
    assert c == K.KICP_ERR_CAPACITY and "4096" in msg
    K.ElevationLayer(0.25, 0.0, 0.0, 4, 4, 0.0, 0.125, 1023.75)  # reach 4095 is the limit
    for bad in (dict(cell=0.0), dict(cell=-0.1), dict(cell=np.nan), dict(cell=np.inf), dict(max_ray=0.0), dict(max_ray=np.inf), dict(origin_x=np.nan),
                dict(origin_y=np.inf), dict(z_origin=np.nan), dict(z_origin=-np.inf), dict(slab=0.0), dict(slab=-1.0), dict(slab=np.nan), dict(slab=np.inf),
                dict(width=0), dict(height=0)):
        assert code(**bad)[0] == K.KICP_ERR_ARG, bad
    lib = K.lib()
    h = C.c_void_p()
    assert lib.kicp_elev_create(None, 0, C.byref(h)) == K.KICP_ERR_ARG
    assert lib.kicp_elev_create(C.byref(K.ElevationConfig(0.25, 0, 0, 4, 4, 0.0, 0.125, 1.0)), 0, None) == K.KICP_ERR_ARG
    layer = make_layer(ec.CFG16)
    buf = np.zeros(16 * 16 + 2, dtype=np.uint64)
    u64, i8, u8 = C.POINTER(C.c_ulonglong), C.POINTER(C.c_byte), C.POINTER(C.c_ubyte)
    pose, sensor = ec.IDENTITY.ctypes.data_as(K._dp), ec.SENSOR16.ctypes.data_as(K._dp)
    assert lib.kicp_elev_columns(layer._h, buf.ctypes.data_as(u64), 257) == K.KICP_ERR_ARG
    assert lib.kicp_elev_columns(layer._h, None, 256) == K.KICP_ERR_ARG and lib.kicp_elev_columns(None, buf.ctypes.data_as(u64), 256) == K.KICP_ERR_ARG
    assert lib.kicp_elev_set_columns(layer._h, buf.ctypes.data_as(u64), 255) == K.KICP_ERR_ARG
    assert lib.kicp_elev_set_columns(layer._h, None, 256) == K.KICP_ERR_ARG and lib.kicp_elev_set_columns(None, buf.ctypes.data_as(u64), 256) == K.KICP_ERR_ARG
    assert lib.kicp_elev_integrate(layer._h, None, 3, pose, sensor, None) == K.KICP_ERR_ARG
    assert lib.kicp_elev_integrate(None, None, 0, pose, sensor, None) == K.KICP_ERR_ARG
    assert lib.kicp_elev_integrate(layer._h, None, 0, pose, None, None) == K.KICP_ERR_ARG
    assert lib.kicp_elev_integrate_device(layer._h, None, 0, None, sensor, None) == K.KICP_ERR_ARG
    assert lib.kicp_elev_integrate_device(layer._h, C.c_void_p(16), 0x7FFFFFF0 // 3 + 1, pose, sensor, None) == K.KICP_ERR_CAPACITY
    assert lib.kicp_elev_clear(None) == K.KICP_ERR_ARG and lib.kicp_elev_info(None, None, None, None) == K.KICP_ERR_ARG
    v = [C.c_uint(9) for _ in range(4)]
    assert lib.kicp_elev_last_window(None, *[C.byref(x) for x in v]) == K.KICP_ERR_ARG
    assert lib.kicp_elev_last_window(layer._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), None) == K.KICP_ERR_ARG
    assert lib.kicp_elev_last_window(layer._h, *[C.byref(x) for x in v]) == K.KICP_OK and [x.value for x in v] == [0, 0, 0, 0]  # before any frame
    cfg = K.ElevationTraversabilityConfig(1, 4)
    out = buf.ctypes.data_as(i8)
    assert lib.kicp_elev_traversability(None, C.byref(cfg), 0, 0, 16, 16, out, None, None, 256) == K.KICP_ERR_ARG
    assert lib.kicp_elev_traversability(layer._h, None, 0, 0, 16, 16, out, None, None, 256) == K.KICP_ERR_ARG
    assert lib.kicp_elev_traversability(layer._h, C.byref(cfg), 0, 0, 16, 16, None, None, None, 256) == K.KICP_ERR_ARG
    assert lib.kicp_elev_traversability(layer._h, C.byref(cfg), 0, 0, 16, 16, out, None, None, 255) == K.KICP_ERR_ARG
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (16, 0, 1, 1), (0, 16, 1, 1), (9, 0, 8, 1), (0, 9, 1, 8)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability(1, 4, rect=rect)
        assert e.value.code == K.KICP_ERR_ARG, rect
    for S, H in ((63, 64), (0, 0), (3, 3), (4, 2), (0, 65)):
        with pytest.raises(K.KicpError) as e:
            layer.traversability(S, H)
        assert e.value.code == K.KICP_ERR_ARG, (S, H)
    info = layer.info()
    assert (info["frames"], info["reach"], info["width"], info["height"], info["cell"], info["z_origin"], info["slab"], info["max_ray"]) == (0, 6, 16, 16, 0.25, -1.0, 0.125, 1.5)
    assert not layer.columns().any() and (layer.traversability(1, 4) == -1).all()  # the handle is unharmed
