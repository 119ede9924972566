"""The depth view on the GPU (kicp_view_*: K.DepthView) against the numpy restatement of include/kicp.h's semantics (tests/view_ref.py),
which tests/test_view_host.py holds to pixels and verdicts written out by hand.  Everything is exact: the image, the two frame
statistics and every verdict must be np.array_equal to the restatement's - no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import view_cases as vc
import view_ref as vr

pytestmark = pytest.mark.gpu

UNIT = vc.unit_cases()


def make_view(cfg):
    return K.DepthView(cfg["res"], cfg["window"], cfg["min_rays"], cfg["max_ray"], cfg["margin"], cfg["margin_per_metre"])


def check_case(case, device=False, view=None):
    """render the case's frame and classify its queries: image, statistics and verdicts equal the restatement's -> (view, depth, verdicts)"""
    cfg = case["cfg"]
    view = view or make_view(cfg)
    depth, stats, c = vr.render(cfg, case["frame"], case["pose"], case["sensor"])
    got = view.render_device(K.DeviceFrame(case["frame"]), case["pose"], case["sensor"]) if device else view.render(case["frame"], case["pose"], case["sensor"])
    print("render: n = %d, restatement %s, device %s" % (len(case["frame"]), stats, got))
    assert got == stats and view.last_frame() == stats
    image = view.depth()
    assert image.dtype == np.float32 and np.array_equal(image, depth)
    sensor_world = view.info()["sensor_world"]
    assert np.array_equal(sensor_world, c, equal_nan=True)
    want = vr.verdict(cfg, depth, c, case["queries"])
    verdicts = view.classify(case["queries"])
    assert verdicts.dtype == np.uint8 and np.array_equal(verdicts, want)
    return view, image, verdicts


@pytest.mark.parametrize("name", sorted(UNIT))
def test_unit_case(name):
    """one point per face and sign, ties, the clamp, m == 0, points / pose / sensor that are not finite, exactly max_ray and just beyond, two
    points in one pixel, a depth float cannot hold, 4 096 points in three pixels, N == min_rays - 1 against N == min_rays, m + margin == D,
    windows clipped at an edge and a corner, an empty image, a face without returns (tests/view_cases.py states each)"""
    case = UNIT[name]
    _, image, verdicts = check_case(case)
    if case["verdicts"] is not None:
        assert verdicts.tolist() == case["verdicts"]
    if case["pixels"] is not None:
        assert int(np.isfinite(image).sum()) == len(case["pixels"])
        for (face, w_, u), d in case["pixels"].items():
            assert image[face, w_, u] == np.float32(d)


@pytest.mark.parametrize("name", ["tilted", "contended", "faces", "empty_image", "not_finite_pose"])
def test_host_entry_and_device_entry_give_the_same_image(name):
    case = UNIT[name]
    _, from_host, v_host = check_case(case)
    _, from_device, v_device = check_case(case, device=True)
    assert np.array_equal(from_host, from_device) and np.array_equal(v_host, v_device)


def test_a_frame_replaces_the_image_and_order_does_not_matter():
    case = UNIT["tilted"]
    view, first, _ = check_case(case)
    rng = np.random.default_rng(2)
    shuffled = dict(case, frame=case["frame"][rng.permutation(len(case["frame"]))])
    _, again, _ = check_case(shuffled, view=view)
    assert np.array_equal(first, again)
    other = dict(UNIT["faces"], cfg=case["cfg"])
    _, image, _ = check_case(other, view=view)  # nothing of the earlier frame is left
    assert int(np.isfinite(image).sum()) == 6
    _, image, _ = check_case(dict(case, frame=np.zeros((0, 3))), view=view)
    assert not np.isfinite(image).any()
    assert view.info()["frames"] == 4


def test_more_than_one_block_and_a_larger_image():
    """20 000 points (79 workgroups) at res 64 and window 4: random directions, depths from 6 m to beyond max_ray, queries on both sides of them"""
    rng = np.random.default_rng(11)
    cfg = vr.make_config(64, 4, 5, 12.0, 0.05, 0.01)
    pose = np.concatenate([vc._unit([0.02, 0.01, -0.3, 0.95]), [-3.0, 4.0, 0.5]])
    frame = rng.normal(size=(20000, 3))
    frame *= (rng.uniform(6.0, 14.0, 20000) / np.abs(frame).max(axis=1))[:, None]
    queries = rng.uniform(-13, 13, (5000, 3)) + pose[4:]
    case = dict(cfg=cfg, frame=frame, pose=pose, sensor=np.array([0.1, 0.0, 0.4]), queries=queries)
    view, image, verdicts = check_case(case, device=True)
    assert view.last_frame()[1] > 1000 and (verdicts == 3).sum() > 200 and (verdicts == 2).sum() > 200 and (verdicts == 0).sum() > 200


def test_capacity_and_argument_errors():
    def code(**kw):
        args = dict(res=16, window=1, min_rays=2, max_ray=10.0, margin=0.2, margin_per_metre=0.02)
        args.update(kw)
        with pytest.raises(K.KicpError) as e:
            K.DepthView(**args)
        return e.value.code, str(e.value)

    c, msg = code(res=1026)
    assert c == K.KICP_ERR_CAPACITY and "1026" in msg
    c, msg = code(window=5, min_rays=1)
    assert c == K.KICP_ERR_CAPACITY and "5" in msg
    K.DepthView(1024, 4, 81, 1.0, 0.0, 0.0)  # the limits themselves
    K.DepthView(8, 0, 1, 1.0, 0.0, 0.0)
    for bad in (dict(res=6), dict(res=17), dict(res=0), dict(window=-1), dict(min_rays=0), dict(min_rays=10), dict(window=0, min_rays=2), dict(max_ray=0.0),
                dict(max_ray=-1.0), dict(max_ray=np.inf), dict(max_ray=np.nan), dict(margin=-0.1), dict(margin=np.nan), dict(margin=np.inf),
                dict(margin_per_metre=-0.01), dict(margin_per_metre=np.nan), dict(margin_per_metre=np.inf)):
        assert code(**bad)[0] == K.KICP_ERR_ARG, bad
    lib = K.lib()
    h = C.c_void_p()
    assert lib.kicp_view_create(None, 0, C.byref(h)) == K.KICP_ERR_ARG
    assert lib.kicp_view_create(C.byref(K.ViewConfig(16, 1, 2, 10.0, 0.2, 0.02)), 0, None) == K.KICP_ERR_ARG
    view = make_view(vr.make_config(16, 1, 2, 10.0, 0.2, 0.02))
    buf = np.zeros(6 * 16 * 16 + 2, dtype=np.float32)
    f32, u8, dp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), K._dp
    pose, sensor = vc.IDENTITY.ctypes.data_as(dp), vc.ORIGIN.ctypes.data_as(dp)
    assert lib.kicp_view_depth(view._h, buf.ctypes.data_as(f32), 6 * 16 * 16 + 1) == K.KICP_ERR_ARG
    assert lib.kicp_view_depth(view._h, None, 6 * 16 * 16) == K.KICP_ERR_ARG
    assert lib.kicp_view_depth(None, buf.ctypes.data_as(f32), 6 * 16 * 16) == K.KICP_ERR_ARG
    assert lib.kicp_view_render(view._h, None, 3, pose, sensor, None) == K.KICP_ERR_ARG
    assert lib.kicp_view_render(None, None, 0, pose, sensor, None) == K.KICP_ERR_ARG
    assert lib.kicp_view_render(view._h, None, 0, None, sensor, None) == K.KICP_ERR_ARG
    assert lib.kicp_view_render_device(view._h, None, 0, pose, None, None) == K.KICP_ERR_ARG
    assert lib.kicp_view_render_device(view._h, None, 2, pose, sensor, None) == K.KICP_ERR_ARG
    pts = np.zeros((2, 3))
    assert lib.kicp_view_render(view._h, pts.ctypes.data_as(dp), (0x7FFFFFF0 // 3) + 1, pose, sensor, None) == K.KICP_ERR_CAPACITY
    assert lib.kicp_view_classify(view._h, None, 2, buf.ctypes.data_as(u8)) == K.KICP_ERR_ARG
    assert lib.kicp_view_classify(view._h, pts.ctypes.data_as(dp), 2, None) == K.KICP_ERR_ARG
    assert lib.kicp_view_classify(None, pts.ctypes.data_as(dp), 2, buf.ctypes.data_as(u8)) == K.KICP_ERR_ARG
    assert lib.kicp_view_classify(view._h, None, 0, None) == K.KICP_OK
    assert lib.kicp_view_info(None, None, None, None) == K.KICP_ERR_ARG
    gmap = K.VoxelHashMap(1.0, 100.0, 20)
    assert lib.kicp_map_remove_seen_through(None, view._h, None) == K.KICP_ERR_ARG
    assert lib.kicp_map_remove_seen_through(gmap._h, None, None) == K.KICP_ERR_ARG
    info = view.info()  # the handle is unharmed
    assert info["frames"] == 0 and np.isnan(info["sensor_world"]).all() and not np.isfinite(view.depth()).any()
    assert view.classify(np.array([[1.0, 0.0, 0.0]])).tolist() == [0]  # before the first frame nothing is in range
