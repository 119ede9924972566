"""The height columns' carve on the GPU (kicp_elev_update*: K.ElevationLayer.update / update_device) against the restatement of
include/kicp.h's semantics (tests/elev_carve_ref.py).  Everything is exact: after EVERY frame the columns and the nine words must be
np.array_equal to the restatement's, through the host entry and the device entry - no tolerance anywhere.  The cases and what each is
there for: tests/elev_carve_cases.py; that each enters its regime is proven on the CPU (tests/test_elev_carve_host.py)."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import clearance_ref as cr
import elev_carve_cases as ecc
import elev_cases as ec
import elev_ref as er

pytestmark = pytest.mark.gpu


def make_layer(cfg, start=None):
    layer = K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"])
    if start is not None:
        layer.set_columns(start)
    return layer


def run_case(name, device):
    case, after, stats = ecc.reference(name)
    layer = make_layer(case["cfg"], case["start"])
    for k, (points, pose, sensor, (G, W, keep)) in enumerate(case["frames"]):
        got = layer.update_device(K.DeviceFrame(points), pose, sensor, G, W, keep) if device and len(points) else layer.update(points, pose, sensor, G, W, keep)
        print("%s frame %d: n = %d, restatement %s, device %s" % (name, k, len(points), stats[k], got))
        assert got == stats[k] and layer.last_update() == stats[k] and layer.last_frame() == stats[k][:6] and sum(got[:4]) == len(points)
        assert np.array_equal(layer.columns(), after[k])
        assert layer.last_window() == er.window(case["cfg"], pose, sensor)
    assert layer.info()["frames"] == len(case["frames"])
    return layer


@pytest.mark.parametrize("device", [False, True], ids=["host_entry", "device_entry"])
@pytest.mark.parametrize("name", sorted(ecc.CASES))
def test_case_equals_the_restatement(name, device):
    run_case(name, device)


def test_classes_change_only_inside_the_window_grown_by_one_cell():
    case, after, _ = ecc.reference("drive")
    cfg = case["cfg"]
    layer = make_layer(cfg, after[3])
    before = layer.traversability(2, 24)
    points, pose, sensor, (G, W, keep) = case["frames"][0]  # the first frame again, over what four frames left: it carves and it marks
    stats = layer.update(points + np.array([0.0, 0.0, 0.4]), pose, sensor, G, W, keep)
    assert stats[4] > 0 and stats[7] > 0
    classes = layer.traversability(2, 24)
    assert not np.array_equal(classes, before) and np.array_equal(classes, K.traversability_from_columns(layer.columns(), 2, 24))
    x0, y0, w, h = cr.grown(layer.last_window(), 1, cfg["width"], cfg["height"])
    pasted = before.copy()
    pasted[y0:y0 + h, x0:x0 + w] = layer.traversability(2, 24, rect=(x0, y0, w, h))
    assert np.array_equal(pasted, classes)


def test_update_and_integrate_share_the_layer():
    """an integrate between two updates never clears; the update after it carves what the integrate set; clear() forgets all"""
    case, after, stats = ecc.reference("keep_ground_clear")
    points, pose, sensor, (G, W, keep) = case["frames"][0]
    layer = make_layer(case["cfg"], case["start"])
    assert layer.last_update() == (0,) * 9
    assert layer.update(points, pose, sensor, G, W, keep) == stats[0]
    layer.set_columns(case["start"])
    want = case["start"].copy()
    plain = er.integrate(case["cfg"], want, points, pose, sensor)
    assert layer.integrate(points, pose, sensor) == plain and np.array_equal(layer.columns(), want) and layer.last_update() == stats[0]
    # without keep_ground (c | marks) & ~M | marks == c & ~M | marks: the columns are the update's on the start columns
    assert layer.update_device(K.DeviceFrame(points), pose, sensor, G, W, keep)[6] == stats[0][6] and np.array_equal(layer.columns(), after[0])
    assert layer.info()["frames"] == 3
    layer.clear()
    assert not layer.columns().any() and layer.info()["frames"] == 0 and layer.last_window() == (0, 0, 0, 0)
    assert layer.update(points, pose, sensor, G, W, keep)[6:] == (len(points), 0, 0)  # usable after clear: nothing is there to carve


def test_passer_by_columns_equal_the_restatement():
    plain, carved = ecc.passer_by_reference()
    layer, layer_plain = make_layer(ecc.PASSER_CFG), make_layer(ecc.PASSER_CFG)
    for k, (points, pose, sensor) in enumerate(ecc.passer_by()):
        frame = K.DeviceFrame(points)
        got = layer.update_device(frame, pose, sensor, *ecc.PASSER_CARVE) if k % 2 else layer.update(points, pose, sensor, *ecc.PASSER_CARVE)
        layer_plain.integrate_device(frame, pose, sensor)
        print("passer-by frame %d: %s" % (k, got))
    assert np.array_equal(layer.columns(), carved) and np.array_equal(layer_plain.columns(), plain)
    S, H = ecc.PASSER_CLASSES
    classes, counts = layer.traversability(S, H, rect=(158, 142, 8, 8), return_counts=True)
    assert (classes == 100).sum() <= 2 and counts[2] == 0 and (layer_plain.traversability(S, H)[ecc.PASSER_REGION] == 100).sum() == 16


def test_argument_errors():
    case, after, stats = ecc.reference("level_rays")
    points, pose, sensor, (G, W, keep) = case["frames"][0]
    layer = make_layer(case["cfg"], case["start"])
    for kw in (dict(widen_slabs=65), dict(keep_ground=2), dict(widen_slabs=0xFFFFFFFF)):
        for call in (lambda: layer.update(points, pose, sensor, **kw), lambda: layer.update_device(K.DeviceFrame(points), pose, sensor, **kw)):
            with pytest.raises(K.KicpError) as e:
                call()
            assert e.value.code == K.KICP_ERR_ARG, kw
    lib, carve, out = K.lib(), K.ElevationCarveConfig(G, W, keep), np.zeros(9, dtype=np.uint64)
    xp, pp, sp, op = points.ctypes.data_as(K._dp), pose.ctypes.data_as(K._dp), sensor.ctypes.data_as(K._dp), out.ctypes.data_as(C.POINTER(C.c_ulonglong))
    assert lib.kicp_elev_update(None, xp, 4, pp, sp, C.byref(carve), op) == K.KICP_ERR_ARG and lib.kicp_elev_update(layer._h, None, 4, pp, sp, C.byref(carve), op) == K.KICP_ERR_ARG
    assert lib.kicp_elev_update(layer._h, xp, 4, None, sp, C.byref(carve), op) == K.KICP_ERR_ARG and lib.kicp_elev_update(layer._h, xp, 4, pp, None, C.byref(carve), op) == K.KICP_ERR_ARG
    assert lib.kicp_elev_update(layer._h, xp, 4, pp, sp, None, op) == K.KICP_ERR_ARG and lib.kicp_elev_update_device(layer._h, None, 0, pp, sp, None, op) == K.KICP_ERR_ARG
    assert lib.kicp_elev_update_device(None, None, 0, pp, sp, C.byref(carve), op) == K.KICP_ERR_ARG and lib.kicp_elev_update_device(layer._h, None, 1, pp, sp, C.byref(carve), op) == K.KICP_ERR_ARG
    assert lib.kicp_elev_update_device(layer._h, C.c_void_p(16), 0x7FFFFFF0 // 3 + 1, pp, sp, C.byref(carve), op) == K.KICP_ERR_CAPACITY
    assert layer.info()["frames"] == 0 and np.array_equal(layer.columns(), case["start"]) and not out.any() and layer.last_window() == (0, 0, 0, 0)  # the handle is unharmed
    assert lib.kicp_elev_update(layer._h, xp, 4, pp, sp, C.byref(carve), None) == K.KICP_OK and np.array_equal(layer.columns(), after[0])  # no statistics asked for
    assert lib.kicp_elev_update_device(layer._h, None, 0, pp, sp, C.byref(carve), op) == K.KICP_OK and not out.any() and layer.info()["frames"] == 2  # n == 0: counted
