"""CPU tests of how the binding is laid out (kinematic_icp_amd/_ffi.py and the feature modules): importing loads nothing, the one
rule for "may this Python object still destroy its handle" reads the live library slot, a handle whose creation failed frees nothing,
and the feature modules' signature tables add up to the one table lib() applies.  No kernel is launched here."""
import os
import subprocess
import sys

import pytest

import kinematic_icp_amd as K
from conftest import ROOT

PACKAGE = os.path.join(ROOT, "kinematic_icp_amd")


def _child(code):
    """run `code` in a fresh interpreter from the repository's root; its assertions are the test"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _declaring_modules():
    """the package's modules that declare entries of the library, by their source"""
    names = [f[:-3] for f in sorted(os.listdir(PACKAGE)) if f.endswith(".py") and f != "__init__.py"]
    return [n for n in names if "_declare(" in open(os.path.join(PACKAGE, n + ".py")).read()]


def test_import_loads_nothing_and_imports_every_declaring_module():
    loaded = _child("""
import sys
import kinematic_icp_amd as K
assert K._ffi._lib is None, "importing the package loaded the library"
assert not hasattr(K, "_lib"), "a re-exported _lib is a copy of import time's None"
print(" ".join(sorted(m.split(".", 1)[1] for m in sys.modules if m.startswith("kinematic_icp_amd."))))
""").split()
    declaring = _declaring_modules()
    assert len(declaring) >= 10 and "_ffi" in declaring
    assert set(declaring) <= set(loaded), sorted(set(declaring) - set(loaded))  # a module __init__ leaves out declares too late for lib()


def test_handles_read_the_live_library_slot():
    """Before lib() no __del__ loads the library or calls into it; after lib() - in the same process, so a `from ._ffi import _lib`
    anywhere would still hold None - a set handle is destroyed exactly once, and a DeviceFrame frees its pointer unless it is borrowed."""
    _child("""
import ctypes as C
import gc
import kinematic_icp_amd as K
m = object.__new__(K.VoxelHashMap)
m._h = C.c_void_p(1)
f = K.DeviceFrame._borrow(4096, 0, 0)
f._borrowed = False
del m, f
gc.collect()
assert K._ffi._lib is None, "__del__ loaded the library"
for module in (K._ffi, K.device, K.elevation, K.explore, K.grid, K.plan, K.presteps, K.registration, K.search, K.view, K.voxel_map):
    assert module is K._ffi or "_lib" not in vars(module), module.__name__
L = K.lib()
assert K._ffi._lib is L
calls = []
L.kicp_map_destroy = lambda h: calls.append(("map", h.value))  # (stand-ins on the loaded library: nothing real is freed)
L.kicp_device_free = lambda device, p: calls.append(("free", device, p.value))
m = object.__new__(K.VoxelHashMap)
m._h = C.c_void_p(1)
m.__del__()
del m
own, borrowed = K.DeviceFrame._borrow(4096, 0, 3), K.DeviceFrame._borrow(8192, 0, 3)
own._borrowed = False
del own, borrowed
gc.collect()
assert calls == [("map", 1), ("free", 3, 4096)], calls
""")


def test_a_handle_whose_creation_failed_frees_nothing():
    """kicp_grid_create refuses width = 0 before it touches a device; what _create leaves behind is collected without a destroy call"""
    _child("""
import ctypes as C
import gc
import kinematic_icp_amd as K
L = K.lib()
calls = []
L.kicp_grid_destroy = lambda h: calls.append(h)
g = object.__new__(K.OccupancyGrid)
cfg = K.GridConfig(0.1, 0.0, 0.0, 0, 4, -1.0, 1.0, 10.0)
try:
    g._create("kicp_grid_create", C.byref(cfg), 0)
    raise SystemExit("kicp_grid_create accepted width = 0")
except K.KicpError as e:
    assert e.code == K.KICP_ERR_ARG, e
assert g._h is None
del g
try:
    K.OccupancyGrid(0.1, 0.0, 0.0, 0, 4, -1.0, 1.0, 10.0)
    raise SystemExit("OccupancyGrid accepted width = 0")
except K.KicpError as e:
    assert e.code == K.KICP_ERR_ARG, e
gc.collect()
assert calls == [], calls
""")


def test_signature_tables_are_disjoint_and_add_up():
    tables = {name: getattr(K, name)._ENTRIES for name in _declaring_modules()}
    names = [entry for table in tables.values() for entry in table]
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert set(names) == set(K._SIGNATURES)
    assert K._SIGNATURES is K._ffi._SIGNATURES
    for table in tables.values():
        for entry, signature in table.items():
            assert K._SIGNATURES[entry] is signature
    with pytest.raises(ImportError, match="kicp_version"):
        K._ffi._declare({"kicp_version": (None, [])})
