"""The GPU itself (kicp_device_*, kicp_comm_unique_id, kicp_probe_dependent_load): how many there are and where they sit, a scan
resident in HBM, and what the multi-GPU exchanges need before a registration exists."""
import ctypes as C
import os

from . import _ffi
from ._ffi import _check, _d, _declare, _hp, _intp, lib

COMM_ID_BYTES = 128

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)

_ENTRIES = _declare({
    "kicp_device_count": (C.c_int, []),
    "kicp_device_locality": (C.c_int, [C.c_int, _intp, C.c_char_p, C.c_size_t]),
    "kicp_device_malloc": (C.c_int, [C.c_int, C.c_size_t, _hp]),
    "kicp_device_free": (C.c_int, [C.c_int, C.c_void_p]),
    "kicp_device_upload": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "kicp_device_synchronize": (C.c_int, [C.c_int]),
    "kicp_comm_unique_id": (C.c_int, [C.c_char_p]),
    "kicp_probe_dependent_load": (C.c_int, [C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
})


def probe_dependent_load(working_set_bytes, workgroups=512, block=256, steps=64, device=0):
    """ns per dependent load step of `workgroups` x `block` lanes walking a random chain through `working_set_bytes` (kicp.h)"""
    out = C.c_double(0.0)
    _check(lib().kicp_probe_dependent_load(device, int(working_set_bytes), workgroups, block, steps, C.byref(out)))
    return out.value


def device_count():
    return lib().kicp_device_count()


def device_locality(device=0):
    """(NUMA node the GPU is attached to | -1, its CPUs as a set | empty) - kicp_device_locality"""
    node, buf = C.c_int(-1), C.create_string_buffer(4096)
    _check(lib().kicp_device_locality(device, C.byref(node), buf, len(buf)))
    cpus = set()
    for part in buf.value.decode().split(","):
        if part.strip():
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
    return node.value, cpus


def cpus_near_gpu(device=0, one_l3_domain=True):
    """CPUs to bind a process that drives `device` to: the GPU's NUMA node, narrowed to what the process may use and (by default) to
    ONE L3 domain of it - the calling thread and the library's helper threads then share a last-level cache.  Empty: unknown."""
    _, cpus = device_locality(device)
    cpus &= os.sched_getaffinity(0)
    if not cpus or not one_l3_domain:
        return cpus
    try:
        with open("/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list" % min(cpus)) as f:
            l3 = set()
            for part in f.read().strip().split(","):
                lo, _, hi = part.partition("-")
                l3.update(range(int(lo), int(hi or lo) + 1))
        return (cpus & l3) or cpus
    except OSError:
        return cpus


class DeviceFrame:
    """A scan resident in HBM (what an on-device pre-step would hand to the registration)."""

    _borrowed = False  # True: `ptr` belongs to someone else (PreSteps.frame) and is not freed here

    def __init__(self, points, device=0):
        a, _ = _d(points)
        self.n, self.device = a.size // 3, device
        self.ptr = C.c_void_p()
        _check(lib().kicp_device_malloc(device, max(a.nbytes, 8), C.byref(self.ptr)))
        if a.nbytes:
            _check(lib().kicp_device_upload(device, self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))

    @classmethod
    def _borrow(cls, ptr, n, device):
        """a view of `n` points at the device address `ptr` that frees nothing"""
        f = object.__new__(cls)
        f.n, f.device, f.ptr, f._borrowed = n, device, C.c_void_p(ptr), True
        return f

    def __del__(self):
        # Handle.__del__'s guard (a pointer is set, the library is loaded, once), and a borrowed frame frees nothing
        if getattr(self, "ptr", None) and _ffi._lib is not None and not self._borrowed:
            _ffi._lib.kicp_device_free(self.device, self.ptr)
            self.ptr = None


def comm_unique_id():
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().kicp_comm_unique_id(buf))
    return buf.raw
