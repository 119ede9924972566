"""What every feature module of the binding shares: the library and when it is loaded, the table of its entries' signatures, the error
type, the conversions from arrays to typed pointers, the base of the classes that own a handle of the library, and the marshalling
that several features repeat (a frame entry's arguments, info(), last_window(), the checks of an array argument)."""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkicp_amd.so")

KICP_OK = 0
KICP_WARN_NO_CORRESPONDENCES = 1
KICP_WARN_TABLE_ORDER = 2
KICP_ERR_HIP, KICP_ERR_ARG, KICP_ERR_CAPACITY, KICP_ERR_COMM, KICP_ERR_INTERNAL = -1, -2, -3, -4, -5


class KicpError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("kicp error %d: %s" % (code, message))
        self.code = code


_dp = C.POINTER(C.c_double)
_i8p, _u8p, _u16p, _u32p, _u64p = (C.POINTER(t) for t in (C.c_byte, C.c_ubyte, C.c_ushort, C.c_uint, C.c_ulonglong))
_i64p, _intp, _szp, _hp = (C.POINTER(t) for t in (C.c_longlong, C.c_int, C.c_size_t, C.c_void_p))

# The loaded library, None until lib() first runs.  Read it as `_ffi._lib`: a `from ._ffi import _lib` copies the None of import time.
_lib = None

# every symbol include/kicp.h declares: (restype, argtypes).  Each feature module adds the entries it calls through _declare().
_SIGNATURES = {}


def _declare(entries):
    """add a module's entries to the table lib() applies -> `entries`; a name declared twice is an error at import"""
    twice = sorted(set(entries) & set(_SIGNATURES))
    if twice:
        raise ImportError("declared by two modules of kinematic_icp_amd: %s" % ", ".join(twice))
    if _lib is not None:
        raise ImportError("the library is loaded: %s can no longer be declared" % ", ".join(sorted(entries)))
    _SIGNATURES.update(entries)
    return entries


_ENTRIES = _declare({
    "kicp_last_error": (C.c_char_p, []),
    "kicp_version": (C.c_int, []),
})


def lib():
    """Load libkicp_amd.so (once).  Fails loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        path = getattr(sys.modules.get(__package__), "LIB_PATH", LIB_PATH)  # the package's name for it: a tool may point it at another build first
        if not os.path.exists(path):
            raise KicpError(KICP_ERR_HIP, "HIP extension %s not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                                          "or `make -C kinematic_icp_amd/csrc`); there is no CPU fallback" % path)
        L = C.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise KicpError(rc, lib().kicp_last_error().decode(errors="replace"))
    return rc


class Handle:
    """An object of the library behind a void*: the one place that says how `_h` is made and when a Python object may still destroy
    it.  A subclass names its destroy entry and makes its handle with _create (in __init__) or _from (clone, load)."""

    _destroy = None  # the entry's name, kicp_*_destroy

    def _create(self, entry, *args, tail=()):
        """self._h = the handle lib().<entry>(*args, &handle, *tail) makes; it is None while that fails, so what is left frees nothing"""
        self._h = None
        h = C.c_void_p()
        _check(getattr(lib(), entry)(*args, C.byref(h), *tail))
        self._h = h

    @classmethod
    def _from(cls, entry, *args, tail=()):
        """an object of cls around the handle `entry` makes, without cls.__init__"""
        obj = object.__new__(cls)
        obj._create(entry, *args, tail=tail)
        return obj

    def __del__(self):
        # a handle is set, the library is loaded (never load it from here: at interpreter exit the module may be half gone), once
        if getattr(self, "_h", None) and _lib is not None:
            getattr(_lib, self._destroy)(self._h)
            self._h = None


def _d(a):
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
        a = np.ascontiguousarray(a, dtype=np.float64)
    return a, C.cast(a.ctypes.data, _dp)


# Small arrays that come back call after call (poses): their ctypes pointer is built once.  The cache holds a reference
# to the array, so its address - and the id() used as the key - stays valid; it is only used for arrays of at most 16
# doubles and is bounded.
_PTR_CACHE = {}


def _pose_ptr(a):
    hit = _PTR_CACHE.get(id(a))
    if hit is not None and hit[0] is a:
        return hit[1]
    arr, ptr = _d(a)
    if arr is a and arr.size <= 16:
        if len(_PTR_CACHE) >= 256:
            _PTR_CACHE.clear()
        _PTR_CACHE[id(a)] = (a, ptr)
    elif arr is not a:
        ptr._keep = arr  # a converted temporary must outlive the call
    return ptr


def _u8(a):
    return a.ctypes.data_as(_u8p)


def _u16(a):
    return a.ctypes.data_as(_u16p)


def _u32(a):
    return a.ctypes.data_as(_u32p)


def _u64(a):
    return a.ctypes.data_as(_u64p)


def _i8(a):
    return a.ctypes.data_as(_i8p)


def _frame_args(pose, sensor_xyz, frame=None, device_frame=None, n=None):
    """the arguments of a frame entry after its handle -> (points | None for none, their number, pose, sensor): `frame` is host
    memory, `device_frame` a DeviceFrame (or anything with .ptr and .n) of whose points `n` count (None: all).  The pointers keep
    the arrays they point into alive."""
    if device_frame is None:
        a, p = _d(np.asarray(frame, dtype=np.float64).reshape(-1, 3))
        p._keep, count = a, a.size // 3
    else:
        p, count = device_frame.ptr, device_frame.n if n is None else int(n)
    s, sp = _d(np.asarray(sensor_xyz, dtype=np.float64).reshape(3))
    sp._keep = s
    return p if count else None, count, _pose_ptr(pose), sp


def _info(entry, h, cfg, **outputs):
    """kicp_*_info -> dict: the fields of the configuration `cfg` and the trailing outputs by name, each a ctypes scalar (the dict
    gets its value) or a float64 array"""
    refs = [v.ctypes.data_as(_dp) if isinstance(v, np.ndarray) else C.byref(v) for v in outputs.values()]
    _check(getattr(lib(), entry)(h, C.byref(cfg), *refs))
    out = {name: getattr(cfg, name) for name, _ in cfg._fields_}
    out.update((name, v if isinstance(v, np.ndarray) else v.value) for name, v in outputs.items())
    return out


def _last_window(entry, h):
    """kicp_*_last_window -> (x0, y0, w, h) as a tuple of int"""
    v = [C.c_uint() for _ in range(4)]
    _check(getattr(lib(), entry)(h, *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def _out_array(out, shape, dtype, what):
    """the array a result is written into: `out` (of `dtype`, C-contiguous, of `shape`) or a new one"""
    if out is None:
        return np.empty(shape, dtype=dtype)
    if not isinstance(out, np.ndarray) or out.dtype != dtype or out.shape != tuple(shape) or not out.flags.c_contiguous or not out.flags.writeable:
        raise KicpError(KICP_ERR_ARG, "out must be a writeable C-contiguous %s array shaped %s" % (np.dtype(dtype).name, what))
    return out


def _rect(rect, width, height):
    """(x0, y0, w, h) of `rect`, the full grid for None; negative numbers are passed as something the library refuses"""
    x0, y0, w, h = (0, 0, width, height) if rect is None else (int(v) for v in rect)
    if min(x0, y0, w, h) < 0:
        raise KicpError(KICP_ERR_ARG, "the rectangle (x0, y0, w, h) must not be negative")
    return x0, y0, w, h


def _occupancy_2d(occupancy):
    occ = np.ascontiguousarray(occupancy, dtype=np.int8)
    if occ.ndim != 2 or occ.size == 0:
        raise KicpError(KICP_ERR_ARG, "occupancy must be shaped (height, width), both at least 1")
    return occ
