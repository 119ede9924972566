"""kicp_pre_download_begin_into (kicp_pre_egress.hip): the handle's copy worker moves a buffer into caller memory while the caller
goes on.  No other test calls the entry; the chained frame (PreSteps.Frame, the facade) enters only the worker's third mode, the
pieces a kernel pushes.  Here: the one-event mode (a transfer below 1 MiB), the pieces mode (1 MiB and more: 43 691 points of
24 bytes), a landing area smaller than the buffer, and a download that nobody collected before the next one began.  The reference
is kicp_pre_download of the same buffer: the very same bytes."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)


def _begin_into(pre, buffer, out, cap):
    rc = K.lib().kicp_pre_download_begin_into(pre._h, buffer, out.ctypes.data_as(_dp), cap)
    assert rc == 0, K.lib().kicp_last_error()


def _finish(pre, buffer, out, cap):
    n = C.c_size_t()
    rc = K.lib().kicp_pre_download_finish(pre._h, buffer, out.ctypes.data_as(_dp), cap, C.byref(n))
    assert rc == 0, K.lib().kicp_last_error()
    return n.value


@pytest.mark.parametrize("n", [300, 44032])  # 7 200 bytes: one event; 1 056 768 bytes: three pieces of 352 256, 352 256 and 352 256
def test_download_into_matches_download(n):
    pre = K.PreSteps()
    pts = np.random.default_rng(n).normal(size=(n, 3))
    pre.upload(1, pts)
    want = pre.download(1)
    assert np.array_equal(want, pts)
    out = np.full((n, 3), np.nan)
    _begin_into(pre, 1, out, n)
    assert _finish(pre, 1, out, n) == n      # (the worker delivered into `out`: _finish only joins it)
    assert np.array_equal(out, want)
    # a landing area of fewer points than the buffer holds: those points and not a byte more; the count reported is the buffer's
    cap = n - 7
    small = np.full((n, 3), np.nan)
    _begin_into(pre, 1, small, cap)
    assert _finish(pre, 1, small, cap) == n
    assert np.array_equal(small[:cap], want[:cap]) and np.isnan(small[cap:]).all()
    # collected into ANOTHER array than the one the worker filled: _finish copies from the landing area
    other = np.full((n, 3), np.nan)
    _begin_into(pre, 1, out, n)
    assert _finish(pre, 1, other, n) == n
    assert np.array_equal(other, want)


def test_uncollected_download_then_the_next_one():
    """A download nobody collected, then the next one begins: the earlier job and its transfer finish first, the later one's result
    is what _finish hands over - on the worker's path and on the plain one."""
    pre = K.PreSteps()
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=(44032, 3)), rng.normal(size=(300, 3))
    pre.upload(0, a), pre.upload(2, b)
    first, second = np.full(a.shape, np.nan), np.full(b.shape, np.nan)
    _begin_into(pre, 0, first, len(a))       # never collected
    _begin_into(pre, 2, second, len(b))
    assert np.array_equal(first, a)          # (settled before the second one began)
    rc = K.lib().kicp_pre_download_finish(pre._h, 0, None, 0, None)
    assert rc == K.KICP_ERR_ARG              # buffer 0's download is no longer the one in flight
    assert _finish(pre, 2, second, len(b)) == len(b)
    assert np.array_equal(second, b)
    _begin_into(pre, 0, first, len(a))       # left to the next plain download ...
    pre.download_begin(2)
    assert np.array_equal(pre.download_finish(2), b)
    pre.download_begin(0)                    # ... and a handle destroyed with a job out and uncollected
    _begin_into(pre, 2, second, len(b))
    del pre
