"""Shapes and shifts for the scroll tests.  The kernel can go wrong at chunk and row boundaries, not at scale, so the shapes are small:
planes smaller than one 16-byte chunk, rows that are neither chunk multiples nor chunk aligned, and one of about a million cells, so
that there are more chunks than lanes in flight and the kernel's loop turns.  The shifts are the alignments of a chunk's source
against 16 bytes for elements of 1, 4 and 8 bytes, the last surviving row or column, and the shifts that empty the plane."""
import itertools

import numpy as np

SMALL = [(1, 1), (1, 7), (7, 1), (3, 5), (4, 4), (16, 3), (37, 29), (64, 2)]  # (width, height)
LARGE = (1031, 1027)


def axis_shifts(size):
    s = {0}
    for v in (1, 3, 4, 5, size - 1, size, size + 3):
        s.update((v, -v))
    return sorted(s)


def shifts(width, height):
    """every (dx, dy) of the two axes' sets on a small shape, a dozen pairs on the large one"""
    if (width, height) == LARGE:
        return [(1, 0), (0, 1), (-3, 5), (4, -4), (5, 3), (-1, -1), (64, 64), (width - 1, 0), (0, -(height - 1)), (-(width - 1), height - 1), (width, 1), (-3, height + 3)]
    return list(itertools.product(axis_shifts(width), axis_shifts(height)))


def counters(width, height, seed=0):
    """random 16-bit words with 0 and 65 535 among them -> uint16 (height, width, 2)"""
    rng = np.random.default_rng([seed, width, height])
    c = rng.integers(0, 65536, (height, width, 2), dtype=np.uint16)
    c[rng.random((height, width, 2)) < 0.1] = 0
    c[rng.random((height, width, 2)) < 0.1] = 65535
    c.flat[0], c.flat[-1] = 65535, 65535
    return c


def columns(width, height, seed=1):
    """random 64-bit words, bit 63 among them -> uint64 (height, width)"""
    rng = np.random.default_rng([seed, width, height])
    c = rng.integers(0, 1 << 64, (height, width), dtype=np.uint64)
    c.flat[0] |= np.uint64(1 << 63)
    c.flat[-1] = np.uint64((1 << 64) - 1)
    return c


def plane(width, height, elem_bytes, seed=2):
    """a random plane of 1, 2, 4 or 8 bytes per element, no element 0 (so that a zero in a result is the shift's)"""
    dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[elem_bytes]
    rng = np.random.default_rng([seed, width, height, elem_bytes])
    return rng.integers(1, 1 << (8 * elem_bytes), (height, width), dtype=dtype, endpoint=False)
