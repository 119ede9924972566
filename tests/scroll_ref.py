"""The scroll restated from include/kicp.h's text: the shift of a plane (a zero array and one slice assignment), the origin after a
shift (two rounded operations on Python floats) and the follow rule (Python integers).  Nothing of the library is called here."""
import math

import numpy as np


def shift(plane, dx, dy):
    """out[iy, ix] = plane[iy + dy, ix + dx] where that lies inside, 0 elsewhere; trailing axes (the counter pair) ride along"""
    p = np.asarray(plane)
    h, w = p.shape[:2]
    out = np.zeros_like(p)
    if abs(dx) < w and abs(dy) < h:
        out[max(-dy, 0):h - max(dy, 0), max(-dx, 0):w - max(dx, 0)] = p[max(dy, 0):h - max(-dy, 0), max(dx, 0):w - max(-dx, 0)]
    return out


def origin(origin, d, cell):
    """origin + (double)d * cell: the product is rounded, then the sum (Python floats never fuse)"""
    step = float(d) * float(cell)
    return float(origin) + step


def follow_shift(c, size, margin, step):
    """the shift along one axis that brings cell c into [margin, size - margin); None where the rule refuses its arguments"""
    if margin < 1 or step < 1 or 2 * margin + step > size:
        return None
    if c < margin:
        return -step * -(-(margin - c) // step)
    if c >= size - margin:
        return step * -(-(c - (size - margin) + 1) // step)
    return 0


def cell_of(x, origin, cell):
    """the grid's own arithmetic: floor((x - origin) / cell)"""
    return math.floor((float(x) - float(origin)) / float(cell))


def follow(x, y, origin_x, origin_y, cell, width, height, margin, step):
    """(dx, dy) kicp_grid_follow applies for the world position (x, y)"""
    return (follow_shift(cell_of(x, origin_x, cell), width, margin, step), follow_shift(cell_of(y, origin_y, cell), height, margin, step))


def window(x0, y0, side, dx, dy, width, height):
    """the unclipped window (x0, y0, side, side) translated by (-dx, -dy) and clipped as kicp_grid_last_window does -> (x0, y0, w, h)"""
    ax, bx = max(x0 - dx, 0), min(x0 - dx + side, width)
    ay, by = max(y0 - dy, 0), min(y0 - dy + side, height)
    return (0, 0, 0, 0) if ax >= bx or ay >= by else (ax, ay, bx - ax, by - ay)


def leaving_strips(dx, dy, width, height):
    """the two rectangles (x0, y0, w, h) of cells that leave under a scroll by (dx, dy), |dx| < width and |dy| < height: the columns over
    all rows, then the rows over the remaining columns; a strip of no cells is None"""
    cols = None if dx == 0 else (0 if dx > 0 else width + dx, 0, abs(dx), height)
    keep_x0, keep_w = (max(dx, 0), width - abs(dx))
    rows = None if dy == 0 else (keep_x0, 0 if dy > 0 else height + dy, keep_w, abs(dy))
    return cols, rows
