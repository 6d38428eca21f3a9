"""Shapes for Render.edit_region (svo_nodes_edit_region): boxes and balls that fill, carve or paint a tree in
the node buffer.  A shape applies to the cells inside it whose state its mode names: EMPTY cells, VOXELS, or both (SET:
a fill with colour != 0, a carve with colour 0).  Shapes are applied in the order they are given.

    box(lo, hi, colour, mode=SET)            the cells lo <= c < hi, in cells of the edit's grid; clipped to the grid
    ball(centre, radius, colour, mode=SET)   the cells whose centre lies within `radius` of `centre`; both in cells, whole
                                             or n + 0.5 (cell c has its centre at c + 0.5); everything is integer from here on
"""
import ctypes as C
from collections import namedtuple

from ._lib import RegionShape

BOX, BALL = 0, 1
EMPTY, VOXELS, SET = 1, 2, 3
MAX_SHAPES = 1024

Shape = namedtuple("Shape", "kind mode colour a b")


def _mode(mode):
    if mode not in (EMPTY, VOXELS, SET):
        raise ValueError(f"mode must be EMPTY (1), VOXELS (2) or SET (3), got {mode!r}")
    return int(mode)


def _halves(v, what):
    """a length in cells, whole or n + 0.5, as half cells"""
    h = 2 * v
    if h != int(h) or h < 0:
        raise ValueError(f"{what} must be a whole number of cells or n + 0.5, not negative (got {v!r})")
    return int(h)


def box(lo, hi, colour, mode=SET):
    lo, hi = list(lo), list(hi)
    if len(lo) != 3 or len(hi) != 3 or any(int(v) != v for v in lo + hi):
        raise ValueError(f"a box takes two corners of 3 whole cells each (got {lo} and {hi})")
    return Shape(BOX, _mode(mode), int(colour) & 0xFFFFFF, tuple(int(v) for v in lo), tuple(int(v) for v in hi))


def ball(centre, radius, colour, mode=SET):
    centre = list(centre)
    if len(centre) != 3:
        raise ValueError(f"a ball's centre has 3 coordinates (got {centre})")
    c2 = tuple(_halves(v, "a ball's centre") for v in centre)
    return Shape(BALL, _mode(mode), int(colour) & 0xFFFFFF, c2, (_halves(radius, "a ball's radius"), 0, 0))


def pack(shapes, depth):
    """(the svo_region_shape array, its length) of `shapes` on the depth grid: boxes clipped to [0, 2^depth), empty ones dropped"""
    side = 1 << max(0, min(int(depth), 21))
    out = []
    for s in shapes:
        if not isinstance(s, Shape):
            raise TypeError(f"edit_region takes region.box(...) and region.ball(...) shapes, got {type(s).__name__}")
        a, b = s.a, s.b
        if s.kind == BOX:
            a, b = tuple(max(0, v) for v in a), tuple(min(side, v) for v in b)
            if any(lo >= hi for lo, hi in zip(a, b)):
                continue
        elif max(a + b) >= 1 << 32:
            raise ValueError(f"a ball's centre and radius must be below 2^31 cells (got {s})")
        out.append((s.kind, s.mode, s.colour, a, b))
    arr = (RegionShape * max(len(out), 1))()
    for r, (kind, mode, colour, a, b) in zip(arr, out):
        r.kind, r.mode, r.colour, r.a, r.b = kind, mode, colour, (C.c_uint32 * 3)(*a), (C.c_uint32 * 3)(*b)
    return arr, len(out)
