"""Affine maps as Render.transform_nodes and svo_nodes_transform take them (include/svo_hip.h): the counterpart of
orientation.py for free turns, scale and shear.

The pass wants the map it samples by, from scene cells to source cells, in Q16: q = floor(A (c + 1/2) + t) for the scene cell c.
A caller thinks the other way round: "turn the model by F about this point of it, and put that point there".  fixed() inverts
that in float64 and rounds to Q16 once, the matrix first and the translation by the rounded matrix, so that the chosen point
stays where it was put; everything behind it is integers.  Points are in cells, a cell's centre at its index
plus 1/2 on every axis.
"""
import math

import numpy as np

from .orientation import PERMS

ONE = 1 << 16          # Q16
MAX_ENTRY = 1 << 20    # |matrix[i][j]| <= 2^20: a factor of 16
MAX_TRANSLATE = 1 << 40


def rotation(axis, degrees):
    """the 3 x 3 matrix of a turn by `degrees`, counter-clockwise seen against the axis: "x", "y", "z" or any vector"""
    v = np.array({"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1)}.get(axis, axis) if isinstance(axis, str) else axis, dtype=np.float64)
    if v.shape != (3,) or not np.linalg.norm(v) > 0:
        raise ValueError(f"axis must be 'x', 'y', 'z' or a vector of three numbers, not all zero (got {axis!r})")
    x, y, z = v / np.linalg.norm(v)
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    k = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + s * k + (1 - c) * (k @ k)


def scale(sx, sy=None, sz=None):
    """the diagonal matrix; a factor left out is sx's"""
    return np.diag([float(sx), float(sx if sy is None else sy), float(sx if sz is None else sz)])


def compose(*maps):
    """the product of 3 x 3 matrices: compose(a, b) applies b first, then a"""
    out = np.eye(3)
    for m in maps:
        m = np.asarray(m, dtype=np.float64)
        if m.shape != (3, 3):
            raise ValueError("every map must be 3 x 3")
        out = out @ m
    return out


def whole_numbers(values, what):
    """`values` as a flat list of Python ints; ValueError for a value that is no whole number, so that a float matrix handed
    over by mistake (rotation()'s, say, where fixed()'s Q16 was meant) is not cut down to 0 and +-1 in silence"""
    out = []
    for v in np.asarray(values, dtype=object).reshape(-1).tolist():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v or v in (math.inf, -math.inf) or v != int(v):
            raise ValueError(f"{what} must hold whole numbers in Q16 (transform.fixed makes them), got {v!r}")
        out.append(int(v))
    return out


def _checked(matrix, translate):
    matrix, translate = whole_numbers(matrix, "matrix"), whole_numbers(translate, "translate")
    if len(matrix) != 9 or len(translate) != 3:
        raise ValueError("matrix must hold 9 numbers and translate 3")
    if any(abs(v) > MAX_ENTRY for v in matrix):
        raise ValueError(f"a matrix entry lies outside [-2^20, 2^20] (a factor of 16): {matrix}")
    if any(abs(v) > MAX_TRANSLATE for v in translate):
        raise ValueError(f"a translation lies outside [-2^40, 2^40]: {translate}")
    return matrix, translate


def fixed(forward, about_scene, about_source):
    """-> (matrix, translate), 9 and 3 Python ints in Q16: the inverse of "turn / scale / shear the source by the 3 x 3 matrix
    `forward` about its point about_source, and put that point on the scene's point about_scene".  A source point p lands on
    forward (p - about_source) + about_scene, so a scene point c samples the source at A (c - about_scene) + about_source with
    A = forward^-1.  Raises ValueError for a singular `forward` and for numbers outside the pass's range."""
    f = np.asarray(forward, dtype=np.float64)
    if f.shape != (3, 3):
        raise ValueError("forward must be 3 x 3")
    try:
        a = np.linalg.inv(f)
    except np.linalg.LinAlgError:
        raise ValueError("forward is singular: it has no inverse to sample by") from None
    # the translation from the rounded matrix, so that about_scene samples about_source whatever the rounding did to A: an
    # entry's error of 2^-17 times a coordinate of 2^21 would move the source by 16 cells
    a = np.rint(a * ONE)
    if np.abs(a).max() > MAX_ENTRY:
        raise ValueError(f"a matrix entry lies outside [-2^20, 2^20] (a factor of 16): {a.astype(np.int64).reshape(-1).tolist()}")
    t = np.asarray(about_source, dtype=np.float64) - (a / ONE) @ np.asarray(about_scene, dtype=np.float64)
    return _checked(a.astype(np.int64), np.rint(t * ONE).astype(np.int64))


def from_orientation(orient, offset=(0, 0, 0), src_depth=1):
    """-> (matrix, translate): Render.place_nodes' map, one of the cube's 48 symmetries (orientation.py) and a whole-cell
    offset.  matrix[perm[i]][i] = f_i ? -1 : 1 and translate[perm[i]] = f_i ? S + offset_i : -offset_i, in Q16."""
    orient = int(orient)
    if not 0 <= orient < 48:
        raise ValueError(f"orient must be 0..47 (got {orient})")
    if len(offset) != 3:
        raise ValueError(f"offset must be three cell coordinates, got {offset!r}")
    perm, side = PERMS[orient >> 3], 1 << int(src_depth)
    matrix, translate = [0] * 9, [0] * 3
    for i in range(3):
        flip = orient >> (2 - i) & 1
        matrix[3 * perm[i] + i] = -ONE if flip else ONE
        translate[perm[i]] = ONE * (side + int(offset[i]) if flip else -int(offset[i]))
    return _checked(matrix, translate)


def source_cell(matrix, translate, cells):
    """the source cell q that every scene cell of `cells` ((..., 3) integers, a numpy array or a torch tensor) samples, by the
    header's rule in int64: P_i = sum_j matrix[i][j] (2 c_j + 1) + 2 translate[i], q_i = P_i >> 17.  -> the same kind of array,
    int64; a q outside [0, 2^src_depth)^3 samples nothing."""
    matrix, translate = _checked(matrix, translate)
    if hasattr(cells, "detach"):  # a torch tensor: stays on its device
        import torch
        c = 2 * cells.to(torch.int64) + 1
        m = torch.tensor(matrix, dtype=torch.int64, device=cells.device).reshape(3, 3)
        t = torch.tensor(translate, dtype=torch.int64, device=cells.device)
        return ((c.unsqueeze(-2) * m).sum(-1) + 2 * t) >> 17
    c = 2 * np.asarray(cells, dtype=np.int64) + 1
    return (c @ np.array(matrix, dtype=np.int64).reshape(3, 3).T + 2 * np.array(translate, dtype=np.int64)) >> 17
