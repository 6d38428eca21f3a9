"""Restatements of the solid voxeliser's contract (csrc/svo_solid.hip) in Python integers.

covers(), height()      the contract's per-triangle quantities for one column: the covering test with the tie rule, and k
inside_by_fractions()   the definition: a real generic point in fractions.Fraction (the centre moved by dy = 2^-100,
                        dx = 2^-300, dz = 2^-900), plain strict tests, the triangles above it counted
square_overlaps()       the 2D separating-axis test of one projected triangle and one closed square
refine()                the level refinement over arrays, with every level's pair count: this is what the device counts
solid()                 crossings, both rules, spans, cells and open columns of a mesh: what the device must give, bit for bit

All coordinates are the contract's doubled units: a vertex is 2 q + 1 (odd), a cell c spans [128 c, 128 (c + 1)] and its
centre is 128 c + 64."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

SUBBITS = 6
EVENODD, NONZERO, SPANS = 0, 1, 2
Stopped = namedtuple("Stopped", "level count")  # solid() with max_pairs: the first level whose pair count passes it
Solid = namedtuple("Solid", "spans cells n_open crossings")
DY, DX, DZ = Fraction(1, 1 << 100), Fraction(1, 1 << 300), Fraction(1, 1 << 900)


def sign(v):
    return (v > 0) - (v < 0)


def doubled(vq, triangles):
    """(t, 3 vertices, 3 axes) int64: the triangles' vertices 2 q + 1"""
    vq = np.asarray(vq, dtype=np.int64).reshape(-1, 3)
    tris = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    assert tris.size == 0 or (tris.min() >= 0 and tris.max() < len(vq))
    return (2 * vq + 1)[tris]


def normal(V):
    e0, e1 = [V[1][a] - V[0][a] for a in range(3)], [V[2][a] - V[1][a] for a in range(3)]
    return [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]


def covers(V, cx, cz):
    """whether triangle V (three vertices of three Python ints) covers the column (cx, cz), by the contract's rule"""
    ny = normal(V)[1]
    if ny == 0:
        return False
    s, Cx, Cz = sign(-ny), 128 * cx + 64, 128 * cz + 64
    for i in range(3):
        ex, ez = V[(i + 1) % 3][0] - V[i][0], V[(i + 1) % 3][2] - V[i][2]
        F = ex * (Cz - V[i][2]) - ez * (Cx - V[i][0])
        assert abs(F) < 1 << 57
        sgn = sign(F) if F else sign(-ez) if ez else sign(ex)
        if s * sgn <= 0:
            return False
    return True


def height(V, cx, cz, depth, widths=None):
    """k: the number of cy in [0, 2^depth) whose centre the triangle's plane crosses above, each cy by the sign test"""
    n = normal(V)
    k = 0
    for cy in range(1 << depth):
        C = (128 * cx + 64, 128 * cy + 64, 128 * cz + 64)
        D = sum(n[a] * (C[a] - V[0][a]) for a in range(3))
        if widths is not None:
            widths["plane_bits"] = max(widths.get("plane_bits", 0), abs(D).bit_length())
        above = D != 0 and sign(D) != sign(n[1])
        assert above or k <= cy  # monotone: a prefix
        if above:
            assert k == cy
            k = cy + 1
    return k


def height_closed_form(V, cx, cz, depth):
    """k without the loop: sign(n.y) D(cy) = b + m cy with m = 128 |n.y|, so k = clamp(ceil(-b / m), 0, 2^depth)"""
    n = normal(V)
    a = n[0] * (128 * cx + 64 - V[0][0]) + n[2] * (128 * cz + 64 - V[0][2]) + n[1] * (64 - V[0][1])
    b, m = sign(n[1]) * a, 128 * abs(n[1])
    return 0 if b >= 0 else min(1 << depth, (-b + m - 1) // m)


def inside_by_fractions(Vs, cell, rule):
    """the definition: the triangles that a ray from the generic point of `cell` towards +y crosses, counted by `rule`"""
    P = (128 * cell[0] + 64 + DX, 128 * cell[1] + 64 + DY, 128 * cell[2] + 64 + DZ)
    count = total = 0
    for V in Vs:
        n = normal(V)
        if n[1] == 0:
            continue
        side = []
        for i in range(3):
            ex, ez = V[(i + 1) % 3][0] - V[i][0], V[(i + 1) % 3][2] - V[i][2]
            F = ex * (P[2] - V[i][2]) - ez * (P[0] - V[i][0])
            assert F != 0  # generic
            side.append(F > 0)
        if side[0] != side[1] or side[1] != side[2]:
            continue
        y = V[0][1] - (n[0] * (P[0] - V[0][0]) + n[2] * (P[2] - V[0][2])) / Fraction(n[1])
        assert y != P[1]
        if y > P[1]:
            count += 1
            total += sign(n[1])
    return bool(total) if rule == NONZERO else bool(count & 1)


def square_overlaps(V, lo, S):
    """the closed projected triangle of V against the closed square [lo, lo + S]^2 in (x, z): 2 box axes, 3 edge normals,
    every comparison strict; for a triangle with n.y != 0"""
    h = S // 2
    u = [(V[j][0] - lo[0] - h, V[j][2] - lo[1] - h) for j in range(3)]
    for a in range(2):
        if min(p[a] for p in u) > h or max(p[a] for p in u) < -h:
            return False
    for i in range(3):
        ex, ez = u[(i + 1) % 3][0] - u[i][0], u[(i + 1) % 3][1] - u[i][1]
        p = [ex * q[1] - ez * q[0] for q in u]
        r = h * (abs(ex) + abs(ez))
        if min(p) > r or max(p) < -r:
            return False
    return True


CHILDREN = np.array([[c >> 1 & 1, c & 1] for c in range(4)], dtype=np.int64)


def _overlaps_many(V, lo, S):
    """square_overlaps over arrays: V (n, 3, 3) int64, lo (n, 2)"""
    h = S // 2
    u = V[:, :, [0, 2]] - (lo + h)[:, None, :]
    e = np.roll(u, -1, axis=1) - u
    assert 2 * int(np.abs(e).max(initial=0)) * max(int(np.abs(u).max(initial=0)), h) < 1 << 62
    ok = ~((u.min(axis=1) > h) | (u.max(axis=1) < -h)).any(axis=1)
    for i in range(3):
        p = e[:, i, 0, None] * u[:, :, 1] - e[:, i, 1, None] * u[:, :, 0]
        r = h * (np.abs(e[:, i, 0]) + np.abs(e[:, i, 1]))
        ok &= ~((p.min(axis=1) > r) | (p.max(axis=1) < -r))
    return ok


def _covers_many(V, col):
    """covers() over arrays: V (n, 3, 3) int64 with n.y != 0, col (n, 2) columns"""
    e = np.roll(V, -1, axis=1) - V
    ny = e[:, 0, 2] * e[:, 1, 0] - e[:, 0, 0] * e[:, 1, 2]
    s = np.sign(-ny)
    C = 128 * col + 64
    ok = np.ones(len(V), dtype=bool)
    for i in range(3):
        ex, ez = e[:, i, 0], e[:, i, 2]
        F = ex * (C[:, 1] - V[:, i, 2]) - ez * (C[:, 0] - V[:, i, 0])
        sgn = np.where(F != 0, np.sign(F), np.where(ez != 0, -np.sign(ez), np.sign(ex)))
        ok &= s * sgn > 0
    return ok


def refine(V, depth, max_pairs=None, levels=None):
    """The (triangle, column) pairs of the last level that cover, as (t, col (n, 2)), refined level by level from one pair
    per triangle that is not edge-on; levels (a list) gets every level's pair count (the last level's: the crossings).
    max_pairs: Stopped(level, count) at the first level that passes it."""
    e = np.roll(V, -1, axis=1) - V
    ny = e[:, 0, 2] * e[:, 1, 0] - e[:, 0, 0] * e[:, 1, 2] if len(V) else np.zeros(0, dtype=np.int64)
    t = np.flatnonzero(ny != 0)
    sq = np.zeros((len(t), 2), dtype=np.int64)
    for level in range(1, depth + 1):
        S = 1 << (depth - level + 7)
        t = np.repeat(t, 4)
        sq = (sq[:, None, :] * 2 + CHILDREN[None, :, :]).reshape(-1, 2)
        keep = _covers_many(V[t], sq) if level == depth else _overlaps_many(V[t], sq * S, S)
        t, sq = t[keep], sq[keep]
        if levels is not None:
            levels.append(len(t))
        if max_pairs is not None and len(t) > max_pairs:
            return Stopped(level, len(t))
    return t, sq


def _heights(V, col, depth):
    """height_closed_form over arrays, in Python ints (object arrays): the plane's products pass 64 bits"""
    O = V.astype(object)
    e0, e1 = O[:, 1] - O[:, 0], O[:, 2] - O[:, 1]
    n = [e0[:, (a + 1) % 3] * e1[:, (a + 2) % 3] - e0[:, (a + 2) % 3] * e1[:, (a + 1) % 3] for a in range(3)]
    C = (128 * col + 64).astype(object)
    a = n[0] * (C[:, 0] - O[:, 0, 0]) + n[2] * (C[:, 1] - O[:, 0, 2]) + n[1] * (64 - O[:, 0, 1])
    k = np.zeros(len(V), dtype=np.int64)
    w = np.zeros(len(V), dtype=np.int64)
    for i in range(len(V)):
        ny = int(n[1][i])
        b, m = sign(ny) * int(a[i]), 128 * abs(ny)
        k[i] = 0 if b >= 0 else min(1 << depth, (-b + m - 1) // m)
        w[i] = sign(ny)
    return k, w


def column_spans(ks, ws, rule):
    """the maximal runs of inside cells of one column from its crossings' heights and signs, each cell by the rule itself,
    evaluated at the first cell of every stretch between two distinct heights; and whether the column is open"""
    ks, ws = np.asarray(ks), np.asarray(ws)

    def inside(cy):
        above = ks > cy
        return bool(ws[above].sum()) if rule == NONZERO else bool(above.sum() & 1)

    runs, prev = [], 0
    for k in sorted(set(ks.tolist())):
        if k > prev and inside(prev):
            if runs and runs[-1][1] == prev:
                runs[-1][1] = k
            else:
                runs.append([prev, k])
        prev = max(prev, k)
    return runs, inside(-1)


def solid(vq, triangles, depth, rule=EVENODD, max_pairs=None, levels=None):
    """Solid(spans (N, 4) uint32 of (x, z, y0, y1) ascending in (x, z, y0), cells (M, 3) uint32 of (x, y, z) ascending in
    (x, z, y), the number of open columns, the number of crossings), or Stopped."""
    vq = np.asarray(vq, dtype=np.int64).reshape(-1, 3)
    assert 1 <= depth <= 21 and (vq.size == 0 or (vq.min() >= 0 and vq.max() < 1 << (depth + SUBBITS)))
    V = doubled(vq, triangles)
    got = refine(V, depth, max_pairs, levels)
    if isinstance(got, Stopped):
        return got
    t, col = got
    k, w = _heights(V[t], col, depth)
    order = np.lexsort((k, col[:, 1], col[:, 0]))
    col, k, w = col[order], k[order], w[order]
    spans, n_open = [], 0
    heads = np.flatnonzero(np.r_[True, (np.diff(col, axis=0) != 0).any(axis=1)]) if len(col) else np.zeros(0, dtype=np.int64)
    for s, e in zip(heads, np.r_[heads[1:], len(col)]):
        runs, is_open = column_spans(k[s:e], w[s:e], rule)
        n_open += is_open
        spans += [(int(col[s, 0]), int(col[s, 1]), y0, y1) for y0, y1 in runs]
    spans = np.array(spans, dtype=np.int64).reshape(-1, 4)
    length = spans[:, 3] - spans[:, 2]
    which = np.repeat(np.arange(len(spans)), length)
    y = spans[which, 2] + np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length)
    cells = np.stack([spans[which, 0], y, spans[which, 1]], axis=1)
    return Solid(spans.astype(np.uint32), cells.astype(np.uint32), int(n_open), len(t))


def cells_brute(vq, triangles, depth, rule=EVENODD, by=None):
    """every cell of the grid against every triangle: the set of inside cells, with covers() and height() (or with
    by=inside_by_fractions, the definition)"""
    Vs = [[[int(x) for x in p] for p in tri] for tri in doubled(vq, triangles)]
    side, out = 1 << depth, set()
    for cx in range(side):
        for cz in range(side):
            if by is not None:
                out |= {(cx, cy, cz) for cy in range(side) if by(Vs, (cx, cy, cz), rule)}
                continue
            cover = [V for V in Vs if covers(V, cx, cz)]
            ks = [height(V, cx, cz, depth) for V in cover]
            ws = [sign(normal(V)[1]) for V in cover]
            for cy in range(side):
                above = [w for k, w in zip(ks, ws) if k > cy]
                if (sum(above) != 0) if rule == NONZERO else len(above) & 1:
                    out.add((cx, cy, cz))
    return out
