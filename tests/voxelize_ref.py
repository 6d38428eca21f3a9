"""Restatements of the mesh voxeliser's contract (csrc/svo_voxelize.hip).  The rule is stated twice:

overlaps_by_clipping()  the definition: the closed triangle clipped by the closed cube's six half-spaces (Sutherland-Hodgman)
                        in fractions.Fraction; an entry exists iff something is left
overlaps()              the integer test of the contract for one triangle and one box in Python ints: 13 separating axes,
                        every comparison strict
overlaps_many()         the same test over arrays: int64 for the box and edge axes (with the assertion that every term
                        stays below 2^62), Python ints in object arrays for the plane, whose products pass 64 bits
voxelize()              the level refinement over overlaps_many: one pair per triangle at the root, the 8 children of every
                        pair tested level by level, kept in input order; this is the list the device must give, bit for bit

All coordinates here are the contract's doubled units: a vertex is 2 q + 1 (odd), a level-l cell c spans [c S, (c + 1) S]
with S = 2^(depth - l + 7) (even bounds)."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

SUBBITS = 6
Stopped = namedtuple("Stopped", "level count")  # voxelize() with a cap: the first level whose pair count passes it


def overlaps_by_clipping(V, lo, S):
    """V: three vertices (3 ints each), the box [lo, lo + S]^3 componentwise"""
    poly = [tuple(Fraction(x) for x in p) for p in V]
    for a in range(3):
        for bound, keep in ((Fraction(lo[a]), lambda x, b: x >= b), (Fraction(lo[a] + S), lambda x, b: x <= b)):
            out = []
            for k in range(len(poly)):
                P, Q = poly[k - 1], poly[k]
                p_in, q_in = keep(P[a], bound), keep(Q[a], bound)
                if p_in != q_in:
                    t = (bound - P[a]) / (Q[a] - P[a])
                    out.append(tuple(P[i] + t * (Q[i] - P[i]) for i in range(3)))
                if q_in:
                    out.append(Q)
            poly = out
            if not poly:
                return False
    return True


def overlaps(V, lo, S):
    """the 13-axis test in Python ints; S even, the box [lo, lo + S]^3"""
    h = S // 2
    u = [[V[j][a] - (lo[a] + h) for a in range(3)] for j in range(3)]
    e = [[V[(j + 1) % 3][a] - V[j][a] for a in range(3)] for j in range(3)]
    for a in range(3):
        if min(u[j][a] for j in range(3)) > h or max(u[j][a] for j in range(3)) < -h:
            return False
    n = [e[0][(a + 1) % 3] * e[1][(a + 2) % 3] - e[0][(a + 2) % 3] * e[1][(a + 1) % 3] for a in range(3)]
    if abs(sum(n[a] * u[0][a] for a in range(3))) > h * sum(abs(x) for x in n):
        return False
    for i in range(3):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            p = [e[i][b] * u[j][c] - e[i][c] * u[j][b] for j in range(3)]
            r = h * (abs(e[i][b]) + abs(e[i][c]))
            if min(p) > r or max(p) < -r:
                return False
    return True


def overlaps_many(V, lo, S, stats=None):
    """V: (n, 3, 3) int64 vertices, lo: (n, 3) int64 box corners, one side S for all.  Returns n bools.  stats (a dict):
    'edge_bits' and 'plane_bits' become the bit lengths of the widest edge-test term and of the widest plane term seen."""
    V, lo = np.asarray(V, dtype=np.int64), np.asarray(lo, dtype=np.int64)
    h = S // 2
    u = V - (lo + h)[:, None, :]
    e = np.roll(V, -1, axis=1) - V
    if V.shape[0] == 0:
        return np.zeros(0, dtype=bool)
    # every int64 term is bounded before it is computed: a product of an edge and a coordinate, twice, and the reach
    e_max, u_max = int(np.abs(e).max()), int(np.abs(u).max())
    edge_term = max(2 * e_max * u_max, 2 * h * e_max)
    assert edge_term < 1 << 62, f"an edge-test term of {edge_term.bit_length()} bits"
    assert 2 * e_max * e_max < 1 << 62  # (the normal's components)
    ok = ~((u.min(axis=1) > h) | (u.max(axis=1) < -h)).any(axis=1)
    for i in range(3):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            p = e[:, i, b, None] * u[:, :, c] - e[:, i, c, None] * u[:, :, b]
            r = h * (np.abs(e[:, i, b]) + np.abs(e[:, i, c]))
            ok &= ~((p.min(axis=1) > r) | (p.max(axis=1) < -r))
    # the plane, for what is left, in Python ints
    k = np.flatnonzero(ok)
    n = [(e[k, 0, (a + 1) % 3] * e[k, 1, (a + 2) % 3] - e[k, 0, (a + 2) % 3] * e[k, 1, (a + 1) % 3]).astype(object) for a in range(3)]
    terms = [n[a] * u[k, 0, a].astype(object) for a in range(3)]
    d = terms[0] + terms[1] + terms[2]
    r = h * (abs(n[0]) + abs(n[1]) + abs(n[2]))
    ok[k[np.array(abs(d) > r, dtype=bool)]] = False
    if stats is not None:
        widest = max([int(abs(x)) for t in terms for x in (t.max(), t.min())] + [int(r.max())]) if len(k) else 0
        stats["edge_bits"] = max(stats.get("edge_bits", 0), edge_term.bit_length())
        stats["plane_bits"] = max(stats.get("plane_bits", 0), (3 * widest).bit_length())  # (three such terms are added)
    return ok


CHILDREN = np.array([[c >> 2 & 1, c >> 1 & 1, c & 1] for c in range(8)], dtype=np.int64)


def voxelize(vq, triangles, depth, colours=None, colour=0xFFFFFF, cap=None, stats=None, levels=None):
    """The contract's list for quantised vertices vq (n, 3) and triangles (t, 3): (xyz (N, 3), colour (N), tri (N)) as
    uint32.  cap: Stopped(level, count) at the first level whose pair count passes it.  levels (a list): gets every level's
    pair count."""
    vq = np.asarray(vq, dtype=np.int64).reshape(-1, 3)
    tris = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    assert 1 <= depth <= 21 and (tris.size == 0 or (tris.min() >= 0 and tris.max() < len(vq)))
    assert vq.size == 0 or (vq.min() >= 0 and vq.max() < 1 << (depth + SUBBITS))
    V = (2 * vq + 1)[tris]  # (t, 3 vertices, 3 axes)
    t = np.arange(len(tris), dtype=np.int64)
    cell = np.zeros((len(tris), 3), dtype=np.int64)
    for level in range(1, depth + 1):
        S = 1 << (depth - level + 7)
        t = np.repeat(t, 8)
        cell = (cell[:, None, :] * 2 + CHILDREN[None, :, :]).reshape(-1, 3)
        keep = overlaps_many(V[t], cell * S, S, stats)
        t, cell = t[keep], cell[keep]
        if levels is not None:
            levels.append(len(t))
        if cap is not None and len(t) > cap:
            return Stopped(level, len(t))
    col = (np.asarray(colours, dtype=np.int64).reshape(-1)[t] if colours is not None else np.full(len(t), colour, dtype=np.int64)) & 0xFFFFFF
    return cell.astype(np.uint32), col.astype(np.uint32), t.astype(np.uint32)


def voxelize_brute(vq, triangles, depth, test=overlaps):
    """every cell of the 2^depth grid against every triangle with `test`: [(tri, x, y, z)] in the contract's order"""
    import build_ref as B
    vq = np.asarray(vq, dtype=np.int64).reshape(-1, 3)
    side, out = 1 << depth, []
    cells = np.array([[x, y, z] for x in range(side) for y in range(side) for z in range(side)], dtype=np.int64)
    cells = cells[np.argsort(B.morton(cells, depth), kind="stable")]
    for k, tri in enumerate(np.asarray(triangles, dtype=np.int64).reshape(-1, 3)):
        V = [[2 * int(q) + 1 for q in vq[v]] for v in tri]
        out += [(k, *c.tolist()) for c in cells if test(V, [int(x) * 128 for x in c], 128)]
    return out
