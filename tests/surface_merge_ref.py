"""Restatements of the merged surface's contract (include/svo_hip.h, csrc/svo_surface_merge.hip), imported
by test_surface_merge_host.py and test_surface_merge_gpu.py only.

quads_to_rects()  the quads of surface_ref.list_surface (QUADS) as the contract's input rectangles.
merge_rects()     the contract in numpy: per phase one lexsort, the follow condition as a diff of neighbours, the runs'
                  extents by reduceat; (rects (n, 6), values (n)) uint32 in the output's order.
greedy_dense()    the same result for a uniform-depth tree, written independently from a dense grid and sharing nothing
                  with merge_rects: exposed faces from shifted copies of the padded grid, then per (face, plane) slice
                  plain loops: runs along u in every row, and runs of equal (u0, w, value) in consecutive rows.
raster()          rectangles painted back into per-face dense masks with a count per cell, so gaps and overlaps show.
followers()       how many pairs of rectangles still satisfy a phase's follow condition, by dictionary lookups.
"""
import numpy as np

FACE, PLANE, U0, V0, W, H = range(6)


def quads_to_rects(quads, depth):
    xyz, value, level, face = (np.asarray(a).astype(np.int64) for a in quads)
    xyz = xyz.reshape(-1, 3)
    rows = np.arange(face.size)
    s = np.int64(1) << (depth - level)
    a = face >> 1
    rects = np.stack([face, xyz[rows, a] + (face & 1) * s, xyz[rows, (a + 1) % 3], xyz[rows, (a + 2) % 3], s, s], axis=1)
    return rects.reshape(-1, 6), value


def phase(rects, values, d, any_value):
    """one phase along d (0: u, 1: v): sorted by (face, plane, position across, extent across, position along), a
    rectangle follows the one before it when the class is the same, it begins where that one ends and the values agree"""
    if not len(rects):
        return rects, values
    pos, ext, across, across_ext = U0 + d, W + d, V0 - d, H - d
    order = np.lexsort((rects[:, pos], rects[:, across_ext], rects[:, across], rects[:, PLANE], rects[:, FACE]))
    r, v = rects[order], values[order]
    cls = r[:, [FACE, PLANE, across, across_ext]]
    follows = (np.diff(cls, axis=0) == 0).all(axis=1) & (r[1:, pos] == r[:-1, pos] + r[:-1, ext])
    if not any_value:
        follows &= np.diff(v) == 0
    head = np.flatnonzero(np.concatenate([[True], ~follows]))
    out = r[head].copy()
    out[:, ext] = np.add.reduceat(r[:, ext], head)
    return out, v[head]


def merge_rects(quads, depth, rounds=1, any_value=False):
    if not 1 <= rounds <= 4:
        raise ValueError(f"rounds outside 1..4 (got {rounds})")
    rects, values = quads_to_rects(quads, depth)
    if any_value:
        values = np.zeros_like(values)
    for _ in range(rounds):
        for d in (0, 1):
            rects, values = phase(rects, values, d, any_value)
    return rects.astype(np.uint32).reshape(-1, 6), values.astype(np.uint32)


def greedy_dense(grid, closed=False):
    """grid[x, y, z]: colours, 0 empty, of side 2^depth.  Returns (rects, values) like merge_rects with rounds = 1."""
    g = np.asarray(grid).astype(np.int64)
    side = g.shape[0]
    solid = np.pad(g != 0, 1, constant_values=bool(closed))
    found = []
    for f in range(6):
        a, up = f >> 1, f & 1
        shifted = np.roll(solid, -1 if up else 1, axis=a)[1:-1, 1:-1, 1:-1]  # the cell behind face f of every cell
        shown = np.where(solid[1:-1, 1:-1, 1:-1] & ~shifted, g, 0)
        slices = np.moveaxis(shown, (a, (a + 1) % 3, (a + 2) % 3), (0, 1, 2))  # [along a, u, v]
        for k in range(side):
            if not slices[k].any():
                continue
            cells = slices[k].tolist()
            open_runs = {}  # (u0, w, value) -> [v0, h] of the run that reached the row before
            for v in range(side + 1):
                row = {}
                u = 0
                while v < side and u < side:
                    value = cells[u][v]
                    if not value:
                        u += 1
                        continue
                    u0 = u
                    while u < side and cells[u][v] == value:
                        u += 1
                    row[(u0, u - u0, value)] = None
                for key in list(open_runs):
                    if key in row:
                        open_runs[key][1] += 1
                    else:
                        v0, h = open_runs.pop(key)
                        found.append((f, k + up, key[0], v0, key[1], h, key[2]))
                for key in row:
                    if key not in open_runs:
                        open_runs[key] = [v, 1]
    found.sort(key=lambda r: (r[FACE], r[PLANE], r[U0], r[W], r[V0]))
    out = np.array(found, dtype=np.int64).reshape(-1, 7)
    return out[:, :6].astype(np.uint32), out[:, 6].astype(np.uint32)


def raster(rects, values, depth):
    """(count, value)[face, plane, u, v]: how many rectangles cover the unit cell (u, v) of plane `plane` of face `face`,
    and the value of the last one that does"""
    side = 1 << depth
    count = np.zeros((6, side + 1, side, side), dtype=np.int32)
    value = np.zeros((6, side + 1, side, side), dtype=np.int64)
    for (f, p, u0, v0, w, h), val in zip(np.asarray(rects).astype(np.int64).tolist(), np.asarray(values).tolist()):
        assert 0 <= f < 6 and 0 <= p <= side and 0 <= u0 and 0 <= v0 and w > 0 and h > 0 and u0 + w <= side and v0 + h <= side
        count[f, p, u0:u0 + w, v0:v0 + h] += 1
        value[f, p, u0:u0 + w, v0:v0 + h] = val
    return count, value


def followers(rects, values, d, any_value=False):
    """the number of rectangles that follow another one in a phase along d"""
    r = np.asarray(rects).astype(np.int64).tolist()
    vals = np.asarray(values).tolist()
    pos, ext, across, across_ext = U0 + d, W + d, V0 - d, H - d
    begins = {(x[FACE], x[PLANE], x[across], x[across_ext], x[pos]): val for x, val in zip(r, vals)}
    n = 0
    for x, val in zip(r, vals):
        after = begins.get((x[FACE], x[PLANE], x[across], x[across_ext], x[pos] + x[ext]))
        n += after is not None and (any_value or after == val)
    return n
