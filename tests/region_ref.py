"""Restatements of the shape edit's contract (include/svo_hip.h: svo_nodes_edit_region) over GPU-layout words.

shapes()       box(...) / ball(...) records as the (n, 8) uint32 array the library takes: kind | mode << 16, colour, a[3], b[3]
classify()     one shape against the cubes of one level: OUT, PART or FULL per cube, in integers
brute_class()  the same answer by enumerating the cell centres of the whole grid (what classify must equal)
edit()         the rule for one word, applied level by level from the root group: the new words and the tallies
apply_cells()  the per-cell contract on a dense [x, y, z] grid of values
table_cases()  the six edits of the depth-7 base that the host and the GPU tests share

The frontier of a level is a list of words in order: the eight children, by child index, of every word of the level above
that was opened or split, those taken in frontier order.  The g-th split of the call gets the group n_words + 8 g.
"""
import numpy as np

from build_ref import EMPTY, VOXEL_OFFSET
from compact_ref import check_length

BOX, BALL = 0, 1
MODE_EMPTY, MODE_VOXELS, MODE_SET = 1, 2, 3
MAX_SHAPES = 1024
OUT, PART, FULL = 0, 1, 2
TALLIES = ("splits", "collapses", "overwrites", "untouched", "opened")


class Refused(Exception):
    """an interior word at `depth` under a shape that does not replace it: the shape's input index and the cell"""

    def __init__(self, shape, cell):
        super().__init__(f"shape {shape} meets an interior node at cell {tuple(cell)}")
        self.shape, self.cell = shape, tuple(cell)


def box(lo, hi, colour, mode=MODE_SET):
    return [BOX | mode << 16, colour & 0xFFFFFF, *lo, *hi]


def ball(centre2, radius2, colour, mode=MODE_SET):
    """centre and radius in HALF cells"""
    return [BALL | mode << 16, colour & 0xFFFFFF, *centre2, radius2, 0, 0]


def shapes(records):
    return np.array(records, dtype=np.int64).reshape(-1, 8).astype(np.uint32)


def check_shapes(sh, depth):
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    sh = np.asarray(sh, dtype=np.uint32).reshape(-1, 8).astype(np.int64)
    if len(sh) > MAX_SHAPES:
        raise ValueError(f"{len(sh)} shapes, more than {MAX_SHAPES}")
    for k, r in enumerate(sh):
        kind, mode = r[0] & 0xFFFF, r[0] >> 16
        if kind not in (BOX, BALL) or not 1 <= mode <= 3:
            raise ValueError(f"shape {k}: kind {kind}, mode {mode}")
        if kind == BOX and not all(r[2 + a] < r[5 + a] <= 1 << depth for a in range(3)):
            raise ValueError(f"shape {k}: the box is empty or leaves the grid")
        if kind == BALL and (max(r[2:5]) > 1 << (depth + 1) or r[5] > 1 << 23):
            raise ValueError(f"shape {k}: the ball's centre or radius is out of range")
    return sh


def classify(rec, q, s):
    """rec: one record (8 ints); q: (N, 3) cells of the level whose cubes are 2^s cells wide.  (N,) of OUT / PART / FULL"""
    rec = [int(v) for v in rec]
    q = np.asarray(q, dtype=np.int64).reshape(-1, 3)
    c0, c1 = q << s, (q + 1) << s
    if rec[0] & 0xFFFF == BOX:
        lo, hi = np.array(rec[2:5]), np.array(rec[5:8])
        full = ((lo <= c0) & (c1 <= hi)).all(axis=1)
        out = ((c1 <= lo) | (c0 >= hi)).any(axis=1)
    else:
        centre, r2 = np.array(rec[2:5]), rec[5] * rec[5]
        a, b = 2 * c0 + 1, 2 * c1 - 1  # the first and the last cell centre per axis, in half cells: odd
        far = np.maximum(np.abs(a - centre), np.abs(b - centre))
        near = np.where(centre < a, a - centre, np.where(centre > b, centre - b, np.where(centre % 2 == 1, 0, 1)))
        full = (far * far).sum(axis=1) <= r2
        out = (near * near).sum(axis=1) > r2
    return np.where(out, OUT, np.where(full, FULL, PART))


def inside(rec, cells):
    """the per-cell test of the contract: (N,) bool for (N, 3) cells of the `depth` grid"""
    rec = [int(v) for v in rec]
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    if rec[0] & 0xFFFF == BOX:
        return ((c >= np.array(rec[2:5])) & (c < np.array(rec[5:8]))).all(axis=1)
    d = 2 * c + 1 - np.array(rec[2:5])
    return (d * d).sum(axis=1) <= rec[5] * rec[5]


def brute_class(rec, depth, level):
    """classify by enumeration: every cell centre of the depth grid is tested, then counted per cube of `level`.  (n, n, n)"""
    side, n, w = 1 << depth, 1 << level, 1 << (depth - level)
    axes = [np.arange(side, dtype=np.int64)] * 3
    cells = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    count = inside(rec, cells).reshape(n, w, n, w, n, w).sum(axis=(1, 3, 5))
    return np.where(count == 0, OUT, np.where(count == w ** 3, FULL, PART))


def _applies(mode, v):
    return np.where(v == 0, mode & 1, mode & 2) != 0


def edit(words, n_words, sh, depth):
    """-> (the new words, uint32, of the new length; the tallies as a dict).  Raises Refused and writes nothing."""
    check_length(words, n_words)
    sh = check_shapes(sh, depth)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    tally = dict.fromkeys(TALLIES, 0)
    writes, groups = [], []  # (addresses, words) per level; the new groups' first words in order
    mode, colour = sh[:, 0] >> 16, sh[:, 1] & 0xFFFFFF
    # the frontier: the word's address, its cell on the level's grid, and the word as it stands (a virtual child's too)
    at = np.arange(8, dtype=np.int64)
    cell = np.stack(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    word = w[:8].copy()
    kids = cell.copy()
    for level in range(1, depth + 1):
        if not len(sh) or not at.size:
            break
        n, s = at.size, depth - level
        cls = np.stack([classify(r, cell, s) for r in sh])  # (shapes, n)
        covering = (cls == FULL) & (mode == MODE_SET)[:, None]
        j = np.where(covering.any(axis=0), len(sh) - 1 - np.argmax(covering[::-1], axis=0), -1)
        later = (cls != OUT) & (np.arange(len(sh))[:, None] > j[None, :])  # the shapes behind j that touch the cube
        touched = (j >= 0) | later.any(axis=0)
        ptr = word >> 4
        leaf = ptr >= VOXEL_OFFSET
        v0 = np.where(leaf, ptr - VOXEL_OFFSET, 0)
        v = np.where(j >= 0, colour[np.maximum(j, 0)], v0)
        split = np.zeros(n, dtype=bool)
        for k in range(len(sh)):
            use = later[k] & leaf & ~split & _applies(mode[k], v)
            full = cls[k] == FULL
            split |= use & ~full & (colour[k] != v)
            v = np.where(use & full, colour[k], v)
        collapse = ~leaf & (j >= 0) & ~later.any(axis=0)
        opened = ~leaf & touched & ~collapse
        if level == depth and opened.any():
            i = int(np.flatnonzero(opened)[0])
            raise Refused(int(np.flatnonzero(later[:, i])[-1]), cell[i])
        assert not (split & (level == depth)).any(), "nothing is PART at the last level"
        over = leaf & ~split & (v != v0)
        new_group = n_words + 8 * (len(groups) + np.cumsum(split) - 1)
        out = np.where(split, new_group << 4, np.where(collapse, (VOXEL_OFFSET + colour[np.maximum(j, 0)]) << 4, (VOXEL_OFFSET + v) << 4))
        wr = split | collapse | over
        writes.append((at[wr], out[wr]))
        groups += [(int(g), int(x) & ~15) for g, x in zip(new_group[split], word[split])]
        tally["splits"] += int(split.sum())
        tally["collapses"] += int(collapse.sum())
        tally["overwrites"] += int(over.sum())
        tally["opened"] += int(opened.sum())
        tally["untouched"] += int(n - wr.sum() - opened.sum())
        # the next frontier
        go = np.flatnonzero(split | opened)
        base = np.where(split, new_group, ptr)[go]
        real = opened[go]
        if ((base[real] % 8 != 0) | (base[real] + 8 > n_words)).any():
            raise ValueError("malformed tree: an interior pointer is unaligned or leaves the words")
        at = (base[:, None] + np.arange(8)[None, :]).reshape(-1)
        cell = (cell[go][:, None, :] * 2 + kids[None, :, :]).reshape(-1, 3)
        word = np.where(real[:, None], w[np.where(real, base, 0)[:, None] + np.arange(8)[None, :]], (word[go] & ~15)[:, None]).reshape(-1)
    result = np.concatenate([w, np.zeros(8 * len(groups), dtype=np.int64)])
    for g, leaf_word in groups:
        result[g:g + 8] = leaf_word
    for a, x in writes:
        result[a] = x
    return result.astype(np.uint32), tally


def apply_cells(grid, depth, sh):
    """grid: (2^depth,)*3 values as svo_nodes_sample gives them, indexed [x, y, z].  The per-cell contract's result."""
    sh = check_shapes(sh, depth)
    side = 1 << depth
    v = np.array(grid, dtype=np.int64).reshape(-1)
    assert v.size == side ** 3
    axes = [np.arange(side, dtype=np.int64)] * 3
    cells = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    for r in sh:
        use = inside(r, cells) & _applies(int(r[0]) >> 16, v)
        v = np.where(use, int(r[1]) & 0xFFFFFF, v)
    return v.reshape(side, side, side).astype(np.uint32)


def table_cases():
    """{name: records} at depth 7, for tests/pass_frame.py's tree7_base: a carved and a filled ball, a painted and a flooded
    box, a stroke of 33 balls (every third a fill, the others carves) under one painting box, and the whole grid"""
    stroke = [ball((40 + 4 * i, 100 + 2 * i, 61 + 3 * i), 17, 0 if i % 3 else 0x00C0FF) for i in range(33)]
    stroke.append(box((30, 40, 20), (100, 90, 80), 0x112233, MODE_VOXELS))
    return {
        "carve ball": [ball((128, 129, 127), 41, 0)],
        "fill ball": [ball((128, 129, 127), 41, 0xABCDEF)],
        "paint box": [box((10, 20, 30), (77, 64, 95), 0x334455, MODE_VOXELS)],
        "flood box": [box((0, 0, 0), (128, 37, 128), 0x2040FF, MODE_EMPTY)],
        "stroke": stroke,
        "whole grid": [box((0, 0, 0), (128, 128, 128), 0x777777)],
    }
