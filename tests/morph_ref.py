"""Restatements of the morphology step's contract (include/svo_hip.h: svo_nodes_morph) over GPU-layout words,
written independently of each other and sharing no table with the kernel.

cells()    the per-cell contract on a dense [x, y, z] grid of values, by shifted copies of the padded grid
morph()    the rule for one word, applied level by level from the root group: the new words and the tallies
steps()    what Render.morph_nodes composes: grow, shrink, close and open of so many steps, on a grid

A frontier word of level l comes with 27 items, the cells q + e of its own level for e in {-1,0,1}^3, as they were before the
call: OUT (outside the grid), a constant (a leaf's value, also one carried down from a coarser leaf) or an interior word.  A
frontier group holds the items of its parent's cell at 9 (ex + 1) + 3 (ey + 1) + ez + 1; item d of child c is, per axis with t = c
+ d, the child t & 1 of the parent's item floor(t / 2).  Only the items of conn's offsets and the cell itself are derived.
"""
import numpy as np

from build_ref import VOXEL_OFFSET
from combine_ref import KIDS, Malformed
from compact_ref import check_length

OPS = ("grow", "shrink")
GROW, SHRINK = range(2)
TALLIES = ("splits", "overwrites", "opened", "refusals")
OUT, CONST, NODE = range(3)  # an item's kinds
# the 26 offsets in priority order: ascending (|d|_1, dx, dy, dz), faces before edges before corners
OFFSETS = sorted(((dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)),
                 key=lambda d: (sum(abs(v) for v in d), d))
REACH = {6: 1, 18: 2, 26: 3}


def offsets(conn):
    return [d for d in OFFSETS if sum(abs(v) for v in d) <= REACH[conn]]


class Refused(Exception):
    """the tree is finer than `depth`: the first refused word of the last level's frontier, and how many there are"""

    def __init__(self, cell, count):
        super().__init__(f"cell {tuple(cell)}: finer than depth")
        self.cell, self.count = tuple(int(v) for v in cell), int(count)


def check_params(op, conn, depth, colour, flags=0):
    if op not in (GROW, SHRINK):
        raise ValueError(f"op must be 0 or 1 (got {op})")
    if conn not in REACH:
        raise ValueError(f"conn must be 6, 18 or 26 (got {conn})")
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    if flags & ~1:
        raise ValueError(f"unknown flag bits (got {flags})")
    if op == SHRINK and colour:
        raise ValueError("a shrink makes no cells: colour must be 0")


def neighbour(grid, d, outside):
    """N[c] = grid[c + d], `outside` where c + d leaves the grid"""
    n = grid.shape
    padded = np.pad(grid, 1, constant_values=outside)
    return padded[1 + d[0]:1 + d[0] + n[0], 1 + d[1]:1 + d[1] + n[1], 1 + d[2]:1 + d[2] + n[2]]


def cells(grid, op, conn, colour=0, open_boundary=False):
    """grid: the (N,)*3 values as svo_nodes_sample gives them, indexed [x, y, z].  The per-cell contract's result."""
    op = OPS.index(op) if isinstance(op, str) else int(op)
    grid = np.asarray(grid, dtype=np.uint32)
    if op == GROW:
        found = np.zeros_like(grid)
        for d in reversed(offsets(conn)):  # the first by priority is applied last, so it wins
            b = neighbour(grid, d, 0)
            found = np.where(b != 0, b, found)
        return np.where(grid != 0, grid, np.where((found != 0) & (colour != 0), np.uint32(colour), found)).astype(np.uint32)
    exposed = np.zeros(grid.shape, dtype=bool)
    for d in offsets(conn):
        exposed |= neighbour(grid, d, 0 if open_boundary else 1) == 0
    return np.where(exposed, 0, grid).astype(np.uint32)


def steps(grid, op, n=1, conn=26, colour=0, open_boundary=False):
    """Render.morph_nodes on a grid: "grow", "shrink", "close" (n grows, then n shrinks) or "open" (the reverse)"""
    for step in {"grow": (GROW,), "shrink": (SHRINK,), "close": (GROW, SHRINK), "open": (SHRINK, GROW)}[op]:
        for _ in range(n):
            grid = cells(grid, step, conn, colour if step == GROW else 0, open_boundary)
    return grid


def slot_of(e):
    return 9 * (e[..., 0] + 1) + 3 * (e[..., 1] + 1) + e[..., 2] + 1


def morph(words, n_words, op, conn, depth, colour=0, open_boundary=False):
    """-> (the new words, uint32, of the new length; the tallies as a dict, with "levels": per level the frontier's words and
    its splits).  op: a number or a name of OPS.  Raises Refused or Malformed and writes nothing."""
    op = OPS.index(op) if isinstance(op, str) else int(op)
    check_params(op, conn, depth, colour)
    check_length(words, n_words)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    grow = op == GROW
    counting = np.array(offsets(conn), dtype=np.int64)          # in priority order
    derived = np.concatenate([np.zeros((1, 3), dtype=np.int64), counting])  # ... and the cell itself
    cols = slot_of(counting)
    tally = dict.fromkeys(TALLIES, 0)
    tally["levels"] = []
    writes, groups = [], []

    # the root group's record: the whole grid as an interior word pointing at group 0, OUT around it
    i_kind, i_val = np.full((1, 27), OUT, dtype=np.int64), np.zeros((1, 27), dtype=np.int64)
    i_kind[0, 13] = NODE
    g_base, g_virt, g_cell = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros((1, 3), dtype=np.int64)
    seen = set()
    for level in range(1, depth + 1):
        n_groups = g_base.size
        if not n_groups:
            break
        real = g_virt == 0
        for g in g_base[real].tolist():
            if g in seen:
                raise Malformed("tree", "a group is reached twice")
            seen.add(g)
        c = np.tile(np.arange(8), n_groups)
        rep = np.repeat(np.arange(n_groups), 8)
        addr = g_base[rep] + c
        word = np.where(real[rep], w[np.where(real[rep], addr, 0)], g_virt[rep])
        cell = g_cell[rep] * 2 + KIDS[c]
        # the word's items, each the child of one of its parent's
        kind, val = np.full((addr.size, 27), OUT, dtype=np.int64), np.zeros((addr.size, 27), dtype=np.int64)
        for e in derived:
            t = KIDS[c] + e
            pk, pv = i_kind[rep, slot_of(t >> 1)], i_val[rep, slot_of(t >> 1)]
            ci = (t[:, 0] & 1) << 2 | (t[:, 1] & 1) << 1 | t[:, 2] & 1
            field = w[np.where(pk == NODE, pv + ci, 0)] >> 4
            is_leaf = field >= VOXEL_OFFSET
            j = int(slot_of(e))
            kind[:, j] = np.select([pk == CONST, pk == NODE], [CONST, np.where(is_leaf, CONST, NODE)], OUT)
            val[:, j] = np.select([pk == CONST, pk == NODE], [pv, np.where(is_leaf, field - VOXEL_OFFSET, field)], 0)
        assert (kind[:, 13] != OUT).all() and (np.where(kind[:, 13] == NODE, val[:, 13], val[:, 13] + VOXEL_OFFSET) == word >> 4).all()
        # normalised: OUT is a constant, 0 for a grow and under an open boundary, set otherwise
        nk = np.where(kind == OUT, CONST, kind)[:, cols]
        nv = np.where(kind == OUT, 0 if grow or open_boundary else 1, val)[:, cols]
        quiet = (nk == CONST) & ((nv == 0) if grow else (nv != 0))
        loud = ~quiet

        ptr = word >> 4
        leaf = ptr >= VOXEL_OFFSET
        a = np.where(leaf, ptr - VOXEL_OFFSET, 0)
        can_change = leaf & ((a == 0) if grow else (a != 0))
        touched = can_change & loud.any(axis=1)
        opened = ~leaf
        split = touched & (level < depth)
        over = touched & (level == depth)
        refused = (over & (loud & (nk == NODE)).any(axis=1)) | (opened & (level == depth))
        if refused.any():
            raise Refused(cell[int(np.flatnonzero(refused)[0])], refused.sum())
        go = split | opened
        followed = val[go][kind[go] == NODE]
        if ((followed % 8) != 0).any():
            raise Malformed("tree", f"an interior pointer at level {level} is not a multiple of 8")
        if (followed + 8 > n_words).any():
            raise Malformed("tree", f"an interior pointer at level {level} leaves the first n_words = {n_words} words")
        # the first value set, in priority order (a grow's loud items are exactly the constants that are set)
        set_ = (nk == CONST) & (nv != 0)
        first = nv[np.arange(addr.size), np.argmax(set_, axis=1)] * set_.any(axis=1)
        v = np.where(first != 0, colour if colour else first, 0) if grow else np.zeros_like(first)
        new_group = n_words + 8 * (len(groups) + np.cumsum(split) - 1)
        out = np.where(split, new_group << 4, (VOXEL_OFFSET + v) << 4)
        wr = split | over
        writes.append((addr[wr], out[wr]))
        groups += [(int(g), int(x) & ~15) for g, x in zip(new_group[split], word[split])]
        tally["splits"] += int(split.sum())
        tally["overwrites"] += int(over.sum())
        tally["opened"] += int(opened.sum())
        tally["levels"].append((int(addr.size), int(split.sum())))
        # the next frontier
        g_base = np.where(split, new_group, ptr)[go]
        g_virt = np.where(split, word & ~15, 0)[go]
        g_cell = cell[go]
        i_kind, i_val = kind[go], val[go]
    result = np.concatenate([w, np.zeros(8 * len(groups), dtype=np.int64)])
    for g, leaf_word in groups:
        result[g:g + 8] = leaf_word
    for addr, x in writes:
        result[addr] = x
    return result.astype(np.uint32), tally
