"""Restatements of the combine's contract (include/svo_hip.h: svo_nodes_combine) over GPU-layout words, written
independently of each other.

combine()      the rule for one word, applied level by level from the root group: the new words and the tallies
apply_cells()  the per-cell contract on two dense [x, y, z] grids of values, with nothing but np.where
ball_source()  the depth-7 source that the host and the GPU tests share: a two-coloured solid ball, merged

A frontier group pairs eight scene words (in the buffer, or the virtual children of a split: one leaf word) with what the
source has for their cubes: the eight words of a source group, a constant carried down from a source leaf, or the path
above the placement, where one child leads on towards `at` and the other seven lie outside the source.  The frontier of a
level is the children, by child index, of every word of the level above that was opened or split, those taken in frontier
order.  The g-th split of the call gets the group n_words + 8 g.
"""
import numpy as np

from build_ref import VOXEL_OFFSET
from compact_ref import check_length

OPS = ("over", "under", "paint", "carve", "keep", "replace")
OVER, UNDER, PAINT, CARVE, KEEP, REPLACE = range(6)
MAX_SRC_WORDS = 1 << 27
TALLIES = ("splits", "collapses", "overwrites", "opened", "carried")
CONST, GROUP, PATH = 0, 1, 2  # what a frontier group has on the source's side
OUT, LEAF, NODE = 0, 1, 2     # ... and a frontier word
KIDS = np.stack(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)  # child c: x << 2 | y << 1 | z


class Refused(Exception):
    """a word that the op has to open or split at level `depth`: the cell, and which tree goes on below it"""

    def __init__(self, cell, finer):
        super().__init__(f"cell {tuple(cell)}: finer there than the combine ({finer})")
        self.cell, self.finer = tuple(int(v) for v in cell), finer


class Malformed(ValueError):
    """a pointer that the call follows is unaligned or leaves its tree's words, or a scene group is reached twice"""

    def __init__(self, which, why):
        super().__init__(f"malformed {which}: {why}")
        self.which = which


def value(op, a, b):
    """f(a, b) of the contract, elementwise on int64 arrays"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    if op == OVER:
        return a * (b == 0) + b
    if op == UNDER:
        return a + b * (a == 0)
    if op == PAINT:
        both = (a != 0) & (b != 0)
        return a * ~both + b * both
    if op == CARVE:
        return a * (b == 0)
    if op == KEEP:
        return a * (b != 0)
    return b + 0 * a


def check_params(op, depth, at_level, at):
    if op not in range(6):
        raise ValueError(f"op must be 0..5 (got {op})")
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    if not 0 <= at_level < depth:
        raise ValueError(f"at_level must be 0..depth-1 (got {at_level})")
    if len(at) != 3 or any(not 0 <= int(v) < 1 << at_level for v in at):
        raise ValueError(f"at must lie in [0, 2^at_level) on every axis (got {tuple(at)})")


def combine(a_words, n_words, b_words, op, depth, at_level=0, at=(0, 0, 0)):
    """-> (the new words, uint32, of the new length; the tallies as a dict, with "levels": per level the frontier's words and
    its splits).  op: a number or a name of OPS.  Raises Refused or Malformed and writes nothing."""
    op = OPS.index(op) if isinstance(op, str) else int(op)
    check_params(op, depth, at_level, at)
    check_length(a_words, n_words)
    src = np.asarray(b_words, dtype=np.uint32).astype(np.int64)
    if src.size < 8 or src.size % 8 or src.size > MAX_SRC_WORDS:
        raise ValueError(f"the source must be a positive multiple of 8 words, at most 2^27 (got {src.size})")
    w = np.asarray(a_words, dtype=np.uint32)[:n_words].astype(np.int64)
    at = np.array([int(v) for v in at], dtype=np.int64)
    tally = dict.fromkeys(TALLIES, 0)
    tally["levels"] = []
    writes, groups = [], []  # (addresses, words) per level; (first word, leaf word) of the new groups in order
    # whether f(., b) is the identity or a constant, and whether f(a, .) is a, asked of f itself with values no tree holds
    probe_a, probe_b = VOXEL_OFFSET, VOXEL_OFFSET + 1

    # the frontier's groups: the scene's first word and virtual leaf word (0: a real group), the source's side, the parent's cell
    g_base, g_virt = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    g_kind, g_val = np.array([PATH if at_level else GROUP]), np.zeros(1, dtype=np.int64)
    g_cell = np.zeros((1, 3), dtype=np.int64)
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
        # the source's side of every word
        kind, b, nxt_kind, nxt_val = (np.zeros(addr.size, dtype=np.int64) for _ in range(4))
        is_path, is_const, is_group = (g_kind[rep] == k for k in (PATH, CONST, GROUP))
        if is_path.any():
            up = at_level - level
            live = ((at[0] >> up) & 1) << 2 | ((at[1] >> up) & 1) << 1 | ((at[2] >> up) & 1)
            kind[is_path] = np.where(c[is_path] == live, NODE, OUT)
            nxt_kind[is_path] = PATH if up else GROUP  # (at at_level: the source's root group, 0)
        kind[is_const], b[is_const] = LEAF, g_val[rep][is_const]
        field = src[np.where(is_group, g_val[rep] + c, 0)] >> 4
        src_leaf = is_group & (field >= VOXEL_OFFSET)
        kind[src_leaf], b[src_leaf] = LEAF, (field - VOXEL_OFFSET)[src_leaf]
        src_node = is_group & ~src_leaf
        kind[src_node], nxt_kind[src_node], nxt_val[src_node] = NODE, GROUP, field[src_node]

        ptr = word >> 4
        leaf = ptr >= VOXEL_OFFSET
        a = np.where(leaf, ptr - VOXEL_OFFSET, 0)
        v = value(op, a, b)
        over = (kind == LEAF) & leaf & (v != a)
        at_zero, at_probe = value(op, 0, b), value(op, probe_a, b)
        identity = (at_zero == 0) & (at_probe == probe_a)
        constant = (at_zero == at_probe) & ~identity
        collapse = (kind == LEAF) & ~leaf & constant
        carry = (kind == LEAF) & ~leaf & ~constant & ~identity
        stays = (value(op, a, 0) == a) & (value(op, a, probe_b) == a)
        split = (kind == NODE) & leaf & ~stays
        opened = carry | ((kind == NODE) & ~leaf)
        go = split | opened
        if level == depth and go.any():
            i = int(np.flatnonzero(go)[0])
            raise Refused(cell[i], "both" if kind[i] == NODE and not leaf[i] else "source" if kind[i] == NODE else "scene")
        if ((ptr[opened] % 8) != 0).any():
            raise Malformed("tree", f"an interior pointer at level {level} is not a multiple of 8")
        if (ptr[opened] + 8 > n_words).any():
            raise Malformed("tree", f"an interior pointer at level {level} leaves the first n_words = {n_words} words")
        follow = go & (kind == NODE) & (nxt_kind == GROUP)
        if ((nxt_val[follow] % 8) != 0).any():
            raise Malformed("source", f"an interior pointer at level {level} is not a multiple of 8")
        if (nxt_val[follow] + 8 > src.size).any():
            raise Malformed("source", f"an interior pointer at level {level} leaves the first src_words = {src.size} words")
        new_group = n_words + 8 * (len(groups) + np.cumsum(split) - 1)
        out = np.where(split, new_group << 4, np.where(collapse, (VOXEL_OFFSET + at_zero) << 4, (VOXEL_OFFSET + v) << 4))
        wr = split | collapse | over
        writes.append((addr[wr], out[wr]))
        groups += [(int(g), int(x) & ~15) for g, x in zip(new_group[split], word[split])]
        tally["splits"] += int(split.sum())
        tally["collapses"] += int(collapse.sum())
        tally["overwrites"] += int(over.sum())
        tally["opened"] += int(opened.sum())
        tally["carried"] += int(is_const.sum())
        tally["levels"].append((int(addr.size), int(split.sum())))
        # the next frontier
        g_base = np.where(split, new_group, ptr)[go]
        g_virt = np.where(split, word & ~15, 0)[go]
        g_kind = np.where(kind == LEAF, CONST, nxt_kind)[go]
        g_val = np.where(kind == LEAF, b, nxt_val)[go]
        g_cell = cell[go]
    result = np.concatenate([w, np.zeros(8 * len(groups), dtype=np.int64)])
    for g, leaf_word in groups:
        result[g:g + 8] = leaf_word
    for addr, x in writes:
        result[addr] = x
    return result.astype(np.uint32), tally


def apply_cells(grid_a, grid_b, op, at, s):
    """grid_a: the scene's (2^depth,)*3 values as svo_nodes_sample gives them, indexed [x, y, z]; grid_b: the source's
    (2^s,)*3 values; the source's cube starts at the cell at << s.  The per-cell contract's result."""
    op = OPS.index(op) if isinstance(op, str) else int(op)
    out = np.array(grid_a, dtype=np.uint32)
    b = np.asarray(grid_b, dtype=np.uint32)
    side = 1 << s
    assert b.shape == (side,) * 3
    x, y, z = (int(v) << s for v in at)
    a = out[x:x + side, y:y + side, z:z + side]
    assert a.shape == b.shape
    if op == OVER:
        f = np.where(b != 0, b, a)
    elif op == UNDER:
        f = np.where(a != 0, a, b)
    elif op == PAINT:
        f = np.where(a != 0, np.where(b != 0, b, a), a)
    elif op == CARVE:
        f = np.where(b != 0, 0, a)
    elif op == KEEP:
        f = np.where(b != 0, a, 0)
    elif op == REPLACE:
        f = np.where(True, b, a)
    else:
        raise ValueError(f"op must be 0..5 (got {op})")
    out[x:x + side, y:y + side, z:z + side] = f
    return out


def ball_cells(depth, centre2, radius2):
    """the cells of the `depth` grid whose centres lie within radius2 half cells of centre2 (half cells): (N, 3)"""
    side = np.arange(1 << depth, dtype=np.int64)
    q = np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3)
    d = 2 * q + 1 - np.array(centre2, dtype=np.int64)
    return q[(d * d).sum(axis=1) <= radius2 * radius2]


def ball_source():
    """a solid ball of radius 50 cells around the middle of the depth-7 grid, one colour below x = 64 and another from there on,
    built and merged: a source with coarse leaves of both colours and of empty space"""
    import build_ref as B
    import simplify_ref as M
    cells = ball_cells(7, (128, 128, 128), 100)
    built = B.build(cells, 7, np.where(cells[:, 0] < 64, 0x40C0FF, 0xFF8020))
    return M.simplify(built, built.size)[0]
