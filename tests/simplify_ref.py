"""Restatements of the simplification's contract (csrc/svo_simplify.hip) over GPU-layout words.

simplify()          from the contract, sequentially: S and U computed recursively, the words rewritten (CUT, then MERGE),
                    then compact_ref.compact(words, n, prune=False) of the rewritten words.
simplify_parallel() the same result the way the kernels reach it: compact_ref.discover(), per level bottom-up the reduce
                    over order / first_child (the mip below cut_level, the uniform field and the children's fates at and
                    above it), then compact_ref.emit() over the candidates, which rewrites on the fly.
merged_cells() /    the per-cell statement on a dense grid: after MERGE every cell samples to what it sampled before; after
cut_cells()         CUT at L every cell samples to S of its level-L cube, or to its old value where the tree ended above L.
mip_pyramid()       S of every cube of every level straight from a dense grid of unit cells, without the tree.

simplify() and simplify_parallel() return (out, perm) with perm[new word] = old word and raise compact_ref.Malformed on a
tree the device refuses.  tally() counts what a scene exercises.
"""
import numpy as np

import compact_ref as K
import sample_ref as S_
from build_ref import VOXEL_OFFSET

NONE = K.KEEP  # no uniform field; as a fate: the group stays
MERGE, CUT = 1, 2


def check_params(merge, cut_level, min_level):
    if not merge and cut_level is None:
        raise ValueError("nothing to simplify: neither merge nor cut_level")
    if cut_level is not None and not 1 <= cut_level <= 31:
        raise ValueError(f"cut_level must be 1..31 (got {cut_level})")
    if not merge and min_level:
        raise ValueError("min_level without merge")


def mip_value(values):
    """S of a group from the S of its eight words"""
    nz = [int(v) for v in values if v]
    if not nz:
        return 0
    return sum(max(1, sum(v >> b & 0xFF for v in nz) // len(nz)) << b for b in (0, 8, 16))


def subtree_mip(w, i):
    """S(W) of the word at index i of the int list w"""
    f = w[i] >> 4
    if f >= VOXEL_OFFSET:
        return f - VOXEL_OFFSET
    return mip_value([subtree_mip(w, f + c) for c in range(8)])


def rewrite(words, n_words, merge=True, cut_level=None, min_level=0):
    """the words after CUT and MERGE, in their old places (what became unreachable keeps what it held or was rewritten
    on the way: it is dropped by the layout), and the tallies"""
    check_params(merge, cut_level, min_level)
    K.compact(words, n_words, False)  # refuses what the device refuses
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)[:n_words]]
    t = {"cut": 0, "merged": 0, "merged_empty": 0, "merged_high": 0, "merged_counters": 0, "cascade": 0, "seven_of_eight": 0,
         "coarsest": 99}

    def cut(g, level):
        for c in range(8):
            f = w[g + c] >> 4
            if f < VOXEL_OFFSET:
                if level == cut_level:
                    w[g + c] = (VOXEL_OFFSET + subtree_mip(w, g + c)) << 4
                    t["cut"] += 1
                else:
                    cut(f, level + 1)

    def uniform(i, level):
        """(U, interior levels merged below and with this word); rewrites bottom-up"""
        f = w[i] >> 4
        if f >= VOXEL_OFFSET:
            return f, 0
        below = [uniform(f + c, level + 1) for c in range(8)]
        us = [u for u, _ in below]
        if level >= min_level and us[0] is not None and all(u == us[0] for u in us):
            t["merged_counters"] += len({w[f + c] & 15 for c in range(8)}) > 1
            w[i] = us[0] << 4
            return us[0], 1 + max(h for _, h in below)
        # what stays: tally the merges right below it
        for c, (u, h) in enumerate(below):
            if h:
                t["merged"] += 1
                t["cascade"] = max(t["cascade"], h)
                t["merged_empty"] += u == VOXEL_OFFSET
                t["merged_high"] += u >= VOXEL_OFFSET + (1 << 24)
                t["coarsest"] = min(t["coarsest"], level + 1)
        leaves = [u for u in us if u is not None]
        if len(leaves) == 7 and len(set(leaves)) == 1:
            t["seven_of_eight"] += 1
        return None, 0

    if cut_level is not None:
        cut(0, 1)
    if merge:
        for c in range(8):
            u, h = uniform(c, 1)
            if h:
                t["merged"] += 1
                t["cascade"] = max(t["cascade"], h)
                t["merged_empty"] += u == VOXEL_OFFSET
                t["merged_high"] += u >= VOXEL_OFFSET + (1 << 24)
                t["coarsest"] = 1
    return np.array(w, dtype=np.uint32), t


def simplify(words, n_words, merge=True, cut_level=None, min_level=0):
    w, _ = rewrite(words, n_words, merge, cut_level, min_level)
    return K.compact(w, n_words, False)


def tally(words, n_words, merge=True, cut_level=None, min_level=0):
    return rewrite(words, n_words, merge, cut_level, min_level)[1]


def simplify_parallel(words, n_words, merge=True, cut_level=None, min_level=0):
    check_params(merge, cut_level, min_level)
    K.check_length(words, n_words)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    order, first_child, level_off = K.discover(w, n_words)
    n_levels, total = len(level_off) - 1, level_off[-1]
    g, interior, child = K.group_words(w, order, first_child)
    # reduce: bottom-up, a launch per level; the words of order[level_off[l], level_off[l + 1]) are of level l + 1
    val = np.zeros(total, dtype=np.int64)
    fate = np.full(total, NONE, dtype=np.int64)
    for l in range(n_levels - 1, -1, -1):
        level, lo, hi = l + 1, level_off[l], level_off[l + 1]
        it, ch, below = interior[lo:hi], child[lo:hi], val[child[lo:hi]]
        if cut_level is not None and level > cut_level:
            s = np.where(it, below, (g[lo:hi] >> 4) - VOXEL_OFFSET)
            nz = s != 0
            n = nz.sum(axis=1)
            mip = np.zeros(hi - lo, dtype=np.int64)
            for b in (0, 8, 16):
                mip |= np.maximum(1, ((s >> b & 0xFF) * nz).sum(axis=1) // np.maximum(n, 1)) << b
            val[lo:hi] = np.where(n > 0, mip, 0)
            continue
        if cut_level is not None and level == cut_level:
            to = VOXEL_OFFSET + below
        elif merge and level >= min_level:
            to = below  # (NONE where the child is not uniform: it stays)
        else:
            to = np.full_like(below, NONE)
        fate[ch[it]] = to[it]
        field = np.where(it, to, g[lo:hi] >> 4)
        same = (field == field[:, :1]).all(axis=1) & (field[:, 0] != NONE)
        val[lo:hi] = np.where(same, field[:, 0], NONE) if merge else NONE
    fate[0] = NONE
    # emit: the groups below cut_level are cut off
    cand = level_off[min(n_levels, cut_level)] if cut_level is not None else total
    return K.emit(w, order, first_child, fate, cand)


def cells(words, n_words, depth):
    """the whole depth grid sampled: (side, side, side) uint32, indexed [x, y, z]"""
    return S_.sample_dense(words, n_words, (0, 0, 0), (1 << depth,) * 3, depth)


def merged_cells(words, n_words, depth):
    """what every cell of the depth grid samples to after MERGE: what it sampled before"""
    return cells(words, n_words, depth)


def cut_cells(words, n_words, depth, cut_level):
    """what every cell of the depth grid samples to after CUT at cut_level: S of its level-cut_level cube where the tree is
    interior there, its old value where the tree ended above"""
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)[:n_words]]
    grid = np.zeros((1 << depth,) * 3, dtype=np.uint32)

    def fill(g, level, x, y, z):
        side = 1 << (depth - level)
        for c in range(8):
            cx, cy, cz = x + side * (c >> 2 & 1), y + side * (c >> 1 & 1), z + side * (c & 1)
            f = w[g + c] >> 4
            if f >= VOXEL_OFFSET:
                grid[cx:cx + side, cy:cy + side, cz:cz + side] = f - VOXEL_OFFSET
            elif level == cut_level:
                grid[cx:cx + side, cy:cy + side, cz:cz + side] = subtree_mip(w, g + c)
            else:
                assert level < depth, "the tree is finer than the grid"
                fill(f, level + 1, cx, cy, cz)

    fill(0, 1, 0, 0, 0)
    return grid


def mip_pyramid(grid):
    """{level: (2^level,) * 3 array of S} of a dense grid of unit cells, [x, y, z], the grid itself at its depth: the mip
    rule applied to 2x2x2 blocks, level by level, without a tree.  Equals S of a tree whose voxels are all unit leaves."""
    g = np.asarray(grid).astype(np.int64)
    depth = g.shape[0].bit_length() - 1
    out = {depth: g}
    for level in range(depth - 1, -1, -1):
        side = 1 << level
        blocks = g.reshape(side, 2, side, 2, side, 2).transpose(0, 2, 4, 1, 3, 5).reshape(side, side, side, 8)
        nz = blocks != 0
        n = nz.sum(axis=-1)
        mip = np.zeros((side,) * 3, dtype=np.int64)
        for b in (0, 8, 16):
            mip |= np.maximum(1, ((blocks >> b & 0xFF) * nz).sum(axis=-1) // np.maximum(n, 1)) << b
        g = np.where(n > 0, mip, 0)
        out[level] = g
    return out
