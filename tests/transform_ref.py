"""Restatements of the affine placement's contract (include/svo_hip.h: svo_nodes_transform) over GPU-layout words,
written independently of each other.

transform()    the rule for one word, applied level by level from the root group: the new words and the tallies
apply_cells()  the per-cell contract on two dense [x, y, z] grids of values: one int64 matrix product and one gather
permutation()  place_ref's (orient, offset) as a matrix and a translation, by the header's formula

A scene word of level l with cell (x, y, z) has zc = 2^(depth - l) cells a side; the source cells its cells can sample lie in
the box qlo..qhi = (mid -+ rad) >> 17 with mid = M (2 cell zc + zc) + 2 t and rad = (zc - 1) sum_j |M[i][j]|.  With e the box's
longest side, s = min(src_depth, ceil(log2 e)) and k = src_depth - s, the word's items are the cells qlo >> s .. qhi >> s of
the source's level-k grid: OUT beyond the cube, else what a walk from the source's root finds on the way to that cell, a leaf
(a constant; carried when it lies above level k) or the interior word of level k.  transform() walks from the root for every
item of every word; it knows no hint.  A source pointer is checked where it is followed: on the way down, for every frontier
word, and as an interior item of a word that is opened or split.
"""
import numpy as np

from build_ref import VOXEL_OFFSET
from combine_ref import CARVE, KEEP, KIDS, MAX_SRC_WORDS, OPS, OVER, PAINT, REPLACE, TALLIES, UNDER, Malformed, Refused, value
from compact_ref import check_length
from place_ref import PERMS

ONE = 1 << 16
MAX_ENTRY, MAX_TRANSLATE = 1 << 20, 1 << 40
OUT, CONST, NODE = range(3)         # an item's kinds
W_OUT, W_LEAF, W_NODE = range(3)    # what a frontier word faces once its items are taken together


def check_params(op, depth, src_depth, matrix, translate):
    if op not in range(6):
        raise ValueError(f"op must be 0..5 (got {op})")
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    if not 1 <= src_depth <= 21:
        raise ValueError(f"src_depth must be 1..21 (got {src_depth})")
    if len(matrix) != 9 or any(abs(int(v)) > MAX_ENTRY for v in matrix):
        raise ValueError(f"a matrix entry must lie in [-2^20, 2^20] (got {tuple(matrix)})")
    if len(translate) != 3 or any(abs(int(v)) > MAX_TRANSLATE for v in translate):
        raise ValueError(f"a translation must lie in [-2^40, 2^40] (got {tuple(translate)})")


def permutation(orient, offset, src_depth):
    """matrix[perm[i]][i] = f_i ? -65536 : 65536, translate[perm[i]] = 65536 (f_i ? S + offset_i : -offset_i)"""
    perm, side = PERMS[orient >> 3], 1 << src_depth
    matrix, translate = [0] * 9, [0] * 3
    for i in range(3):
        flip = (orient >> (2 - i)) & 1
        matrix[3 * perm[i] + i] = -ONE if flip else ONE
        translate[perm[i]] = ONE * (side + offset[i]) if flip else -ONE * offset[i]
    return tuple(matrix), tuple(translate)


def bit_length(v):
    """of non-negative int64 below 2^31, elementwise"""
    out = np.zeros(v.shape, dtype=np.int64)
    for b in range(31):
        out += (v >> b) > 0
    return out


def transform(a_words, n_words, b_words, op, depth, matrix, translate, src_depth=None):
    """-> (the new words, uint32, of the new length; the tallies as a dict, with "levels": per level the frontier's words and
    its splits).  op: a number or a name of OPS.  Raises Refused or Malformed and writes nothing."""
    op = OPS.index(op) if isinstance(op, str) else int(op)
    src_depth = depth if src_depth is None else int(src_depth)
    check_params(op, depth, src_depth, matrix, translate)
    check_length(a_words, n_words)
    src = np.asarray(b_words, dtype=np.uint32).astype(np.int64)
    if src.size < 8 or src.size % 8 or src.size > MAX_SRC_WORDS:
        raise ValueError(f"the source must be a positive multiple of 8 words, at most 2^27 (got {src.size})")
    w = np.asarray(a_words, dtype=np.uint32)[:n_words].astype(np.int64)
    m = np.array([int(v) for v in matrix], dtype=np.int64).reshape(3, 3)
    t2 = 2 * np.array([int(v) for v in translate], dtype=np.int64)
    spread = np.abs(m).sum(axis=1)
    tally = dict.fromkeys(TALLIES, 0)
    tally["levels"] = []
    writes, groups = [], []
    probe_a, probe_b = VOXEL_OFFSET, VOXEL_OFFSET + 1
    out_is_zero = op in (OVER, UNDER, PAINT, CARVE)  # f(a, 0) == a
    one_value = op in (CARVE, KEEP)                  # f asks only whether b is set

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
        zc = 1 << (depth - level)
        c = np.tile(np.arange(8), n_groups)
        rep = np.repeat(np.arange(n_groups), 8)
        addr = g_base[rep] + c
        word = np.where(real[rep], w[np.where(real[rep], addr, 0)], g_virt[rep])
        cell = g_cell[rep] * 2 + KIDS[c]
        n = addr.size

        # the word's box and the level of the source's grid that it faces
        mid = (2 * cell * zc + zc) @ m.T + t2
        rad = (zc - 1) * spread
        qlo, qhi = (mid - rad) >> 17, (mid + rad) >> 17
        e = (qhi - qlo + 1).max(axis=1)
        s_free = bit_length(e - 1)
        big = s_free > src_depth
        s = np.minimum(s_free, src_depth)
        k = src_depth - s
        lo, hi = qlo >> s[:, None], qhi >> s[:, None]

        kind, val = np.zeros((n, 8), dtype=np.int64), np.zeros((n, 8), dtype=np.int64)
        act, inh = np.zeros((n, 8), dtype=bool), np.zeros((n, 8), dtype=bool)
        unaligned = beyond = False  # a pointer followed on the way down
        for j in range(8):
            idx = lo + KIDS[j]
            on = (idx <= hi).all(axis=1) & ~big
            inside = on & (idx >= 0).all(axis=1) & (idx < (1 << k)[:, None]).all(axis=1)
            act[:, j] = on
            # from the root, an interior word pointing at group 0, down to level k or to a leaf
            node = np.zeros(n, dtype=np.int64)        # the word without its counter
            at_level = np.zeros(n, dtype=np.int64)
            going = inside.copy()
            for lvl in range(1, src_depth + 1):
                going &= ((node >> 4) < VOXEL_OFFSET) & (lvl <= k)
                if not going.any():
                    break
                ptr = node[going] >> 4
                unaligned |= bool((ptr % 8 != 0).any())
                beyond |= bool(((ptr % 8 == 0) & (ptr + 8 > src.size)).any())
                sh = (k[going] - lvl)[:, None]
                bits = (idx[going] >> sh) & 1
                good = (ptr % 8 == 0) & (ptr + 8 <= src.size)
                node[going] = np.where(good, src[np.where(good, ptr + (bits[:, 0] << 2 | bits[:, 1] << 1 | bits[:, 2]), 0)] & ~15, node[going])
                at_level[going] = lvl
                going[going] = good
            is_leaf = (node >> 4) >= VOXEL_OFFSET
            kind[:, j] = np.where(inside, np.where(is_leaf, CONST, NODE), OUT)
            val[:, j] = np.where(inside, np.where(is_leaf, (node >> 4) - VOXEL_OFFSET, node >> 4), 0)
            inh[:, j] = inside & is_leaf & (at_level < k)
        # a box larger than the cube: the cell at the origin is the root, and some other cell is OUT
        root_met = big & (qlo < (1 << src_depth)).all(axis=1) & (qhi >= 0).all(axis=1)
        act[big, 0], kind[big, 0], val[big, 0] = root_met[big], NODE, 0
        act[big, 1], kind[big, 1] = True, OUT

        # normalised, then taken together
        nk = np.where((kind == OUT) & out_is_zero, CONST, kind)
        nv = np.where(nk == CONST, np.minimum(val, 1) if one_value else val, 0)
        first = nv[np.arange(n), act.argmax(axis=1)]
        all_out = ((nk == OUT) | ~act).all(axis=1)
        all_const = ((nk == CONST) | ~act).all(axis=1) & ((nv == first[:, None]) | ~act).all(axis=1)
        facing = np.where(all_out, W_OUT, np.where(all_const, W_LEAF, W_NODE))
        b = np.where(all_const, first, 0)

        ptr = word >> 4
        leaf = ptr >= VOXEL_OFFSET
        a = np.where(leaf, ptr - VOXEL_OFFSET, 0)
        v = value(op, a, b)
        over = (facing == W_LEAF) & leaf & (v != a)
        at_zero, at_probe = value(op, 0, b), value(op, probe_a, b)
        identity = (at_zero == 0) & (at_probe == probe_a)
        constant = (at_zero == at_probe) & ~identity
        collapse = (facing == W_LEAF) & ~leaf & constant
        carry = (facing == W_LEAF) & ~leaf & ~constant & ~identity
        stays = (value(op, a, 0) == a) & (value(op, a, probe_b) == a)
        split = (facing == W_NODE) & leaf & ~stays
        opened = carry | ((facing == W_NODE) & ~leaf)
        go = split | opened
        refused = level == depth and go.any()
        if not refused:
            if ((ptr[opened] % 8) != 0).any():
                raise Malformed("tree", f"an interior pointer at level {level} is not a multiple of 8")
            if (ptr[opened] + 8 > n_words).any():
                raise Malformed("tree", f"an interior pointer at level {level} leaves the first n_words = {n_words} words")
            followed = val[go][(kind[go] == NODE) & act[go]]
            unaligned |= bool(((followed % 8) != 0).any())
            beyond |= bool(((followed % 8 == 0) & (followed + 8 > src.size)).any())
        if unaligned:
            raise Malformed("source", f"an interior pointer at level {level} is not a multiple of 8")
        if beyond:
            raise Malformed("source", f"an interior pointer at level {level} leaves the first src_words = {src.size} words")
        if refused:
            i = int(np.flatnonzero(go)[0])
            raise Refused(cell[i], "both" if facing[i] == W_NODE and not leaf[i] else "source" if facing[i] == W_NODE else "scene")
        new_group = n_words + 8 * (len(groups) + np.cumsum(split) - 1)
        out = np.where(split, new_group << 4, np.where(collapse, (VOXEL_OFFSET + at_zero) << 4, (VOXEL_OFFSET + v) << 4))
        wr = split | collapse | over
        writes.append((addr[wr], out[wr]))
        groups += [(int(g), int(x) & ~15) for g, x in zip(new_group[split], word[split])]
        tally["splits"] += int(split.sum())
        tally["collapses"] += int(collapse.sum())
        tally["overwrites"] += int(over.sum())
        tally["opened"] += int(opened.sum())
        tally["carried"] += int((inh | ~act).all(axis=1).sum())
        tally["levels"].append((int(n), int(split.sum())))
        # the next frontier
        g_base = np.where(split, new_group, ptr)[go]
        g_virt = np.where(split, word & ~15, 0)[go]
        g_cell = cell[go]
    result = np.concatenate([w, np.zeros(8 * len(groups), dtype=np.int64)])
    for g, leaf_word in groups:
        result[g:g + 8] = leaf_word
    for addr, x in writes:
        result[addr] = x
    return result.astype(np.uint32), tally


def apply_cells(grid_a, grid_b, op, matrix, translate):
    """grid_a: the scene's (N,)*3 values, indexed [x, y, z]; grid_b: the source's (S,)*3 values.  The per-cell contract's
    result: f(a, b) where the cell's centre maps into the source's cube, b the source's value at the cell it lands in; the
    scene elsewhere."""
    op = OPS.index(op) if isinstance(op, str) else int(op)
    a = np.array(grid_a, dtype=np.uint32)
    grid_b = np.asarray(grid_b, dtype=np.uint32)
    cells = np.stack(np.meshgrid(*(np.arange(n, dtype=np.int64) for n in a.shape), indexing="ij"), -1).reshape(-1, 3)
    p = (2 * cells + 1) @ np.array([int(v) for v in matrix], dtype=np.int64).reshape(3, 3).T + 2 * np.array([int(v) for v in translate], dtype=np.int64)
    q = p >> 17
    hit = ((q >= 0) & (q < np.array(grid_b.shape))).all(axis=1)
    q = q[hit]
    before = a.reshape(-1)[hit]
    b = grid_b[q[:, 0], q[:, 1], q[:, 2]]
    out = a.reshape(-1).copy()
    out[hit] = {OVER: np.where(b != 0, b, before), UNDER: np.where(before != 0, before, b), PAINT: np.where((before != 0) & (b != 0), b, before),
                CARVE: np.where(b != 0, 0, before), KEEP: np.where(b != 0, before, 0), REPLACE: b}[op]
    return out.reshape(a.shape)
