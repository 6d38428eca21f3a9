"""Restatements of the placement's contract (include/svo_hip.h: svo_nodes_place) over GPU-layout words, written
independently of each other.

place()        the rule for one word, applied level by level from the root group: the new words and the tallies
apply_cells()  the per-cell contract on two dense [x, y, z] grids of values: numpy's transpose, flip and slice
orient_grid()  the oriented source as a grid
child_map()    the one permutation of 0..7 that takes an oriented child index to the source's

A scene word of level l has cells of z = 2^(depth - l) and faces the cells of size z of the oriented source that its cube
overlaps: per axis the one with index floor((x z - offset) / z), and the next one when (-offset) mod z != 0.  Such an item is
OUT (outside the source's cube), a constant, a source interior word, or ABOVE k: the cell of size S 2^k at the origin, k >= 1,
whose child 0 is ABOVE k - 1, or with k == 1 the source's root as an interior word pointing at group 0, and whose other seven
are OUT.  A cell above the root holds the source's cube in its corner: a word faces it only when its own cube overlaps the
source's, and is OUT of it otherwise.  A frontier group holds the eight items (jx << 2 | jy << 1 | jz; the unused ones OUT) of its parent's cell; the item
j of child c is the child ((t_x & 1) << 2 | (t_y & 1) << 1 | t_z & 1) of the parent's item (t_x >> 1, t_y >> 1, t_z >> 1), with
t = c + h + j per axis and h = ((-offset) mod 2 z) >= z.
"""
import numpy as np

from build_ref import VOXEL_OFFSET
from combine_ref import CARVE, KEEP, KIDS, MAX_SRC_WORDS, OPS, OVER, PAINT, REPLACE, TALLIES, UNDER, Malformed, Refused, value
from compact_ref import check_length

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
MAX_OFFSET = 1 << 21
OUT, CONST, NODE, ABOVE = range(4)  # an item's kinds
W_OUT, W_LEAF, W_NODE = range(3)    # what a frontier word faces once its items are taken together


def unpack(orient):
    """-> (perm, flips) of orient = 8 p + 4 fx + 2 fy + fz"""
    return PERMS[orient >> 3], ((orient >> 2) & 1, (orient >> 1) & 1, orient & 1)


def child_map(orient):
    """source child index of the oriented child index r: bit of q[perm[i]] = bit of r[i] ^ f_i"""
    perm, flips = unpack(orient)
    out = []
    for r in range(8):
        bits, q = ((r >> 2) & 1, (r >> 1) & 1, r & 1), [0, 0, 0]
        for i in range(3):
            q[perm[i]] = bits[i] ^ flips[i]
        out.append(q[0] << 2 | q[1] << 1 | q[2])
    return np.array(out, dtype=np.int64)


def orient_grid(grid_b, orient):
    """R[r] = grid_b[q] with r[i] = f_i ? S - 1 - q[perm[i]] : q[perm[i]]"""
    perm, flips = unpack(orient)
    return np.flip(np.transpose(np.asarray(grid_b), perm), [i for i in range(3) if flips[i]])


def check_params(op, depth, src_depth, orient, offset):
    if op not in range(6):
        raise ValueError(f"op must be 0..5 (got {op})")
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    if not 1 <= src_depth <= depth:
        raise ValueError(f"src_depth must be 1..depth (got {src_depth})")
    if orient not in range(48):
        raise ValueError(f"orient must be 0..47 (got {orient})")
    if len(offset) != 3 or any(abs(int(v)) > MAX_OFFSET for v in offset):
        raise ValueError(f"offset must lie in [-2^21, 2^21] on every axis (got {tuple(offset)})")


def place(a_words, n_words, b_words, op, depth, offset=(0, 0, 0), orient=0, src_depth=None):
    """-> (the new words, uint32, of the new length; the tallies as a dict, with "levels": per level the frontier's words and
    its splits).  op: a number or a name of OPS.  Raises Refused or Malformed and writes nothing."""
    op = OPS.index(op) if isinstance(op, str) else int(op)
    src_depth = depth if src_depth is None else int(src_depth)
    check_params(op, depth, src_depth, orient, offset)
    check_length(a_words, n_words)
    src = np.asarray(b_words, dtype=np.uint32).astype(np.int64)
    if src.size < 8 or src.size % 8 or src.size > MAX_SRC_WORDS:
        raise ValueError(f"the source must be a positive multiple of 8 words, at most 2^27 (got {src.size})")
    w = np.asarray(a_words, dtype=np.uint32)[:n_words].astype(np.int64)
    minus = -np.array([int(v) for v in offset], dtype=np.int64)
    cmap = child_map(orient)
    tally = dict.fromkeys(TALLIES, 0)
    tally["levels"] = []
    writes, groups = [], []
    probe_a, probe_b = VOXEL_OFFSET, VOXEL_OFFSET + 1
    out_is_zero = op in (OVER, UNDER, PAINT, CARVE)  # f(a, 0) == a
    one_value = op in (CARVE, KEEP)                  # f asks only whether b is set

    # the root group's record: the items of the whole scene cube, z = 2^depth >= S
    z0 = 1 << depth
    first, two0 = minus // z0, (minus % z0 != 0).astype(np.int64)
    i_kind, i_val = np.zeros((1, 8), dtype=np.int64), np.zeros((1, 8), dtype=np.int64)
    for j in range(8):
        if (KIDS[j] <= two0).all() and (first + KIDS[j] == 0).all():
            k = depth - src_depth
            i_kind[0, j], i_val[0, j] = (ABOVE, k) if k else (NODE, 0)
    i_inh = np.zeros((1, 8), dtype=bool)
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
        z = 1 << (depth - level)
        h, two = (minus % (2 * z) >= z).astype(np.int64), (minus % z != 0).astype(np.int64)
        c = np.tile(np.arange(8), n_groups)
        rep = np.repeat(np.arange(n_groups), 8)
        addr = g_base[rep] + c
        word = np.where(real[rep], w[np.where(real[rep], addr, 0)], g_virt[rep])
        cell = g_cell[rep] * 2 + KIDS[c]
        # the word's items, each the child of one of its parent's
        kind, val = np.zeros((addr.size, 8), dtype=np.int64), np.zeros((addr.size, 8), dtype=np.int64)
        inh = np.zeros((addr.size, 8), dtype=bool)
        active = np.array([(KIDS[j] <= two).all() for j in range(8)])
        for j in np.flatnonzero(active):
            t = KIDS[c] + h + KIDS[j]
            slot = (t[:, 0] >> 1) << 2 | (t[:, 1] >> 1) << 1 | t[:, 2] >> 1
            ci = (t[:, 0] & 1) << 2 | (t[:, 1] & 1) << 1 | t[:, 2] & 1
            pk, pv = i_kind[rep, slot], i_val[rep, slot]
            field = src[np.where(pk == NODE, pv + cmap[ci], 0)] >> 4
            is_leaf = field >= VOXEL_OFFSET
            on = (pk == ABOVE) & (ci == 0)
            kind[:, j] = np.select([pk == CONST, pk == NODE, on], [CONST, np.where(is_leaf, CONST, NODE), np.where(pv > 1, ABOVE, NODE)], OUT)
            val[:, j] = np.select([pk == CONST, pk == NODE, on], [pv, np.where(is_leaf, field - VOXEL_OFFSET, field), np.where(pv > 1, pv - 1, 0)], 0)
            inh[:, j] = pk == CONST
        # a cell above the root holds the source's cube in its corner and nothing else: a word beside the cube is OUT of it
        beside = ((cell * z + minus) >= (1 << src_depth)).any(axis=1)
        kind[(kind == ABOVE) & beside[:, None]] = OUT
        val[kind == OUT] = 0
        # normalised, then taken together
        nk = np.where((kind == OUT) & out_is_zero, CONST, kind)
        nv = np.where(nk == CONST, np.minimum(val, 1) if one_value else val, 0)
        all_out = (nk[:, active] == OUT).all(axis=1)
        all_const = (nk[:, active] == CONST).all(axis=1) & (nv[:, active] == nv[:, :1]).all(axis=1)
        facing = np.where(all_out, W_OUT, np.where(all_const, W_LEAF, W_NODE))
        b = np.where(all_const, nv[:, 0], 0)

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
        if level == depth and go.any():
            i = int(np.flatnonzero(go)[0])
            raise Refused(cell[i], "both" if facing[i] == W_NODE and not leaf[i] else "source" if facing[i] == W_NODE else "scene")
        if ((ptr[opened] % 8) != 0).any():
            raise Malformed("tree", f"an interior pointer at level {level} is not a multiple of 8")
        if (ptr[opened] + 8 > n_words).any():
            raise Malformed("tree", f"an interior pointer at level {level} leaves the first n_words = {n_words} words")
        followed = val[go][kind[go] == NODE]
        if ((followed % 8) != 0).any():
            raise Malformed("source", f"an interior pointer at level {level} is not a multiple of 8")
        if (followed + 8 > src.size).any():
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
        tally["carried"] += int(inh[:, active].all(axis=1).sum())
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


def apply_cells(grid_a, grid_b, op, offset=(0, 0, 0), orient=0):
    """grid_a: the scene's (N,)*3 values, indexed [x, y, z]; grid_b: the source's (S,)*3 values.  The per-cell contract's
    result: f(a, b) where the oriented source, moved by `offset`, lies over the scene, the scene elsewhere."""
    op = OPS.index(op) if isinstance(op, str) else int(op)
    out = np.array(grid_a, dtype=np.uint32)
    turned = orient_grid(np.asarray(grid_b, dtype=np.uint32), orient)
    lo = [max(0, int(o)) for o in offset]
    hi = [min(n, int(o) + s) for n, o, s in zip(out.shape, offset, turned.shape)]
    if any(h <= l for l, h in zip(lo, hi)):
        return out
    box = tuple(slice(l, h) for l, h in zip(lo, hi))
    a = out[box]
    b = turned[tuple(slice(l - int(o), h - int(o)) for l, h, o in zip(lo, hi, offset))]
    out[box] = {OVER: np.where(b != 0, b, a), UNDER: np.where(a != 0, a, b), PAINT: np.where((a != 0) & (b != 0), b, a),
                CARVE: np.where(b != 0, 0, a), KEEP: np.where(b != 0, a, 0), REPLACE: b}[op]
    return out
