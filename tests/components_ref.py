"""Restatements of the component labelling's contract (include/svo_hip.h, csrc/svo_components.hip) over
GPU-layout words.

labels()        from the contract: the entries of list_ref.list_voxels (flags 0); per entry and face the cell behind the
                face on the entry's own level is looked up by a plain walk from group 0, as surface_ref.covered walks, but
                the walk says WHICH word it stopped on; a voxel word it stops on is an entry, and the two are linked (with
                same_value only when their values are equal).  A plain union-find with the smaller rank as the root gives
                label; the roots numbered in ascending order give ids.  Returns (label, ids, n_components, index), index
                the entries' word indices.  The walks of all entries go level by level in numpy; the rule is per walk.
dense_labels()  independently: the entries expanded into a [x, y, z] grid and labelled by scipy.ndimage.label
                (6-connectivity; per value for same_value).  Returns (component grid, 0 = empty; entry grid, -1 = empty).
same_partition() two labellings of the same items induce the same partition.
drop_floating() drop_floating restated on a grid of values.

labels() raises what list_ref.list_voxels raises.
"""
import numpy as np

import list_ref as L
from build_ref import VOXEL_OFFSET

SAME_VALUE = 1
NO_INDEX = -1


def walk(w, cells, levels):
    """per row the index of the word that the walk from group 0 towards `cell` of the level-`level` grid stops on, or
    NO_INDEX when the word at `level` is still interior (the tree is finer there)"""
    cells, levels = np.asarray(cells, dtype=np.int64).reshape(-1, 3), np.asarray(levels, dtype=np.int64)
    group = np.zeros(levels.size, dtype=np.int64)
    index = np.full(levels.size, NO_INDEX, dtype=np.int64)
    going = np.ones(levels.size, dtype=bool)
    for l in range(1, int(levels.max(initial=0)) + 1):
        rows = np.flatnonzero(going & (levels >= l))
        if not rows.size:
            break
        bit = (cells[rows] >> (levels[rows] - l)[:, None]) & 1
        i = group[rows] + (bit[:, 0] << 2 | bit[:, 1] << 1 | bit[:, 2])
        pointer = w[i] >> 4
        leaf = pointer >= VOXEL_OFFSET
        index[rows[leaf]] = i[leaf]
        going[rows[leaf]] = False
        group[rows[~leaf]] = pointer[~leaf]
    return index


def links(words, n_words, depth, same_value=False):
    """(u, v) entry pairs, every link from the side that finds it; the listing; the entries' word indices"""
    xyz, value, level = L.list_voxels(words, n_words, depth)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    lv = level.astype(np.int64)
    cell = xyz.astype(np.int64) >> (depth - lv)[:, None]
    index = walk(w, cell, lv)
    assert (index >= 0).all() and ((w[index] >> 4) - VOXEL_OFFSET == value).all()  # every entry is found at its own cell
    entry_at = np.full(n_words, -1, dtype=np.int64)
    entry_at[index] = np.arange(value.size)
    us, vs = [], []
    for f in range(6):
        behind = cell.copy()
        behind[:, f >> 1] += 1 if f & 1 else -1
        inside = np.flatnonzero((behind[:, f >> 1] >= 0) & (behind[:, f >> 1] < (1 << lv)))
        stop = walk(w, behind[inside], lv[inside])
        hit = stop >= 0
        hit[hit] = (w[stop[hit]] >> 4) > VOXEL_OFFSET
        u, v = inside[hit], entry_at[stop[hit]]
        assert (v >= 0).all()  # a voxel word a walk stops on is reachable, so it is listed
        if same_value:
            keep = value[u] == value[v]
            u, v = u[keep], v[keep]
        us.append(u)
        vs.append(v)
    return np.concatenate(us), np.concatenate(vs), (xyz, value, level), index.astype(np.uint32)


def labels(words, n_words, depth, same_value=False):
    u, v, (xyz, value, level), index = links(words, n_words, depth, same_value)
    parent = list(range(value.size))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(u.tolist(), v.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.array([find(a) for a in range(value.size)], dtype=np.uint32)
    roots = np.flatnonzero(label == np.arange(value.size))
    number = np.zeros(value.size, dtype=np.uint32)
    number[roots] = np.arange(roots.size)
    return label, number[label], int(roots.size), index


def entry_grid(words, n_words, depth):
    """the [x, y, z] grid of the `depth` grid's cells holding the entry that covers the cell, -1 where none does; the values"""
    xyz, value, level = L.list_voxels(words, n_words, depth)
    side = 1 << depth
    grid = np.full((side,) * 3, -1, dtype=np.int64)
    for e in range(value.size):
        s = 1 << (depth - int(level[e]))
        x, y, z = (int(c) for c in xyz[e])
        grid[x:x + s, y:y + s, z:z + s] = e
    return grid, value.astype(np.int64)


def label_grid(values):
    """scipy's 6-connected labelling of a grid of values' non-zero cells, per value: (labels, 0 = empty; their number)"""
    from scipy import ndimage
    out = np.zeros(values.shape, dtype=np.int64)
    total = 0
    for v in np.unique(values[values != 0]):
        lab, n = ndimage.label(values == v)
        out += np.where(lab > 0, lab + total, 0)
        total += n
    return out, total


def dense_labels(words, n_words, depth, same_value=False):
    entries, value = entry_grid(words, n_words, depth)
    values = np.where(entries >= 0, value[np.maximum(entries, 0)] if value.size else 0, 0)
    if not same_value:
        values = (values != 0).astype(np.int64)
    return label_grid(values)[0], entries


def same_partition(a, b):
    """a[i] == a[j] exactly when b[i] == b[j]"""
    a, b = np.asarray(a).reshape(-1).astype(np.int64), np.asarray(b).reshape(-1).astype(np.int64)
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return a.shape == b.shape and len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def drop_floating(values, anchor=None, same_value=False):
    """a [x, y, z] grid of values without the components that do not meet the box anchor = (lo, hi), hi exclusive (None: the
    floor layer y == 0): (the grid, components, dropped components)"""
    values = np.asarray(values, dtype=np.int64)
    lo, hi = ((0, 0, 0), (values.shape[0], 1, values.shape[2])) if anchor is None else anchor
    lab, n = label_grid(values if same_value else (values != 0).astype(np.int64))
    box = lab[tuple(slice(max(0, a), max(0, b)) for a, b in zip(lo, hi))]
    held = np.zeros(n + 1, dtype=bool)
    held[np.unique(box)] = True
    held[0] = True  # (empty cells stay empty)
    return np.where(held[lab], values, 0), n, int((~held).sum())
