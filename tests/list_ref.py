"""Restatements of the voxel listing's contract (csrc/svo_list.hip) over GPU-layout words.

list_voxels()   from the contract, sequentially: a depth-first walk from group 0 by child index; every voxel word
                (word >> 4 > VOXEL_OFFSET, counter ignored) is an entry (minimum corner on the `depth` grid, value, level);
                with `expand` a voxel above `depth` becomes its cells of the `depth` grid in Morton order.
list_parallel() the same result the way the kernels reach it: compact_ref.discover() (frontier per level, order,
                first_child, the reached-twice test), entry and record counts bottom-up per level, starts and Morton
                prefixes top-down per level, the emit, and for the expansion the search of the record that covers an entry.

Both return (xyz (N, 3) uint32, value (N) uint32, level (N) uint32) and raise compact_ref.Malformed on a tree the device
refuses as malformed, TooDeep when a voxel or an interior word lies deeper than `depth`, TooMany for 2^31 entries or more;
of several causes the first in that order.
"""
import numpy as np

from build_ref import VOXEL_OFFSET
from compact_ref import MAX_LEVELS, Malformed, check_length, discover, exclusive_scan, group_words

MAX_ENTRIES = 1 << 31


class TooDeep(ValueError):
    def __init__(self, level, depth):
        super().__init__(f"the tree holds a voxel or an interior word at level {level}, deeper than depth = {depth}")
        self.level = level


class TooMany(OverflowError):
    def __init__(self, count):
        super().__init__(f"the list has {count} entries, 2^31 or more")
        self.count = count


def demorton(keys, depth):
    """(N, 3) uint32 cells of Morton keys (build_ref.morton's convention)"""
    k = np.asarray(keys, dtype=np.uint64).reshape(-1)
    out = np.zeros((k.size, 3), dtype=np.uint64)
    for b in range(depth):
        for axis, pos in ((0, 2), (1, 1), (2, 0)):
            out[:, axis] |= ((k >> np.uint64(3 * b + pos)) & np.uint64(1)) << np.uint64(b)
    return out.astype(np.uint32)


def finish(cells, levels, values, depth, expand):
    """entries (cell key on its level's grid, level, value), in order -> the three arrays; cells as python ints"""
    count = sum(8 ** (depth - l) for l in levels) if expand else len(levels)
    if count >= MAX_ENTRIES:
        raise TooMany(count)
    cell, level = np.array(cells, dtype=np.uint64), np.array(levels, dtype=np.int64)
    size = np.where(level < depth, 8 ** (depth - np.minimum(level, depth)), 1) if expand else np.ones(level.size, dtype=np.int64)
    start = exclusive_scan(size)
    xyz = np.zeros((count, 3), dtype=np.uint32)
    val, lev = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    for l in np.unique(level[size == 1]):  # the entries that stay one entry, level by level
        pick = (level == l) & (size == 1)
        xyz[start[pick]] = demorton(cell[pick], l) << np.uint32(depth - l)
        val[start[pick]], lev[start[pick]] = np.array(values, dtype=np.uint32)[pick], l
    for i in np.flatnonzero(size > 1):  # the voxels above `depth`, one by one
        at, m = start[i], size[i]
        xyz[at:at + m] = demorton((cells[i] << 3 * (depth - levels[i])) + np.arange(m, dtype=np.uint64), depth)
        val[at:at + m], lev[at:at + m] = values[i], depth
    return xyz, val, lev


def list_voxels(words, n_words, depth, expand=False):
    check_length(words, n_words)
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)[:n_words]]
    cells, levels, values = [], [], []
    seen, deepest = set(), 0  # (deepest: of the voxel and interior words)
    stack = [("group", 0, 1, 0)]  # (kind, group or cell key, level, Morton prefix or value), the next in child order on top
    while stack:
        kind, g, level, prefix = stack.pop()
        if kind == "voxel":
            cells.append(g)
            levels.append(level)
            values.append(prefix)
            continue
        if level > MAX_LEVELS:
            raise Malformed(f"deeper than {MAX_LEVELS} levels")
        if g in seen:
            raise Malformed("a group is reached twice")
        seen.add(g)
        below = []
        for c in range(8):
            pointer = w[g + c] >> 4
            if pointer == VOXEL_OFFSET:
                continue
            deepest = max(deepest, level)
            if pointer < VOXEL_OFFSET:
                if pointer % 8:
                    raise Malformed("a pointer is not a multiple of 8")
                if pointer + 8 > n_words:
                    raise Malformed("a pointer leaves the words")
                below.append(("group", pointer, level + 1, prefix << 3 | c))
            else:
                below.append(("voxel", prefix << 3 | c, level, pointer - VOXEL_OFFSET))
        stack.extend(reversed(below))
    if deepest > depth:
        raise TooDeep(deepest, depth)
    return finish(cells, levels, values, depth, expand)


def list_parallel(words, n_words, depth, expand=False):
    check_length(words, n_words)
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)

    # discover and check; a group reached twice is refused here, ahead of the counts, which refuse nothing themselves
    order, first_child, level_off = discover(w, n_words)
    total, n_levels = order.size, len(level_off) - 1
    g, interior, child = group_words(w, order, first_child)
    pointer = g >> 4
    voxel = pointer > VOXEL_OFFSET
    leaf = lambda l: 8 ** (depth - l) if expand else 1  # noqa: E731
    coarse = lambda l: 1 if expand and l < depth else 0  # noqa: E731

    # count: bottom-up, a launch per level; python ints, as the device counts in 64 bits
    cnt, rcnt = np.zeros(total, dtype=object), np.zeros(total, dtype=np.int64)
    deep = 0
    for l in range(n_levels, 0, -1):
        lo, hi = level_off[l - 1], level_off[l]
        if l > depth:
            if (pointer[lo:hi] != VOXEL_OFFSET).any():
                deep = max(deep, l)
            continue
        cnt[lo:hi] = np.where(interior[lo:hi], cnt[child[lo:hi]], np.where(voxel[lo:hi], leaf(l), 0).astype(object)).sum(axis=1)
        rcnt[lo:hi] = np.where(interior[lo:hi], rcnt[child[lo:hi]], np.where(voxel[lo:hi], coarse(l), 0)).sum(axis=1)
    if deep:
        raise TooDeep(deep, depth)
    count, n_rec = int(cnt[0]), int(rcnt[0])
    if count >= MAX_ENTRIES:
        raise TooMany(count)

    # offsets: top-down, a launch per level
    cnt = cnt.astype(np.int64)
    listed = min(n_levels, depth)
    start, rstart, key = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.int64), np.ones(total, dtype=np.uint64)
    share = np.zeros((total, 8), dtype=np.int64)
    rshare = np.zeros((total, 8), dtype=np.int64)
    level_of = np.zeros(total, dtype=np.int64)
    for l in range(1, listed + 1):
        lo, hi = level_off[l - 1], level_off[l]
        level_of[lo:hi] = l
        share[lo:hi] = np.where(interior[lo:hi], cnt[child[lo:hi]], np.where(voxel[lo:hi], leaf(l), 0))
        rshare[lo:hi] = np.where(interior[lo:hi], rcnt[child[lo:hi]], np.where(voxel[lo:hi], coarse(l), 0))
    at = np.cumsum(share, axis=1) - share  # exclusive prefix over the 8 lanes
    rat = np.cumsum(rshare, axis=1) - rshare
    for l in range(1, listed):
        lo, hi = level_off[l - 1], level_off[l]
        rows, cols = np.nonzero(interior[lo:hi])
        kids = child[lo:hi][rows, cols]
        start[kids] = start[lo + rows] + at[lo + rows, cols]
        rstart[kids] = rstart[lo + rows] + rat[lo + rows, cols]
        key[kids] = key[lo + rows] << np.uint64(3) | cols.astype(np.uint64)

    # emit: every voxel lane of the listed levels
    m = level_off[listed]
    rows, cols = np.nonzero(voxel[:m])
    where = start[rows] + at[rows, cols]
    cell = key[rows] << np.uint64(3) | cols.astype(np.uint64)  # (with the leading 1)
    lvl = level_of[rows]
    value = (pointer[rows, cols] - VOXEL_OFFSET).astype(np.uint32)
    xyz = np.zeros((count, 3), dtype=np.uint32)
    val, lev = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    record = (lvl < depth) if expand else np.zeros(rows.size, dtype=bool)
    for l in range(1, listed + 1):
        pick = (lvl == l) & ~record
        plain = cell[pick] ^ (np.uint64(1) << np.uint64(3 * l))
        xyz[where[pick]] = demorton(plain, l) << np.uint32(depth - l)
        val[where[pick]], lev[where[pick]] = value[pick], l
    if n_rec:
        rec_start, rec_key, rec_value = (np.zeros(n_rec, dtype=t) for t in (np.int64, np.uint64, np.uint32))
        j = rstart[rows[record]] + rat[rows[record], cols[record]]
        rec_start[j], rec_key[j], rec_value[j] = where[record], cell[record], value[record]
        assert (np.diff(rec_start) > 0).all()
        # one lane per output entry: the last record that starts at or before it, if it reaches that far
        i = np.arange(count)
        r = np.searchsorted(rec_start, i, side="right") - 1
        rec_level = np.array([(int(k).bit_length() - 1) // 3 for k in rec_key], dtype=np.int64)
        ok = r >= 0
        r = np.where(ok, r, 0)
        below = 3 * (depth - rec_level[r])
        suffix = i - rec_start[r]
        ok &= suffix < (np.int64(1) << below)
        full = ((rec_key[r] ^ (np.uint64(1) << (3 * rec_level[r]).astype(np.uint64))) << below.astype(np.uint64)) | suffix.astype(np.uint64)
        xyz[ok] = demorton(full[ok], depth)
        val[ok], lev[ok] = rec_value[r[ok]], depth
    return xyz, val, lev
