"""Restatements of the in-place tree edit's contract (csrc/svo_edit.hip) over GPU-layout words.

edit()          the host model, sequentially: put(p, leaf, depth) once per distinct cell in ascending Morton-key order,
                the last of several voxels in one cell winning; a leaf split on the way down gets 8 empty children
                appended at the end.
edit_parallel() the same result the way the kernels reach it: a read-only plan per voxel (l0 from a walk of the words
                as they are, c from the predecessor's key, l = max(l0, c + 1)), an exclusive scan of the group counts,
                a fill of the new groups and a link pass in which no two voxels write the same word.
"""
import numpy as np

from build_ref import EMPTY, VOXEL_OFFSET, morton


class Refused(ValueError):
    """A cell is an interior node at `depth`: the tree is finer there than the edit.  index = the voxel's input index."""

    def __init__(self, index):
        super().__init__(f"voxel {index} is an interior node at the edit's depth")
        self.index = index


def distinct(coords, depth, colours=None, colour=0xFFFFFF):
    """(keys ascending, 24-bit colours, input indices) of the distinct cells: of several voxels in one cell the last."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    n = c.shape[0]
    if n:
        assert c.min() >= 0 and c.max() < (1 << depth)
    col = (np.asarray(colours, dtype=np.int64).reshape(-1) if colours is not None else np.full(n, colour, dtype=np.int64)) & 0xFFFFFF
    keys, first = np.unique(morton(c, depth)[::-1], return_index=True)
    index = n - 1 - first
    return keys, col[index], index


def child(key, level, depth):
    return (int(key) >> (3 * (depth - level))) & 7


def edit(words, n_words, coords, depth, colours=None, colour=0xFFFFFF):
    """The words after the edit (np.uint32, n_words + 8 * groups created); raises Refused."""
    assert n_words >= 8 and n_words % 8 == 0
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)[:n_words]]
    for key, col, index in zip(*distinct(coords, depth, colours, colour)):
        base = 0
        for level in range(1, depth + 1):
            at = base + child(key, level, depth)
            pointer = w[at] >> 4
            if level == depth:
                if pointer < VOXEL_OFFSET:
                    raise Refused(int(index))
                w[at] = (VOXEL_OFFSET + int(col)) << 4
            elif pointer >= VOXEL_OFFSET:  # a leaf above `depth`: split it, the children are empty
                base = len(w)
                w[at] = base << 4
                w.extend([EMPTY] * 8)
            else:
                base = pointer
    return np.array(w, dtype=np.uint32)


def plan(words, n_words, keys, depth):
    """Per distinct voxel, reading only: l0 (level of the first leaf on its path), that leaf's index, refused."""
    m = keys.size
    l0 = np.zeros(m, dtype=np.int64)
    leaf_at = np.zeros(m, dtype=np.int64)
    refused = np.zeros(m, dtype=bool)
    for k in range(m):
        base = 0
        for level in range(1, depth + 1):
            at = base + child(keys[k], level, depth)
            pointer = int(words[at]) >> 4
            if pointer >= VOXEL_OFFSET:
                l0[k], leaf_at[k] = level, at
                break
            if level == depth:
                refused[k] = True
            base = pointer
    return l0, leaf_at, refused


def edit_parallel(words, n_words, coords, depth, colours=None, colour=0xFFFFFF):
    words = np.asarray(words, dtype=np.uint32)[:n_words]
    keys, col, index = distinct(coords, depth, colours, colour)
    m = keys.size
    if m == 0:
        return words.copy()
    l0, leaf_at, refused = plan(words, n_words, keys, depth)
    if refused.any():
        raise Refused(int(index[np.flatnonzero(refused)[0]]))
    # c: the leading levels shared with the predecessor; l: the level of the leaf the host finds when it gets to k
    ik = [int(k) for k in keys]
    c = np.zeros(m, dtype=np.int64)
    for k in range(1, m):
        x = ik[k] ^ ik[k - 1]
        c[k] = (3 * depth - x.bit_length()) // 3
    lvl = np.maximum(l0, c + 1)
    lvl[0] = l0[0]
    groups = depth - lvl
    start = np.cumsum(groups) - groups  # exclusive scan
    out = np.concatenate([words.astype(np.int64), np.full(8 * int(groups.sum()), EMPTY, dtype=np.int64)])  # fill
    written = np.zeros(out.size, dtype=bool)
    for k in range(m):  # link
        l = int(lvl[k])
        if l == l0[k]:
            at = int(leaf_at[k])
        else:  # the slot in the group that the head of the run sharing c levels made below the shared prefix
            shift = 3 * (depth - int(c[k]))
            head = int(np.searchsorted(keys, np.uint64((ik[k] >> shift) << shift), side="left"))
            at = n_words + 8 * int(start[head] + c[k] - lvl[head]) + child(ik[k], l, depth)
        for j in range(l, depth):
            group = n_words + 8 * int(start[k] + j - l)
            assert not written[at]
            written[at] = True
            out[at] = group << 4
            at = group + child(ik[k], j + 1, depth)
        assert not written[at]
        written[at] = True
        out[at] = (VOXEL_OFFSET + int(col[k])) << 4
    return out.astype(np.uint32)
