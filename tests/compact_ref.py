"""Restatements of the compaction's contract (csrc/svo_compact.hip) over GPU-layout words.

compact()          from the contract, sequentially: the groups reachable from group 0 breadth-first, each level in the
                   order of its parents; with `prune` a group is dead when each word, counter ignored, is the empty word
                   or points at a dead group (the root never is), a word pointing at a dead group becomes the empty
                   word and dead groups are dropped; pointers rewritten, counters kept.
compact_parallel() the same result the way the kernels reach it: discover(), live bottom-up per level, emit().
discover()         the walk that the compaction, the simplification and the listing share (svo_tree_discover): per level
                   the interior counts of the frontier, their exclusive scan, the children scattered behind the
                   frontier; plain stores of new_of and the test for a group reached twice.  simplify_ref and list_ref
                   call it.
emit()             the canonical layout that the compaction and the simplification share (svo_tree_rewrite::finish): one
                   scan of the kept groups, then every kept group's words with the interior ones rewritten by the
                   child's fate.

compact() and compact_parallel() return (out, perm) with perm[new word] = old word and raise Malformed on a tree the device refuses.
"""
import numpy as np

from build_ref import EMPTY, VOXEL_OFFSET

MAX_LEVELS = 31
KEEP = 0xFFFFFFFF  # a group's fate: it stays (any other: the 28-bit field that its parent's word becomes)


class Malformed(ValueError):
    def __init__(self, why):
        super().__init__(f"malformed tree: {why}")


def check_length(words, n_words):
    if n_words < 8 or n_words % 8 or n_words > len(words):
        raise ValueError(f"n_words must be a positive multiple of 8 within the words (got {n_words})")


def compact(words, n_words, prune):
    check_length(words, n_words)
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)[:n_words]]
    order, kids, seen = [], {}, set()  # old group starts breadth-first; a group's interior children (slot, group)
    level, frontier = 1, [0]
    while frontier:
        if level > MAX_LEVELS:
            raise Malformed(f"deeper than {MAX_LEVELS} levels")
        below = []
        for g in frontier:
            if g in seen:
                raise Malformed("a group is reached twice")
            seen.add(g)
            order.append(g)
            kids[g] = []
            for c in range(8):
                pointer = w[g + c] >> 4
                if pointer < VOXEL_OFFSET:
                    if pointer % 8:
                        raise Malformed("a pointer is not a multiple of 8")
                    if pointer + 8 > n_words:
                        raise Malformed("a pointer leaves the words")
                    kids[g].append((c, pointer))
                    below.append(pointer)
        frontier, level = below, level + 1
    dead = set()
    if prune:
        for g in reversed(order):  # children before parents
            interior = dict(kids[g])
            if g and all(interior[c] in dead if c in interior else w[g + c] >> 4 == VOXEL_OFFSET for c in range(8)):
                dead.add(g)
    kept = [g for g in order if g not in dead]
    new_of = {g: 8 * k for k, g in enumerate(kept)}
    out, perm = [], []
    for g in kept:
        interior = dict(kids[g])
        for c in range(8):
            word = w[g + c]
            if c in interior:
                word = EMPTY if interior[c] in dead else new_of[interior[c]] << 4 | word & 15
            out.append(word)
            perm.append(g + c)
    return np.array(out, dtype=np.uint32), np.array(perm, dtype=np.uint32)


def exclusive_scan(a):
    return np.cumsum(a) - a


def discover(w, n_words):
    """the discovery and the check of the int64 words w (svo_tree_discover): (order, first_child, level_off).  order grows
    by one frontier per level, first_child[k] indexes order, order[level_off[l]:level_off[l + 1]] is level l + 1"""
    cap = n_words // 8
    lanes = np.arange(8)
    order = np.zeros(1, dtype=np.int64)
    first_child = np.zeros(0, dtype=np.int64)
    level_off = [0]
    off, n, level = 0, 1, 1
    while True:
        g = w[order[off:off + n, None] + lanes]
        interior = (g >> 4) < VOXEL_OFFSET
        pointers = g[interior] >> 4  # row-major: scan + the interior lanes below
        if (pointers % 8).any():
            raise Malformed("a pointer is not a multiple of 8")
        if (pointers + 8 > n_words).any():
            raise Malformed("a pointer leaves the words")
        first_child = np.concatenate([first_child, off + n + exclusive_scan(interior.sum(axis=1))])
        if off + n + pointers.size > cap:
            raise Malformed("a group is reached twice (more groups than n_words / 8)")
        order = np.concatenate([order, pointers])
        off += n
        level_off.append(off)
        if not pointers.size:
            break
        if level == MAX_LEVELS:
            raise Malformed(f"deeper than {MAX_LEVELS} levels")
        n, level = pointers.size, level + 1
    # check: whichever of two stores wins, one of the two groups sees the other's number
    new_of = np.full(cap, -1, dtype=np.int64)
    new_of[order // 8] = np.arange(off)
    if (new_of[order // 8] != np.arange(off)).any():
        raise Malformed("a group is reached twice")
    return order, first_child, level_off


def group_words(w, order, first_child):
    """per group of order its (groups, 8) words, their interior mask and the children's indices in order (0 where the
    word is not interior)"""
    g = w[order[:, None] + np.arange(8)]
    interior = (g >> 4) < VOXEL_OFFSET
    return g, interior, np.where(interior, first_child[:, None] + np.cumsum(interior, axis=1) - interior, 0)


def emit(w, order, first_child, fate, cand):
    """the emit of the canonical layout (svo_tree_rewrite::finish): of the candidates order[:cand] the groups with fate KEEP
    stay, numbered by one scan; an interior word links its child's new place or becomes the leaf of the child's fate"""
    g, interior, child = (a[:cand] for a in group_words(w, order, first_child))
    kept = fate[:cand] == KEEP
    number = np.zeros(order.size, dtype=np.int64)
    number[:cand] = exclusive_scan(kept.astype(np.int64))
    to = fate[child]  # (a child behind the candidates has a fate too)
    linked = np.where(to == KEEP, (8 * number[child]) << 4 | g & 15, to << 4)
    out = np.where(interior, linked, g)[kept].reshape(-1)
    perm = (order[:cand, None] + np.arange(8))[kept].reshape(-1)
    return out.astype(np.uint32), perm.astype(np.uint32)


def compact_parallel(words, n_words, prune):
    check_length(words, n_words)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    order, first_child, level_off = discover(w, n_words)
    # prune: bottom-up, a launch per level
    live = np.ones(order.size, dtype=np.int64)
    if prune:
        g, interior, child = group_words(w, order, first_child)
        for l in range(len(level_off) - 2, -1, -1):
            lo, hi = level_off[l], level_off[l + 1]
            keeps = np.where(interior[lo:hi], live[child[lo:hi]] != 0, (g[lo:hi] >> 4) != VOXEL_OFFSET)
            live[lo:hi] = keeps.any(axis=1)
        live[0] = 1
    # emit: a dead group's parent word becomes the empty word
    return emit(w, order, first_child, np.where(live != 0, KEEP, VOXEL_OFFSET), order.size)
