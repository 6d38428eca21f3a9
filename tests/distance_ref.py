"""Restatements of the distance contract (csrc/svo_distance.hip, include/svo_hip.h) over GPU-layout words.

occupancy()   the grown box [origin - R, origin + size + R) as a boolean array: True where sample_ref.sample gives a value
              other than 0 (a colour, FINER, BROKEN), False outside the grid.
grown(), brute_grid()  the same from the whole grid's sampled values, for many boxes of one tree.
brute()       the rule read literally: the offsets of the ball sorted by (d2, dx, dy, dz), each filling, with shifted
              slices, the cells that are still unset.  Gives d2 and the packed sites.
separable()   three window passes over packed keys d2 << 24 | x << 16 | y << 8 | z: the best over x' of the best over y'
              of the best over z'.  Gives the same two arrays: that they are equal is the decomposition.
edt_d2()      d2 alone from scipy.ndimage.distance_transform_edt of the grown box, squared and rounded.
from_sites()  for a tree given as a short list of its occupied cells: the rule by broadcasting over the list, any radius.

d2 is int32 (FAR where no site lies within R; in signed mode an occupied cell's value negated), the sites are uint32
(NO_SITE likewise), both of shape `size`, indexed [x, y, z].
"""
import numpy as np

import sample_ref as S

FAR, NO_SITE = 0x7FFFFFFF, 0xFFFFFFFF
TO_VOXELS, TO_EMPTY, SIGNED = 0, 1, 2
MAX_RADIUS = 127
INF = 1 << 62


def check(origin, size, depth, R, mode):
    S.check_box(origin, size, depth)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"max_distance must be 1..{MAX_RADIUS} (got {R})")
    if mode not in (TO_VOXELS, TO_EMPTY, SIGNED):
        raise ValueError(f"mode must be 0..2 (got {mode})")


def occupancy(words, n_words, depth, origin, size, R):
    lo = np.array(origin, dtype=np.int64) - R
    shape = tuple(int(s) + 2 * R for s in size)
    occ = np.zeros(shape, dtype=bool)
    side = 1 << depth
    first, last = np.maximum(lo, 0), np.minimum(lo + shape, side)  # the part inside the grid
    if (last > first).all():
        inside = S.sample(words, n_words, S.box_cells(first, last - first), depth)[0] != 0
        occ[tuple(slice(a - l, b - l) for a, b, l in zip(first, last, lo))] = inside.reshape(tuple(last - first))
    return occ


def ball(R):
    """the offsets with |o|^2 <= R^2 in the rule's order: (d2, dx, dy, dz), lexicographically"""
    r = np.arange(-R, R + 1)
    o = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    d2 = (o * o).sum(axis=1)
    o, d2 = o[d2 <= R * R], d2[d2 <= R * R]
    order = np.lexsort((o[:, 2], o[:, 1], o[:, 0], d2))
    return o[order], d2[order]


def pack(o):
    return (int(o[0]) + 128) << 16 | (int(o[1]) + 128) << 8 | (int(o[2]) + 128)


def brute_sites(site, size, R):
    """the rule over a boolean array of sites of the grown box"""
    d2 = np.full(tuple(size), FAR, dtype=np.int64)
    packed = np.full(tuple(size), NO_SITE, dtype=np.int64)
    unset = np.ones(tuple(size), dtype=bool)
    for o, d in zip(*ball(R)):
        if not unset.any():
            break
        hit = unset & site[tuple(slice(R + int(v), R + int(v) + n) for v, n in zip(o, size))]
        d2[hit], packed[hit] = d, pack(o)
        unset &= ~hit
    return d2, packed


def by_mode(occ, size, R, mode, rule):
    """d2 and sites of a mode from the rule over the voxels and over the empty cells of the grown box"""
    own = occ[R:R + size[0], R:R + size[1], R:R + size[2]]
    if mode == TO_VOXELS:
        d2, packed = rule(occ, size, R)
    elif mode == TO_EMPTY:
        d2, packed = rule(~occ, size, R)
    else:
        (dv, pv), (de, pe) = rule(occ, size, R), rule(~occ, size, R)
        d2, packed = np.where(own, -de, dv), np.where(own, pe, pv)
    return d2.astype(np.int32), packed.astype(np.uint32)


def grown(grid, origin, size, R):
    """occupancy()'s array from the whole grid's sampled values (sample_dense of [0, 2^depth)^3), for many boxes of one tree"""
    pad = np.pad(np.asarray(grid) != 0, R)
    return pad[tuple(slice(o, o + n + 2 * R) for o, n in zip(origin, size))]


def brute_grid(grid, origin, size, R, mode):
    """brute() over the whole grid's sampled values"""
    return by_mode(grown(grid, origin, size, R), size, R, mode, brute_sites)


def brute(words, n_words, depth, origin, size, R, mode):
    check(origin, size, depth, R, mode)
    return by_mode(occupancy(words, n_words, depth, origin, size, R), size, R, mode, brute_sites)


def window_min(keys, axis, n, R, shift):
    """min over d in [-R, R] of keys[.. + d ..] + (d * d << 24) + (d << shift) along `axis`, for the n cells behind the
    first R; INF stays INF"""
    best = np.full(tuple(n if a == axis else s for a, s in enumerate(keys.shape)), INF, dtype=np.int64)
    for d in range(-R, R + 1):
        part = keys[tuple(slice(R + d, R + d + n) if a == axis else slice(None) for a in range(3))]
        best = np.minimum(best, np.where(part < INF, part + (d * d << 24) + (d << shift), INF))
    return best


def separable_sites(site, size, R):
    keys = np.where(site, 128 << 16 | 128 << 8 | 128, INF).astype(np.int64)
    for axis, shift in ((2, 0), (1, 8), (0, 16)):
        keys = window_min(keys, axis, size[axis], R, shift)
    found = (keys >> 24) <= R * R
    return np.where(found, keys >> 24, FAR), np.where(found, keys & 0xFFFFFF, NO_SITE)


def separable(words, n_words, depth, origin, size, R, mode):
    check(origin, size, depth, R, mode)
    return by_mode(occupancy(words, n_words, depth, origin, size, R), size, R, mode, separable_sites)


def edt_d2(words, n_words, depth, origin, size, R, mode):
    from scipy.ndimage import distance_transform_edt

    def rule(site, size, R):
        d = distance_transform_edt(~site) if site.any() else np.full(site.shape, np.inf)
        d2 = np.where(np.isfinite(d), np.rint(d * d), FAR).astype(np.int64)[R:R + size[0], R:R + size[1], R:R + size[2]]
        return np.where(d2 <= R * R, d2, FAR), np.zeros(tuple(size), dtype=np.int64)

    check(origin, size, depth, R, mode)
    return by_mode(occupancy(words, n_words, depth, origin, size, R), size, R, mode, rule)[0]


def from_sites(cells, origin, size, R):
    """to-voxels mode for a tree whose occupied cells are the few rows of `cells`"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    c = S.box_cells(origin, size)
    o = cells[None, :, :] - c[:, None, :]
    d2 = (o * o).sum(axis=2)
    key = (d2 << 24) + ((o[..., 0] + 128) << 16) + ((o[..., 1] + 128) << 8) + (o[..., 2] + 128)
    key = np.where((d2 <= R * R) & (np.abs(o) <= R).all(axis=2), key, INF).min(axis=1)
    found = key < INF
    return (np.where(found, key >> 24, FAR).astype(np.int32).reshape(tuple(size)),
            np.where(found, key & 0xFFFFFF, NO_SITE).astype(np.uint32).reshape(tuple(size)))


def morph_ball(whole, origin, size, d2, packed, op, colour):
    """the per-cell contract of Render.morph_ball: `whole` is sample_dense of the whole grid before the call, d2 and packed
    brute's over the box with R = radius, to the voxels for "grow" and to the empty cells for "shrink".  Returns the whole
    grid afterwards and the changed cells of the box."""
    after = whole.copy()
    box = after[tuple(slice(o, o + n) for o, n in zip(origin, size))]
    changed = (d2 > 0) & (d2 != FAR)
    if op == "shrink":
        box[changed] = 0
    elif colour:
        box[changed] = colour
    else:
        p = packed[changed].astype(np.int64)
        site = S.box_cells(origin, size).reshape(tuple(size) + (3,))[changed] + np.stack([p >> 16 & 0xFF, p >> 8 & 0xFF, p & 0xFF], axis=1) - 128
        box[changed] = whole[site[:, 0], site[:, 1], site[:, 2]]
    return after, changed
