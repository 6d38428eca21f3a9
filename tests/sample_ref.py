"""Restatements of the sampling contract (csrc/svo_sample.hip) over GPU-layout words.

sample()         the rule for one cell, from the contract, applied to every cell of a list: the walk from group 0 by the
                 cell's child indices, level by level.  Returns (value, level, index), uint32 arrays of one entry per cell.
sample_dense()   sample() over the cells of a box: the values as a uint32 array of shape `size`, indexed [x, y, z].
sample_bricks()  the same array the way the dense kernel reaches it: waves of RUN aligned 4x4x4 bricks along z, one walk
                 of the common levels 1 .. depth - 2 per brick, which settles the brick when it ends on a leaf or a broken
                 pointer, then every lane's last two levels, lanes outside the box storing nothing.

The marks: FINER where the tree is interior at `depth`, OUTSIDE for a coordinate >= 2^depth, BROKEN where the path met a
pointer that is unaligned or leaves the words.  No walk follows a pointer before it passed that check (the guard is an
assertion here), and none takes more than `depth` steps, so every tree terminates.
"""
import numpy as np

from build_ref import VOXEL_OFFSET
from compact_ref import check_length

FINER, OUTSIDE, BROKEN = 1 << 28, 1 << 29, 1 << 30
NO_INDEX = 0xFFFFFFFF
RUN = 4  # bricks along z per wave


def check_depth(depth):
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")


def child(x, y, z, bit):
    return ((x >> bit) & 1) << 2 | ((y >> bit) & 1) << 1 | ((z >> bit) & 1)


def walk(w, n_words, x, y, z, depth, first, group):
    """the rule from level `first` on, for cells whose group of that level is `group`; int64 arrays"""
    n = x.size
    value, level, index = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    group = np.array(group, dtype=np.int64)
    live = np.arange(n)
    for l in range(first, depth + 1):
        if not live.size:
            break
        i = group[live] + child(x[live], y[live], z[live], depth - l)
        assert (i < n_words).all(), "a word outside the tree would be read"
        ptr = w[i] >> 4
        leaf = ptr >= VOXEL_OFFSET
        finer = ~leaf & (l == depth)
        broken = ~leaf & ~finer & ((ptr % 8 != 0) | (ptr + 8 > n_words))
        stop = leaf | finer | broken
        value[live[stop]] = np.where(leaf, ptr - VOXEL_OFFSET, np.where(finer, FINER, BROKEN))[stop]
        level[live[stop]], index[live[stop]] = l, i[stop]
        group[live[~stop]] = ptr[~stop]
        live = live[~stop]
    assert not live.size
    return value, level, index


def sample(words, n_words, cells, depth):
    check_length(words, n_words)
    check_depth(depth)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    c = (np.asarray(cells).reshape(-1, 3).astype(np.int64)) & 0xFFFFFFFF  # (u32 bit patterns)
    inside = (c < (1 << depth)).all(axis=1)
    value, level, index = (np.full(len(c), fill, dtype=np.uint32) for fill in (OUTSIDE, 0, NO_INDEX))
    x, y, z = c[inside].T
    value[inside], level[inside], index[inside] = walk(w, n_words, x, y, z, depth, 1, np.zeros(x.size, dtype=np.int64))
    return value, level, index


def box_cells(origin, size):
    """the cells of a box, (N, 3), in the order of the [x, y, z] array"""
    axes = [np.arange(o, o + s, dtype=np.int64) for o, s in zip(origin, size)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def check_box(origin, size, depth):
    check_depth(depth)
    if len(origin) != 3 or len(size) != 3 or any(o < 0 or s < 0 or o + s > 1 << depth for o, s in zip(origin, size)):
        raise ValueError(f"the box {tuple(origin)} + {tuple(size)} leaves the depth-{depth} grid")
    if size[0] * size[1] * size[2] >= 1 << 31:
        raise ValueError("the box has 2^31 cells or more")


def sample_dense(words, n_words, origin, size, depth):
    check_box(origin, size, depth)
    return sample(words, n_words, box_cells(origin, size), depth)[0].reshape(tuple(size))


def sample_bricks(words, n_words, origin, size, depth):
    check_length(words, n_words)
    check_box(origin, size, depth)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    origin, size = np.array(origin, dtype=np.int64), np.array(size, dtype=np.int64)
    grid = np.full(tuple(size), 0xDEADBEEF, dtype=np.uint32)
    if not size.all():
        return grid
    end = origin + size
    top = max(depth - 2, 0)  # the levels of the common path

    # the waves: one per run of RUN bricks along z, over the bricks that meet the box
    b0 = origin >> 2
    bricks = ((end - 1) >> 2) - b0 + 1
    runs = -(-bricks[2] // RUN)
    bx, by, rz = (a.reshape(-1) for a in np.meshgrid(b0[0] + np.arange(bricks[0]), b0[1] + np.arange(bricks[1]), np.arange(runs),
                                                     indexing="ij"))
    bz = b0[2] + rz * RUN

    # the common walk of every brick of every run: the group its lanes go on from, or settled with one value for all
    settled = np.ones((bx.size, RUN), dtype=bool)
    value = np.zeros((bx.size, RUN), dtype=np.int64)
    group = np.zeros((bx.size, RUN), dtype=np.int64)
    for r in range(RUN):
        met = np.flatnonzero((bz + r) * 4 < end[2])  # (the others lie behind the box: none of their lanes stores)
        g = np.zeros(met.size, dtype=np.int64)
        live = np.arange(met.size)
        settled[met, r] = False
        for l in range(1, top + 1):
            i = g[live] + child(bx[met][live], by[met][live], bz[met][live] + r, top - l)
            assert (i < n_words).all(), "a word outside the tree would be read"
            ptr = w[i] >> 4
            leaf = ptr >= VOXEL_OFFSET
            broken = ~leaf & ((ptr % 8 != 0) | (ptr + 8 > n_words))
            stop = leaf | broken
            settled[met[live[stop]], r] = True
            value[met[live[stop]], r] = np.where(leaf, ptr - VOXEL_OFFSET, BROKEN)[stop]
            g[live[~stop]] = ptr[~stop]
            live = live[~stop]
        group[met, r] = g

    # the lanes: z = lane & 15 runs fastest, y = lane >> 4, one x per step; a lane's brick of the run is (lane >> 2) & 3
    lane = np.arange(64)
    mine = (lane >> 2) & (RUN - 1)
    for step in range(4):
        x = np.broadcast_to((bx * 4 + step)[:, None], (bx.size, 64))
        y = (by * 4)[:, None] + (lane >> 4)[None, :]
        z = (bz * 4)[:, None] + (lane & 15)[None, :]
        inside = ((x >= origin[0]) & (x < end[0]) & (y >= origin[1]) & (y < end[1]) & (z >= origin[2]) & (z < end[2]))
        done, val, grp = settled[:, mine], value[:, mine], group[:, mine]
        assert not (inside & done & ((bz[:, None] + mine[None, :]) * 4 >= end[2])).any()
        out = val.copy()
        own = inside & ~done
        out[own] = walk(w, n_words, x[own], y[own], z[own], depth, top + 1, grp[own])[0]
        grid[x[inside] - origin[0], y[inside] - origin[1], z[inside] - origin[2]] = out[inside]
    return grid
