"""Restatements of the structure scattering contract (csrc/svo_structure.hip) over GPU-layout words.

column_tops()           literally the rule: sample_ref.sample down each column of the rectangle from y_hi - 1 to y_lo, the
                        first cell whose value is not 0.  Returns (top, value), uint32 arrays of shape size_xz, [x, z].
column_tops_skipping()  the same arrays the way the kernel reaches them: one walk per column that keeps the groups of its
                        path by level, jumps below an empty word's whole cube and goes on from the deepest group that the
                        old and the new cell share.  No pointer is followed before it passed the check (the guard is an
                        assertion), and every step goes a level down or moves y down.
sites()                 the hash and the four tests of a site; (origins int32 (N, 3), rots uint32 (N)) in the arrays' order.
stamp()                 placements x structure, clipped to the grid: (xyz uint32 (N, 3), colour, placement).
load_structure()        the position, index and colour rule of a structure's voxels from a decoded .vox model.
"""
import numpy as np

import sample_ref as S
from build_ref import VOXEL_OFFSET
from compact_ref import check_length

TOP_NONE = 0xFFFFFFFF
ROTATE = 1
REACH = 1 << 22


def check_columns(origin_xz, size_xz, depth, y_lo, y_hi):
    S.check_depth(depth)
    if not 0 <= y_lo < y_hi <= 1 << depth:
        raise ValueError(f"the y range {(y_lo, y_hi)} must be y_lo < y_hi <= 2^{depth}")
    if len(origin_xz) != 2 or len(size_xz) != 2 or any(o < 0 or s < 0 or o + s > 1 << depth for o, s in zip(origin_xz, size_xz)):
        raise ValueError(f"the rectangle {tuple(origin_xz)} + {tuple(size_xz)} leaves the depth-{depth} grid")
    if size_xz[0] * size_xz[1] >= 1 << 31:
        raise ValueError("the rectangle has 2^31 columns or more")


def columns(origin_xz, size_xz):
    """(x, z) of the rectangle's columns, flat, z fastest"""
    x, z = np.meshgrid(np.arange(origin_xz[0], origin_xz[0] + size_xz[0], dtype=np.int64),
                       np.arange(origin_xz[1], origin_xz[1] + size_xz[1], dtype=np.int64), indexing="ij")
    return x.reshape(-1), z.reshape(-1)


def column_tops(words, n_words, origin_xz, size_xz, depth, y_lo=0, y_hi=None, chunk=1 << 21):
    y_hi = 1 << depth if y_hi is None else y_hi
    check_length(words, n_words)
    check_columns(origin_xz, size_xz, depth, y_lo, y_hi)
    x, z = columns(origin_xz, size_xz)
    top, value = np.full(x.size, TOP_NONE, dtype=np.uint32), np.zeros(x.size, dtype=np.uint32)
    ys = np.arange(y_hi - 1, y_lo - 1, -1, dtype=np.int64)  # from the top down
    per = max(1, chunk // ys.size)
    for first in range(0, x.size, per):
        cx, cz = x[first:first + per], z[first:first + per]
        cells = np.stack([np.repeat(cx, ys.size), np.tile(ys, cx.size), np.repeat(cz, ys.size)], axis=1)
        v = S.sample(words, n_words, cells, depth)[0].reshape(cx.size, ys.size)
        hit = v != 0
        found = hit.any(axis=1)
        at = hit.argmax(axis=1)  # the first from the top
        top[first:first + per][found] = ys[at[found]]
        value[first:first + per][found] = v[np.flatnonzero(found), at[found]]
    return top.reshape(tuple(size_xz)), value.reshape(tuple(size_xz))


def column_tops_skipping(words, n_words, origin_xz, size_xz, depth, y_lo=0, y_hi=None):
    y_hi = 1 << depth if y_hi is None else y_hi
    check_length(words, n_words)
    check_columns(origin_xz, size_xz, depth, y_lo, y_hi)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    x, z = columns(origin_xz, size_xz)
    n = x.size
    top, value = np.full(n, TOP_NONE, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    y = np.full(n, y_hi - 1, dtype=np.int64)
    level, group = np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    stack = np.zeros((depth, n), dtype=np.int64)  # stack[l - 1]: the group of level l on the column's path
    live = np.arange(n)
    while live.size:
        lv = level[live]
        i = group[live] + S.child(x[live], y[live], z[live], depth - lv)
        assert (i < n_words).all(), "a word outside the tree would be read"
        ptr = w[i] >> 4
        leaf = ptr >= VOXEL_OFFSET
        coloured = ptr > VOXEL_OFFSET
        finer = ~leaf & (lv >= depth)
        broken = ~leaf & ~finer & ((ptr % 8 != 0) | (ptr + 8 > n_words))
        stop = coloured | finer | broken
        top[live[stop]] = y[live[stop]]
        value[live[stop]] = np.where(coloured, ptr - VOXEL_OFFSET, np.where(finer, S.FINER, S.BROKEN))[stop]
        # an empty cube of level lv: on below it, from the deepest group the two cells share
        e = live[leaf & ~coloured]
        shift = depth - level[e]
        floor = y[e] >> shift << shift
        go = e[floor > y_lo]
        nxt = floor[floor > y_lo] - 1
        differ = y[go] ^ nxt
        b = sum(((differ >> k) != 0).astype(np.int64) for k in range(1, depth + 1))  # the highest bit set
        assert (depth - b <= level[go]).all() and (depth - b >= 1).all()
        level[go] = depth - b
        group[go] = stack[level[go] - 1, go]
        y[go] = nxt
        # an interior word that passed the check: one level down
        d = live[~leaf & ~finer & ~broken]
        group[d] = ptr[~leaf & ~finer & ~broken]
        stack[level[d], d] = group[d]
        level[d] += 1
        live = np.concatenate([go, d])
    return top.reshape(tuple(size_xz)), value.reshape(tuple(size_xz))


def lowbias32(v):
    v = np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF
    v ^= v >> np.uint64(16)
    v = (v * np.uint64(0x7feb352d)) & 0xFFFFFFFF
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x846ca68b)) & 0xFFFFFFFF
    v ^= v >> np.uint64(16)
    return v


def site_hash(x, z, seed):
    x, z = np.asarray(x, dtype=np.uint64), np.asarray(z, dtype=np.uint64)
    return lowbias32(lowbias32((x + np.uint64(seed)) & 0xFFFFFFFF) ^ z)


def sites(tops, values, origin_xz, one_in, seed=0, on_value=0, lift=1, flags=ROTATE):
    if one_in < 1:
        raise ValueError("one_in must be at least 1")
    if values is None and on_value:
        raise ValueError("on_value needs the values")
    tops = np.asarray(tops).astype(np.int64) & 0xFFFFFFFF
    x, z = columns(origin_xz, tops.shape)
    t = tops.reshape(-1)
    ok = t != TOP_NONE
    if values is not None:
        v = np.asarray(values).astype(np.int64).reshape(-1) & 0xFFFFFFFF
        ok &= v < VOXEL_OFFSET
        if on_value:
            ok &= v == on_value
    h = site_hash(x, z, seed)
    ok &= h % np.uint64(one_in) == 0
    origins = np.stack([x[ok], (t[ok] + lift) & 0xFFFFFFFF, z[ok]], axis=1).astype(np.uint32).view(np.int32)
    rots = (lowbias32(h[ok] + np.uint64(0x9E3779B9)) >> np.uint64(30)).astype(np.uint32) if flags & ROTATE else np.zeros(int(ok.sum()), dtype=np.uint32)
    return origins.reshape(-1, 3), rots


def rotate(offsets, r):
    """R^r of (m, 3) offsets: R (dx, dy, dz) = (dz, dy, -dx)"""
    o = np.asarray(offsets, dtype=np.int64).reshape(-1, 3)
    for _ in range(int(r)):
        o = np.stack([o[:, 2], o[:, 1], -o[:, 0]], axis=1)
    return o


class BadInput(ValueError):
    pass


def stamp(offsets, colours, origins, rots, depth):
    S.check_depth(depth)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 3)
    origins = np.asarray(origins, dtype=np.int64).reshape(-1, 3)
    colours = np.asarray(colours, dtype=np.int64).reshape(-1) & 0xFFFFFFFF
    rots = np.zeros(len(origins), dtype=np.int64) if rots is None else np.asarray(rots, dtype=np.int64).reshape(-1)
    if len(origins) * len(offsets) >= 1 << 31:
        raise BadInput("2^31 entries or more")
    for name, bad in (("origin", ((origins < -REACH) | (origins >= REACH)).any(axis=1)), ("rotation", (rots < 0) | (rots >= 4))):
        if bad.any():
            raise BadInput(f"placement {int(np.flatnonzero(bad)[0])}: {name}")
    bad = (np.abs(offsets) >= REACH).any(axis=1)
    if bad.any():
        raise BadInput(f"voxel {int(np.flatnonzero(bad)[0])}: offset")
    xyz, colour, placement = [], [], []
    turned = [rotate(offsets, r) for r in range(4)]
    for p, (origin, r) in enumerate(zip(origins, rots)):
        cells = origin + turned[r]
        inside = ((cells >= 0) & (cells < 1 << depth)).all(axis=1)
        xyz.append(cells[inside])
        colour.append(colours[inside])
        placement.append(np.full(int(inside.sum()), p, dtype=np.int64))
    cat = lambda parts, shape: np.concatenate(parts).astype(np.uint32) if parts else np.zeros(shape, dtype=np.uint32)  # noqa: E731
    return cat(xyz, (0, 3)).reshape(-1, 3), cat(colour, 0), cat(placement, 0)


def load_structure(size, xyzi, palette):
    """(offsets int32 (m, 3), index uint32, colours uint32) of a decoded model: offset (size.x / 2 - x, z, y - size.y / 2)
    in integer division, voxel.i = file colour index - 1 (0 for a file index of 0), index = voxel.i + 1, colour
    0x00RRGGBB of the little-endian RGBA word palette[voxel.i]"""
    xyzi = np.asarray(xyzi, dtype=np.int64).reshape(-1, 4)
    pal = np.asarray(palette, dtype=np.int64)
    i = np.where(xyzi[:, 3] > 0, xyzi[:, 3] - 1, 0)
    rgba = pal[i]
    offsets = np.stack([int(size[0]) // 2 - xyzi[:, 0], xyzi[:, 2], xyzi[:, 1] - int(size[1]) // 2], axis=1)
    colours = (rgba & 0xFF) << 16 | (rgba >> 8 & 0xFF) << 8 | (rgba >> 16 & 0xFF)
    return offsets.astype(np.int32), (i + 1).astype(np.uint32), colours.astype(np.uint32)
