"""numpy restatement of the chunk-tree and world builder's contract (csrc/svo_build.hip): voxels split into
chunks by the top world_depth bits of their cells, every chunk a breadth-first tree in the host CpuOctree layout (the
level logic of build_ref.build), mips by integer means, and the <id>.bin bytes of every chunk.  relayout() puts a host
CpuOctree into the same breadth-first order, so trees built on the host compare node for node."""
import numpy as np

import build_ref as B

CHUNK_OFFSET = 1 << 31


def mip(rgb8):
    """(k, 8, 3) children -> (k, 3): per channel max(1, sum // count) over the non-(0,0,0) children, 1 when none"""
    rgb8 = np.asarray(rgb8, dtype=np.int64)
    nz = rgb8.any(axis=2)
    cnt = nz.sum(1)
    s = (rgb8 * nz[..., None]).sum(1)
    return np.maximum(s // np.maximum(cnt, 1)[:, None], 1)


def split_rgb(colours):
    c = np.asarray(colours, dtype=np.int64) & 0xFFFFFF
    return np.stack([c >> 16, (c >> 8) & 0xFF, c & 0xFF], 1)


def chunk_tree(keys, colours, depth):
    """sorted unique Morton keys (3 * depth bits) and their colours -> (pointers, rgb (n, 3), top_mip (3,))"""
    keys = np.asarray(keys, dtype=np.uint64)
    levels = {depth: keys}
    for lvl in range(depth - 1, 0, -1):
        levels[lvl] = np.unique(levels[lvl + 1] >> np.uint64(3))
    levels[0] = np.zeros(1, dtype=np.uint64)
    base = {1: 0}
    for lvl in range(1, depth):
        base[lvl + 1] = base[lvl] + 8 * levels[lvl - 1].size
    n = base[depth] + 8 * levels[depth - 1].size
    ptr = np.full(n, CHUNK_OFFSET, dtype=np.int64)
    rgb = np.zeros((n, 3), dtype=np.int64)
    at = {}
    for lvl in range(1, depth + 1):
        k = levels[lvl]
        parent = np.searchsorted(levels[lvl - 1], k >> np.uint64(3))
        dst = base[lvl] + 8 * parent + (k & np.uint64(7)).astype(np.int64)
        if lvl == depth:
            rgb[dst] = split_rgb(colours)
        else:
            ptr[dst] = base[lvl + 1] + 8 * np.arange(k.size)
        at[lvl] = dst
    for lvl in range(depth - 1, 0, -1):  # bottom-up
        d = at[lvl]
        rgb[d] = mip(rgb[ptr[d][:, None] + np.arange(8)])
    return ptr.astype(np.uint32), rgb.astype(np.uint8), mip(rgb[None, 0:8])[0].astype(np.uint8)


def to_bin(ptr, rgb):
    """<id>.bin bytes: LE u32 pointer, r, g, b, 0 per node"""
    out = np.zeros((ptr.size, 8), dtype=np.uint8)
    out[:, 0:4] = np.asarray(ptr, dtype="<u4").view(np.uint8).reshape(-1, 4)
    out[:, 4:7] = rgb
    return out.tobytes()


def leaves(coords, depth, colours=None, colour=0xFFFFFF):
    """last-wins unique cells: (sorted Morton keys, colours, cells)"""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    n = c.shape[0]
    col = (np.asarray(colours, dtype=np.int64).reshape(-1) if colours is not None else np.full(n, colour, dtype=np.int64)) & 0xFFFFFF
    key = B.morton(c, depth)
    keys, first = np.unique(key[::-1], return_index=True)
    keep = n - 1 - first
    return keys, col[keep], c[keep]


def tree(coords, depth, colours=None, colour=0xFFFFFF):
    """CpuOctree.build: (pointers, rgb, top_mip), or None for no voxels"""
    if len(coords) == 0:
        return None
    keys, col, _ = leaves(coords, depth, colours, colour)
    return chunk_tree(keys, col, depth)


def world(coords, depth, world_depth, colours=None, colour=0xFFFFFF):
    """World.build_world's chunks: {id: (bin bytes, top_mip)} in id order, id = CHUNK_OFFSET / 2 + (cx * s + cy) * s + cz"""
    out = {}
    if len(coords) == 0:
        return out
    keys, col, cells = leaves(coords, depth, colours, colour)
    cd, s = depth - world_depth, 1 << world_depth
    ch = cells >> cd
    cid = (ch[:, 0] * s + ch[:, 1]) * s + ch[:, 2]
    mask = np.uint64((1 << (3 * cd)) - 1)
    for i in np.unique(cid):
        sel = cid == i
        ptr, rgb, top = chunk_tree(keys[sel] & mask, col[sel], cd)
        out[CHUNK_OFFSET // 2 + int(i)] = (to_bin(ptr, rgb), top)
    return out


def relayout(ptrs, rgb):
    """a host CpuOctree's (raw() pointers, rgb) in canonical breadth-first order: root group first, every level's groups
    in the order of their parents"""
    ptrs = np.asarray(ptrs, dtype=np.int64)
    groups = [0]
    new_of = {0: 0}
    head = 0
    while head < len(groups):
        g = groups[head]
        head += 1
        for c in range(8):
            p = int(ptrs[g + c])
            if p < CHUNK_OFFSET:
                new_of[p] = 8 * len(groups)
                groups.append(p)
    order = (np.asarray(groups, dtype=np.int64)[:, None] + np.arange(8)).reshape(-1)
    out = ptrs[order].copy()
    interior = out < CHUNK_OFFSET
    out[interior] = [new_of[int(p)] for p in out[interior]]
    return out.astype(np.uint32), np.asarray(rgb)[order].astype(np.uint8)


def host_tree(pkg, coords, depth, colours=None, colour=0xFFFFFF):
    """the host path: sequential put_in_voxel(cell / 2^depth * 2 - 1) + generate_mip_tree, relayouted"""
    t = pkg.CpuOctree()
    col = np.asarray(colours, dtype=np.int64) if colours is not None else np.full(len(coords), colour, dtype=np.int64)
    rgb = split_rgb(col)
    for (x, y, z), (r, g, b) in zip(np.asarray(coords, dtype=np.int64), rgb):
        pos = [float(v) / (1 << depth) * 2.0 - 1.0 for v in (x, y, z)]
        t.put_in_voxel(pos, pkg.Voxel(r, g, b), depth)
    top = t.generate_mip_tree()
    ptrs, rgb = relayout(*t.raw())
    return ptrs, rgb, np.array([top.r, top.g, top.b], dtype=np.uint8)
