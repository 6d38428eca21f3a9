"""numpy restatement of the GPU tree builder's contract (csrc/svo_build.hip): Morton keys, last-wins
dedupe, then one level at a time -- unique keys per level and every node's parent rank by searchsorted."""
import numpy as np

VOXEL_OFFSET = 1 << 27
EMPTY = VOXEL_OFFSET << 4


def morton(coords, depth):
    """key with level 1 in the top bits: child index at level L = x bit << 2 | y bit << 1 | z bit, bit depth - L"""
    c = np.asarray(coords, dtype=np.uint64).reshape(-1, 3)
    key = np.zeros(c.shape[0], dtype=np.uint64)
    for b in range(depth):
        for axis, pos in ((0, 2), (1, 1), (2, 0)):
            key |= ((c[:, axis] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + pos)
    return key


def build(coords, depth, colours=None, colour=0xFFFFFF):
    """The breadth-first words of the voxels' tree (np.uint32)."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    n = c.shape[0]
    if n == 0:
        return np.full(8, EMPTY, dtype=np.uint32)
    assert c.min() >= 0 and c.max() < (1 << depth)
    key = morton(c, depth)
    col = (np.asarray(colours, dtype=np.int64).reshape(-1) if colours is not None else np.full(n, colour, dtype=np.int64)) & 0xFFFFFF
    # last one wins: the first occurrence in the reversed list
    leaves, first = np.unique(key[::-1], return_index=True)
    leaf_col = col[::-1][first]
    levels = {depth: leaves}
    for lvl in range(depth - 1, 0, -1):
        levels[lvl] = np.unique(levels[lvl + 1] >> np.uint64(3))
    levels[0] = np.zeros(1, dtype=np.uint64)
    base = {1: 0}
    for lvl in range(1, depth):
        base[lvl + 1] = base[lvl] + 8 * levels[lvl - 1].size
    n_words = base[depth] + 8 * levels[depth - 1].size
    words = np.full(n_words, EMPTY, dtype=np.int64)
    for lvl in range(1, depth + 1):
        k = levels[lvl]
        parent = np.searchsorted(levels[lvl - 1], k >> np.uint64(3))
        dst = base[lvl] + 8 * parent + (k & np.uint64(7)).astype(np.int64)
        if lvl == depth:
            words[dst] = (VOXEL_OFFSET + leaf_col) << 4
        else:
            words[dst] = (base[lvl + 1] + 8 * np.arange(k.size)) << 4
    return words.astype(np.uint32)


def vox_voxels(size, xyzi, palette):
    """A .vox model's voxels as tree_from_voxels places them: cell (size-1-x, z, y), colour pal[i-1] as r<<16|g<<8|b."""
    xyzi = np.asarray(xyzi, dtype=np.int64).reshape(-1, 4)
    pal = np.asarray(palette, dtype=np.int64)
    rgba = pal[np.where(xyzi[:, 3] > 0, xyzi[:, 3] - 1, 0)]
    colours = (rgba & 0xFF) << 16 | (rgba >> 8 & 0xFF) << 8 | (rgba >> 16 & 0xFF)
    coords = np.stack([size - 1 - xyzi[:, 0], xyzi[:, 2], xyzi[:, 1]], 1)
    return coords, colours, int(size).bit_length() - 1


def dense_to_voxels(grid):
    """the non-zero cells of a (side, side, side) grid indexed [x, y, z] and their colours"""
    g = np.asarray(grid)
    coords = np.argwhere(g != 0)
    return coords, g[tuple(coords.T)].astype(np.int64) & 0xFFFFFF


BLOCKS = ("stone", "dirt", "grass", "wood", "leaf", "slate", "crystal", "glass")
FIXTURES = ("small", "monu9", "monu10", "defualt", "phantom_mansion", "blocks")


def fixture_models(golden, name):
    """[(label, size, xyzi, palette)] of a tests/golden/<name>_vox.npz: one model, or the 8 16^3 blocks of `blocks`"""
    import os
    z = np.load(os.path.join(golden, f"{name}_vox.npz"))
    if name != "blocks":
        return [(name, int(z["size"][0]), z["xyzi"], z["palette"])]
    return [(f"blocks/{b}", 16, z[b + "_xyzi"], z[b + "_palette"]) for b in BLOCKS]
