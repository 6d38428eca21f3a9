"""Restatements of the height-map edit's contract (include/svo_hip.h: svo_nodes_edit_heightmap) over GPU-layout
words, in numpy alone.

params()       the layers, the two modes and the colour above the ground as the dict the functions below take
apply_cells()  the per-cell contract on a dense [x, y, z] grid of values, by broadcasting (apply_columns: on the map's columns alone)
pyramid()      level s of the min/max pyramid over the map: the extremes per octree-aligned tile that meets the rectangle
edit()         the rule for one word, applied level by level from the root group: the new words and the tallies (the five
               of TALLIES, and "level_splits", the splits of each level)
table_cases()  the edits of the depth-7 base that the host and the GPU tests share

The frontier of a level is a list of words in order: the eight children, by child index, of every word of the level above
that was opened or split, those taken in frontier order.  The g-th split of the call gets the group n_words + 8 g.
"""
import numpy as np

from build_ref import VOXEL_OFFSET
from compact_ref import check_length

MODES = {None: 0, "empty": 1, "voxels": 2, "set": 3}
MODE_SET = 3
MAX_LAYERS = 8
NONE = 0xFFFFFFFF  # the identity of a minimum
TALLIES = ("splits", "collapses", "overwrites", "untouched", "opened")
GRASS, DIRT, STONE = 0x3A9D23, 0x8B5A2B, 0x808080
TERRAIN = ((1, GRASS), (3, DIRT), (0, STONE))


class Refused(Exception):
    """an interior word at `depth` under a mode that does not replace it: the cell"""

    def __init__(self, cell):
        super().__init__(f"the height map meets an interior node at cell {tuple(cell)}")
        self.cell = tuple(int(c) for c in cell)


def params(layers=((0, 0xFFFFFF),), below="set", above=None, above_colour=0):
    return {"layers": [(int(t), int(c) & 0xFFFFFF) for t, c in layers], "below": below, "above": above, "above_colour": int(above_colour) & 0xFFFFFF}


def check(H, origin, depth, p):
    """-> (the clamped heights as int64 [sx, sz], ox, oz, mode_below, mode_above, T (the bands' ends but the last), colours)"""
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    H = np.asarray(H)
    if H.ndim != 2 or H.size >= 1 << 31:
        raise ValueError(f"heights must be (sx, sz) with fewer than 2^31 columns, got {H.shape}")
    ox, oz = (int(v) for v in origin)
    if min(ox, oz) < 0 or ox + H.shape[0] > 1 << depth or oz + H.shape[1] > 1 << depth:
        raise ValueError(f"the rectangle at {(ox, oz)} of size {H.shape} leaves the depth-{depth} grid")
    below, above = MODES[p["below"]], MODES[p["above"]]
    layers = p["layers"]
    if len(layers) > MAX_LAYERS or (below and not layers):
        raise ValueError(f"{len(layers)} layers with mode_below {below}")
    T = np.cumsum([int(t) for t, _ in layers[:-1]], dtype=object).tolist() if len(layers) > 1 else []  # (Python integers: no wrap)
    h = np.minimum(H.astype(np.uint64), np.uint64(1 << depth)).astype(np.int64)
    return h, ox, oz, below, above, [int(t) for t in T], np.array([c for _, c in layers] or [0], dtype=np.int64)


def _band(d, T):
    """the layer index of the cells d >= 0 below the ground's top cell"""
    k = np.zeros(np.shape(d), dtype=np.int64)
    for t in T:
        k += d >= t
    return k


def _applies(mode, v):
    return np.where(v == 0, mode & 1, mode & 2) != 0


def apply_columns(v, depth, H, p):
    """v: (sx, 2^depth, sz) values of the map's columns, indexed [i, y, k].  The per-cell contract's result for them."""
    h, _, _, below, above, T, colours = check(H, (0, 0), depth, p)
    v = np.asarray(v).astype(np.int64)
    assert v.shape == (h.shape[0], 1 << depth, h.shape[1])
    y = np.arange(1 << depth, dtype=np.int64)[None, :, None]
    hh = h[:, None, :]
    under = y < hh
    layer = colours[_band(np.maximum(hh - 1 - y, 0), T)]
    return np.where(under & _applies(below, v), layer, np.where(~under & _applies(above, v), p["above_colour"], v)).astype(np.uint32)


def apply_cells(grid, depth, H, origin, p):
    """grid: (2^depth,)*3 values as svo_nodes_sample gives them, indexed [x, y, z].  The per-cell contract's result."""
    h, ox, oz = check(H, origin, depth, p)[:3]
    out = np.array(grid, dtype=np.uint32)
    assert out.shape == (1 << depth,) * 3
    out[ox:ox + h.shape[0], :, oz:oz + h.shape[1]] = apply_columns(out[ox:ox + h.shape[0], :, oz:oz + h.shape[1]], depth, H, p)
    return out


def _starts(o, n, s):
    """the tiles of 2^s columns that [o, o + n) meets: (the first tile, their count, each one's first column minus o)"""
    t0, t1 = o >> s, (o + n - 1) >> s
    first = np.maximum(np.arange(t0, t1 + 1, dtype=np.int64) << s, o) - o
    return t0, t1 - t0 + 1, first


def _pyramid(h, ox, oz, s):
    x0, nx, fx = _starts(ox, h.shape[0], s)
    z0, nz, fz = _starts(oz, h.shape[1], s)
    lo = np.minimum.reduceat(np.minimum.reduceat(h, fx, axis=0), fz, axis=1)
    hi = np.maximum.reduceat(np.maximum.reduceat(h, fx, axis=0), fz, axis=1)
    return x0, z0, lo, hi


def pyramid(H, origin, depth, s):
    """level s (0: the clamped map itself) as uint32 [nx, nz, 2] of (min, max), the tile (origin >> s) + (i, k) at [i, k]"""
    h, ox, oz = check(H, origin, depth, params())[:3]
    if not 0 <= s <= depth:
        raise ValueError(f"s must be 0..{depth} (got {s})")
    _, _, lo, hi = _pyramid(h, ox, oz, s)
    return np.stack([lo, hi], axis=-1).astype(np.uint32)


def edit(words, n_words, H, origin, depth, p):
    """-> (the new words, uint32, of the new length; the tallies as a dict).  Raises Refused and writes nothing."""
    check_length(words, n_words)
    h, ox, oz, below, above, T, colours = check(H, origin, depth, p)
    w = np.asarray(words, dtype=np.uint32)[:n_words].astype(np.int64)
    tally = dict.fromkeys(TALLIES, 0)
    writes, groups = [], []  # (addresses, words) per level; the new groups' first words in order
    if not h.size or not (below or above):
        return w.astype(np.uint32), tally
    sx, sz = h.shape
    above_colour = p["above_colour"]
    # the frontier: the word's address, its cell on the level's grid, and the word as it stands (a virtual child's too)
    at = np.arange(8, dtype=np.int64)
    cell = np.stack(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    word = w[:8].copy()
    kids = cell.copy()
    for level in range(1, depth + 1):
        if not at.size:
            break
        n, s = at.size, depth - level
        S = 1 << s
        x0, y0, z0 = (cell << s).T
        tx0, tz0, lo, hi = _pyramid(h, ox, oz, s)
        xi, zi = cell[:, 0] - tx0, cell[:, 2] - tz0
        meets = (xi >= 0) & (xi < lo.shape[0]) & (zi >= 0) & (zi < lo.shape[1])
        inside = (x0 >= ox) & (x0 + S <= ox + sx) & (z0 >= oz) & (z0 + S <= oz + sz)
        xi, zi = np.where(meets, xi, 0), np.where(meets, zi, 0)
        hmin, hmax = lo[xi, zi], hi[xi, zi]
        k_lo, k_hi = _band(np.maximum(hmin - y0 - S, 0), T), _band(np.maximum(hmax - 1 - y0, 0), T)
        cand_above = meets & (y0 + S > hmin) & (above != 0)
        cand_below = meets & (y0 < hmax) & (below != 0)
        all_above = meets & (y0 >= hmax)
        all_below = meets & (y0 + S <= hmin) & (k_lo == k_hi)
        touched = cand_above | cand_below
        uniform = touched & inside & (all_above | all_below)
        mode = np.where(all_above, above, below)
        colour = np.where(all_above, above_colour, colours[k_lo])
        ptr = word >> 4
        leaf = ptr >= VOXEL_OFFSET
        v0 = np.where(leaf, ptr - VOXEL_OFFSET, 0)
        over = uniform & leaf & _applies(mode, v0) & (colour != v0)
        collapse = uniform & ~leaf & (mode == MODE_SET)
        changes = cand_above & _applies(above, v0) & (above_colour != v0)
        for k in range(len(colours)):
            changes |= cand_below & _applies(below, v0) & (k_lo <= k) & (k <= k_hi) & (colours[k] != v0)
        split = touched & ~uniform & leaf & changes
        opened = touched & ~leaf & ~collapse
        if level == depth and opened.any():
            raise Refused(cell[int(np.flatnonzero(opened)[0])])
        assert not (split & (level == depth)).any(), "nothing is mixed at the last level"
        new_group = n_words + 8 * (len(groups) + np.cumsum(split) - 1)
        out = np.where(split, new_group << 4, (VOXEL_OFFSET + colour) << 4)
        wr = split | collapse | over
        writes.append((at[wr], out[wr]))
        groups += [(int(g), int(x) & ~15) for g, x in zip(new_group[split], word[split])]
        tally["splits"] += int(split.sum())
        tally["collapses"] += int(collapse.sum())
        tally["overwrites"] += int(over.sum())
        tally["opened"] += int(opened.sum())
        tally["untouched"] += int(n - wr.sum() - opened.sum())
        tally.setdefault("level_splits", []).append(int(split.sum()))
        # the next frontier
        go = np.flatnonzero(split | opened)
        base = np.where(split, new_group, ptr)[go]
        real = opened[go]
        if ((base[real] % 8 != 0) | (base[real] + 8 > n_words)).any():
            raise ValueError("malformed tree: an interior pointer is unaligned or leaves the words")
        at = (base[:, None] + np.arange(8)[None, :]).reshape(-1)
        cell = (cell[go][:, None, :] * 2 + kids[None, :, :]).reshape(-1, 3)
        word = np.where(real[:, None], w[np.where(real, base, 0)[:, None] + np.arange(8)[None, :]], (word[go] & ~15)[:, None]).reshape(-1)
    result = np.concatenate([w, np.zeros(8 * len(groups), dtype=np.int64)])
    for g, leaf_word in groups:
        result[g:g + 8] = leaf_word
    for a, x in writes:
        result[a] = x
    return result.astype(np.uint32), tally


def terrain(sx, sz, lo=20, hi=90, seed=32):
    """h = lo + f (hi - lo) + (0 or 1 at random), f two sines normalised to [0, 1]: int64 [sx, sz]"""
    x, z = np.arange(sx, dtype=np.float64)[:, None], np.arange(sz, dtype=np.float64)[None, :]
    f = np.sin(x * 0.11 + 0.5) * np.cos(z * 0.07) + 0.5 * np.sin((x + 2.0 * z) * 0.045 + 1.0)
    f = (f - f.min()) / max(f.max() - f.min(), 1e-9)
    return (lo + f * (hi - lo)).astype(np.int64) + np.random.default_rng(seed).integers(0, 2, (sx, sz))


def table_cases():
    """{name: (base, H, origin, params)} at depth 7; base "base7" is tests/pass_frame.py's tree7_base, "root" the empty
    root group"""
    whole = terrain(128, 128)
    rng = np.random.default_rng(7)
    eight = [(2, GRASS), (1, 0), (0, 0xFF00FF), (3, DIRT), (4, 0), (2, 0x112233), (5, STONE), (9, 0x445566)]
    return {
        "terraform": ("base7", whole, (0, 0), params(TERRAIN, "set", "set", 0)),
        "raise only": ("base7", whole, (0, 0), params(TERRAIN, "empty", None)),
        "lower only": ("base7", whole, (0, 0), params(TERRAIN, None, "set", 0)),
        "repaint": ("base7", whole, (0, 0), params(TERRAIN, "voxels", None)),
        "rectangle": ("base7", rng.integers(0, 141, (67, 50)), (5, 9), params(TERRAIN, "set", "set", 0)),
        "one column": ("base7", np.array([[77]]), (127, 0), params(TERRAIN, "set", "set", 0)),
        "row": ("base7", terrain(1, 128, 10, 100), (64, 0), params(TERRAIN, "set", "voxels", 0x00C0FF)),
        "empty root": ("root", whole, (0, 0), params(TERRAIN)),
        "flat": ("root", np.full((128, 128), 64), (0, 0), params()),
        "eight layers": ("base7", whole, (0, 0), params(eight, "set", "set", 0)),
    }
