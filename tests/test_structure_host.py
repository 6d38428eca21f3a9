"""Structures scattered over a tree (csrc/svo_structure.hip), CPU side: the entry points are exported with
signatures and the params have the header's layouts; the skipping walk of the column tops (tests/structure_ref.py:
column_tops_skipping, the kernel's formulation) equals the literal rule (column_tops: sample_ref.sample down each column)
on the smallest trees at which it can go wrong; the host loader equals the restatement of the reference's position rule
on both of its structure models; the restatements of the sites and of the stamp equal brute-force loops."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import build_ref as B
import compact_ref as K
import sample_ref as S
import structure_ref as R
from conftest import GOLDEN
from pass_frame import tree7_base
from test_compact_host import malformed_cases
from test_list_host import EMPTY_ROOT, full_root, mixed_levels, one_leaf_root

NEW = ("svo_nodes_column_tops", "svo_structures_sites", "svo_structures_stamp", "svo_structure_timing")
DEEP = ((1 << 21) - 3, 1234567, 5)  # the one voxel of the depth-21 tree
ODD_RECT = ((3, 5), (9, 70))        # aligned to nothing
ISLAND_SITES, ISLAND_EMPTY, ISLAND_VOXELS = 163, 5095, 33867


def structure_models():
    """{name: (size, xyzi, palette)} of the reference's two structure models (tests/golden/structures_vox.npz)"""
    z = np.load(os.path.join(GOLDEN, "structures_vox.npz"))
    return {name: (tuple(int(v) for v in z[name + "_size"]), z[name + "_xyzi"], z[name + "_palette"]) for name in ("tree", "crystal")}


@functools.lru_cache(maxsize=None)
def tree_structure():
    """tree.vox by the restatement: (offsets, index, colours)"""
    return R.load_structure(*structure_models()["tree"])


@functools.lru_cache(maxsize=None)
def island():
    """the depth-7 heightfield of the end-to-end tests: h = floor(20 + 10 sin(x / 9) + 8 cos(z / 13)), the cells h - 2 .. h of
    every column within 60 cells of (64, 64), coloured by position: (coords, colours, canonical words, h, mask)"""
    x, z = np.meshgrid(np.arange(128), np.arange(128), indexing="ij")
    mask = (x - 64) ** 2 + (z - 64) ** 2 <= 60 * 60
    h = np.floor(20 + 10 * np.sin(x / 9) + 8 * np.cos(z / 13)).astype(np.int64)
    coords = np.concatenate([np.stack([x[mask], h[mask] - k, z[mask]], axis=1) for k in (2, 1, 0)])
    colours = 0x204020 + coords[:, 0] * 0x10000 + coords[:, 1] * 0x100 + coords[:, 2]
    return coords, colours, B.build(coords, 7, colours), h, mask


@functools.lru_cache(maxsize=None)
def tree7_tops():
    """pass_frame.tree7_base's edited words and the literal rule over every column of its 128 x 128 grid"""
    words = tree7_base()["words"]
    return words, R.column_tops(words, words.size, (0, 0), (128, 128), 7)


def small_trees():
    """{name: (words, depth)}: random builds at the depths 1, 2 and 3"""
    rng = np.random.default_rng(22)
    out = {}
    for depth, n in ((1, 3), (2, 9), (3, 40)):
        out[f"depth {depth}"] = (B.build(rng.integers(0, 1 << depth, (n, 3)), depth, rng.integers(1, 1 << 24, n)), depth)
    return out


def assert_tops(got, want, what):
    for g, w, name in zip(got, want, ("top", "value")):
        assert g.dtype == np.uint32 and g.shape == w.shape, f"{what}: {name}"
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: {len(bad)} columns differ in {name}, first at {bad[:3].tolist()}: got {g[g != w][:3]} want {w[g != w][:3]}"


def both(words, origin, size, depth, what, y_lo=0, y_hi=None):
    want = R.column_tops(words, words.size, origin, size, depth, y_lo, y_hi)
    assert_tops(R.column_tops_skipping(words, words.size, origin, size, depth, y_lo, y_hi), want, what)
    return want


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert [len(getattr(lib, name).argtypes) for name in NEW] == [6, 9, 12, 2]
    assert "svo_structure_load" in pkg._lib.HOST_SYMBOLS and "svo_vox_write_box" in pkg._lib.HOST_SYMBOLS
    for name in ("column_tops", "structure_sites", "stamp_structures", "place_structures", "scatter_structures"):
        assert callable(getattr(pkg.Render, name)), name
    assert callable(pkg.Gpu.structure_timing) and callable(pkg.load_structure) and callable(pkg.Structure.from_vox_bytes)


def test_params_have_the_headers_layouts(pkg):
    def layout(P):
        return C.sizeof(P), [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_]
    assert layout(pkg._lib.TopsParams) == (24, [("flags", 0, 4), ("depth", 4, 4), ("n_words", 8, 8), ("y_lo", 16, 4), ("y_hi", 20, 4)])
    assert layout(pkg._lib.SitesParams) == (32, [("flags", 0, 4), ("seed", 4, 4), ("one_in", 8, 4), ("on_value", 12, 4), ("lift", 16, 4),
                                                 ("reserved", 20, 4), ("max_sites", 24, 8)])
    assert layout(pkg._lib.StampParams) == (16, [("flags", 0, 4), ("depth", 4, 4), ("max_voxels", 8, 8)])
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "svo_hip.h")).read()
    for text in ("#define SVO_TOP_NONE 0xFFFFFFFFu", "#define SVO_SITES_ROTATE 1u", "#define SVO_STRUCTURE_TIMES 3"):
        assert text in header
    assert pkg.render.TOP_NONE == -1 and np.uint32(R.TOP_NONE).view(np.int32) == -1


def test_skipping_walk_equals_the_rule_on_small_and_special_trees():
    for name, (words, depth) in small_trees().items():
        side = 1 << depth
        top, value = both(words, (0, 0), (side, side), depth, name)
        assert (top != R.TOP_NONE).any() and ((top == R.TOP_NONE) == (value == 0)).all(), name
    # the empty tree: nothing anywhere, at any depth
    for depth in (1, 5, 21):
        top, value = both(EMPTY_ROOT, ((1 << depth) - 2, 0), (2, 2), depth, f"empty, depth {depth}", y_lo=max(0, (1 << depth) - 4000))
        assert (top == R.TOP_NONE).all() and (value == 0).all()
    assert (R.column_tops_skipping(EMPTY_ROOT, 8, (0, 0), (4, 4), 21)[0] == R.TOP_NONE).all()
    # eight level-1 leaves: the top is the grid's, the value the upper octant's
    full = full_root()
    top, value = both(full, (0, 0), (16, 16), 4, "full root")
    assert (top == 15).all() and set(value.reshape(-1).tolist()) == {k * 0x010203 for k in (3, 4, 7, 8)}
    # one level-1 leaf (child 5 = x 1, y 0, z 1): its columns top out at the octant's highest cell
    one = one_leaf_root()
    top, value = both(one, (0, 0), (16, 16), 4, "one leaf")
    assert (top[8:, 8:] == 7).all() and (value[8:, 8:] == 0xABCDEF).all() and (np.delete(top.reshape(-1), np.flatnonzero(top.reshape(-1) == 7)) == R.TOP_NONE).all()


def test_y_range_cuts_a_coarse_leaf():
    # a level-2 leaf of the depth-5 grid covers 8 cells of a column: y in [8, 16) under child (1, 1, 0) of child (0, 0, 1)
    words = B.build([[0, 1, 2]], 2, [0x445566])  # the cell (0, 1, 2) of the depth-2 grid: x 0..7, y 8..15, z 16..23 at depth 5
    whole = both(words, (0, 16), (8, 8), 5, "whole height")
    assert (whole[0] == 15).all() and (whole[1] == 0x445566).all()
    for y_lo, y_hi, want in ((0, 12, 11), (0, 9, 8), (0, 8, R.TOP_NONE), (15, 32, 15), (16, 32, R.TOP_NONE), (10, 13, 12), (8, 16, 15)):
        top, value = both(words, (0, 16), (8, 8), 5, f"y in [{y_lo}, {y_hi})", y_lo, y_hi)
        assert (top == want).all() and (value == (0x445566 if want != R.TOP_NONE else 0)).all(), (y_lo, y_hi)
    # next to it nothing
    assert (both(words, (8, 16), (3, 8), 5, "beside the leaf")[0] == R.TOP_NONE).all()


def test_one_deep_column_at_depth_21():
    words = B.build([DEEP], 21, [0x00FF00])
    top, value = R.column_tops_skipping(words, words.size, (DEEP[0] - 1, DEEP[2] - 1), (3, 3), 21)
    assert top[1, 1] == DEEP[1] and value[1, 1] == 0x00FF00 and (np.delete(top.reshape(-1), 4) == R.TOP_NONE).all()
    # the literal rule over a window of the height that holds the voxel, and over windows that do not
    for y_lo, y_hi in ((DEEP[1] - 2000, DEEP[1] + 2000), (DEEP[1] + 1, DEEP[1] + 3000), (DEEP[1] - 3000, DEEP[1]), (DEEP[1], DEEP[1] + 1)):
        top, _ = both(words, (DEEP[0] - 1, DEEP[2] - 1), (3, 3), 21, f"depth 21, y in [{y_lo}, {y_hi})", y_lo, y_hi)
        assert (top[1, 1] == DEEP[1]) == (y_lo <= DEEP[1] < y_hi)


def test_mixed_levels_finer_and_counters():
    mixed = mixed_levels()
    top, value = both(mixed, (0, 0), (64, 64), 6, "mixed levels, depth 6")
    assert (value < S.FINER).all() and (top != R.TOP_NONE).any()
    # leaves above the grid, an odd rectangle of the depth-8 grid
    both(mixed, (37, 61), (100, 77), 8, "mixed levels, depth 8", 30, 201)
    # the tree refined below the grid: FINER counts as occupied and is said so
    top, value = both(mixed, (0, 0), (16, 16), 4, "mixed levels, depth 4")
    assert (value == S.FINER).any() and ((value != 0) & (value < S.FINER)).any()
    # a depth-7 tree asked at depth 5
    words = tree7_base()["words"]
    top, value = both(words, (0, 0), (32, 32), 5, "tree7 at depth 5")
    assert (value == S.FINER).sum() > 100 and ((top == R.TOP_NONE) == (value == 0)).all()
    # random counter bits in every word: the same arrays
    counted = mixed | np.random.default_rng(6).integers(0, 16, mixed.size).astype(np.uint32)
    assert_tops(R.column_tops_skipping(counted, counted.size, (0, 0), (64, 64), 6), R.column_tops(mixed, mixed.size, (0, 0), (64, 64), 6), "counters")


def test_edited_tree_and_its_layouts():
    words, want = tree7_tops()
    assert_tops(R.column_tops_skipping(words, words.size, (0, 0), (128, 128), 7), want, "tree7, put order")
    assert (want[0] != R.TOP_NONE).sum() > 5000
    origin, size = ODD_RECT
    got = both(words, origin, size, 7, "tree7, a rectangle aligned to nothing")
    window = tuple(slice(o, o + s) for o, s in zip(origin, size))
    assert np.array_equal(got[0], want[0][window]) and np.array_equal(got[1], want[1][window])
    plain = K.compact(words, words.size, False)[0]
    assert_tops(R.column_tops_skipping(plain, plain.size, (0, 0), (128, 128), 7), want, "tree7, compacted")
    pruned = K.compact(words, words.size, True)[0]
    assert pruned.size < plain.size
    assert_tops(R.column_tops_skipping(pruned, pruned.size, (0, 0), (128, 128), 7), want, "tree7, pruned")
    # a size with a 0: no columns
    for size in ((0, 5), (5, 0), (0, 0)):
        for f in (R.column_tops, R.column_tops_skipping):
            assert f(words, words.size, (1, 2), size, 7)[0].shape == size


def test_malformed_trees_give_broken_and_read_nothing_outside():
    broken = 0
    for name, words in malformed_cases().items():
        # both forms assert that no word outside the tree is read, and both end on every tree
        top, value = both(words, (0, 0), (32, 32), 5, f"{name}, depth 5")
        broken += int((value == S.BROKEN).any())
        both(words, (5 << 16, 9 << 16), (4, 6), 21, f"{name}, depth 21", (3 << 16) - 100, (3 << 16) + 100)
    assert broken == 2  # the two pointer cases


def test_refusals_of_the_restatement():
    words = EMPTY_ROOT
    for f in (R.column_tops, R.column_tops_skipping):
        for args in (((0, 0), (1, 1), 0), ((0, 0), (1, 1), 22), ((120, 0), (9, 1), 7), ((0, 128), (1, 1), 7)):
            with pytest.raises(ValueError):
                f(words, 8, *args)
        for y in ((5, 5), (6, 5), (0, 129)):
            with pytest.raises(ValueError):
                f(words, 8, (0, 0), (1, 1), 7, *y)
        with pytest.raises(ValueError):
            f(words, 12, (0, 0), (1, 1), 7)


@pytest.mark.parametrize("name, voxels", [("tree", 187), ("crystal", 2739)])
def test_host_loader_equals_the_restatement(pkg, tmp_path, name, voxels):
    size, xyzi, palette = structure_models()[name]
    assert len(xyzi) == voxels and len(set(size)) == 3  # no cube
    blob = pkg.cpu_octree.vox_write(size, xyzi, palette)
    assert pkg.cpu_octree.vox_parse(blob)[0] == size
    want = R.load_structure(size, xyzi, palette)
    path = tmp_path / f"{name}.vox"
    path.write_bytes(blob)
    for got in (pkg.Structure.from_vox_bytes(blob), pkg.load_structure(path)):
        assert len(got) == voxels
        for g, w, what in zip((got.offsets, got.index, got.colours), want, ("offsets", "index", "colours")):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what
    # the model stands on y = 0 and is centred on x and z, as the reference places it
    offsets = want[0]
    assert offsets[:, 1].min() == 0 and offsets[:, 0].max() <= size[0] // 2 and offsets[:, 2].min() >= -(size[1] // 2)
    assert (want[1] >= 1).all() and (want[2] < 1 << 24).all() and (want[2] != 0).any()
    # a scalar size still means a cube
    assert pkg.cpu_octree.vox_parse(pkg.cpu_octree.vox_write(16, xyzi[:3], palette))[0] == (16, 16, 16)
    with pytest.raises(ValueError):
        pkg.Structure.from_vox_bytes(b"not a vox file at all")
    with pytest.raises(ValueError):
        pkg.load_structure(tmp_path / "missing.vox")


def test_signed_device_inputs_keep_negatives_and_stay_out_of_range(pkg):
    import torch
    cpu = torch.device("cpu")
    t = pkg._device.device_u32(np.array([[-5, 0, 1 << 22], [1 << 40, -(1 << 40), -1]]), cpu, signed=True)
    assert t.dtype == torch.int32 and t.tolist() == [[-5, 0, 1 << 22], [(1 << 31) - 1, -(1 << 31), -1]]
    same = torch.tensor([-7, 7], dtype=torch.int32)
    assert pkg._device.device_u32(same, cpu, signed=True) is same or pkg._device.device_u32(same, cpu, signed=True).tolist() == [-7, 7]
    s = pkg.Structure([[1, -2, 3]], [4], [0xFFFFFFFF])
    offsets, colours = s.on(cpu)
    assert offsets.tolist() == [[1, -2, 3]] and colours.tolist() == [-1] and s.on(cpu)[0] is offsets and len(s) == 1
    with pytest.raises(ValueError):
        pkg.Structure([[1, 2, 3]], [1, 2], [5])


def lowbias32_scalar(v):
    v &= 0xFFFFFFFF
    v ^= v >> 16
    v = v * 0x7feb352d & 0xFFFFFFFF
    v ^= v >> 15
    v = v * 0x846ca68b & 0xFFFFFFFF
    return v ^ v >> 16


def test_sites_against_a_loop():
    rng = np.random.default_rng(5)
    tops = rng.integers(0, 100, (23, 17)).astype(np.uint32)
    tops[rng.random((23, 17)) < 0.2] = R.TOP_NONE
    values = rng.integers(1, 4, (23, 17)).astype(np.uint32)
    values[rng.random((23, 17)) < 0.1] = S.FINER
    values[0, 0] = S.BROKEN
    origin = (1000, 7)
    for seed, one_in, on_value, lift, flags, with_values in ((0, 1, 0, 1, 1, True), (9, 3, 2, -4, 1, True), (0xFFFFFFF0, 2, 0, 0, 0, True),
                                                             (5, 2, 0, 1, 1, False)):
        want_o, want_r = [], []
        for i in range(23):
            for k in range(17):
                x, z, top, value = origin[0] + i, origin[1] + k, int(tops[i, k]), int(values[i, k])
                h = lowbias32_scalar(lowbias32_scalar(x + seed) ^ z)
                if top == R.TOP_NONE or h % one_in:
                    continue
                if with_values and (value >= 1 << 27 or (on_value and value != on_value)):
                    continue
                want_o.append((x, top + lift, z))
                want_r.append(lowbias32_scalar(h + 0x9E3779B9) >> 30 if flags else 0)
        got_o, got_r = R.sites(tops, values if with_values else None, origin, one_in, seed, on_value, lift, flags)
        assert got_o.dtype == np.int32 and got_r.dtype == np.uint32
        assert got_o.tolist() == [list(o) for o in want_o] and got_r.tolist() == want_r and len(want_o) > 10
    with pytest.raises(ValueError):
        R.sites(tops, None, origin, 2, on_value=3)
    with pytest.raises(ValueError):
        R.sites(tops, values, origin, 0)


def test_all_four_rotations_occur():
    tops = np.zeros((128, 128), dtype=np.uint32)
    origins, rots = R.sites(tops, None, (0, 0), 64, seed=5)
    assert np.bincount(rots, minlength=4).tolist() == [51, 71, 55, 62] and len(origins) == 239
    assert (R.sites(tops, None, (0, 0), 64, seed=5, flags=0)[1] == 0).all()


def test_island_counts():
    coords, colours, words, h, mask = island()
    assert len(coords) == ISLAND_VOXELS and int((~mask).sum()) == ISLAND_EMPTY
    top, value = both(words, (0, 0), (128, 128), 7, "island")
    assert np.array_equal(top[mask], h[mask]) and (top[~mask] == R.TOP_NONE).all()
    assert np.array_equal(value[mask], 0x204020 + np.argwhere(mask)[:, 0] * 0x10000 + h[mask] * 0x100 + np.argwhere(mask)[:, 1])
    origins, rots = R.sites(top, value, (0, 0), 64, seed=5)
    assert len(origins) == ISLAND_SITES and set(rots.tolist()) == {0, 1, 2, 3}


def test_stamp_against_a_loop():
    offsets, _, colours = tree_structure()
    rng = np.random.default_rng(12)
    origins = rng.integers(-6, 40, (40, 3))
    rots = rng.integers(0, 4, 40)
    depth = 5
    turn = {0: lambda d: (d[0], d[1], d[2]), 1: lambda d: (d[2], d[1], -d[0]), 2: lambda d: (-d[0], d[1], -d[2]), 3: lambda d: (-d[2], d[1], d[0])}
    want = []
    for p in range(40):
        for v in range(len(offsets)):
            d = turn[int(rots[p])](offsets[v].tolist())
            cell = [int(origins[p][a]) + d[a] for a in range(3)]
            if all(0 <= c < 32 for c in cell):
                want.append((*cell, int(colours[v]), p))
    xyz, colour, placement = R.stamp(offsets, colours, origins, rots, depth)
    got = np.concatenate([xyz, colour[:, None], placement[:, None]], axis=1)
    assert got.dtype == np.uint32 and got.tolist() == [list(w) for w in want] and 0 < len(want) < 40 * len(offsets)
    # no rotations given: all 0
    assert np.array_equal(R.stamp(offsets, colours, origins, None, depth)[0], R.stamp(offsets, colours, origins, np.zeros(40), depth)[0])
    # four quarter turns are none
    assert np.array_equal(R.rotate(offsets, 4), offsets) and not np.array_equal(R.rotate(offsets, 1), offsets)
    for bad in (dict(origins=[[0, 1 << 22, 0]]), dict(origins=[[0, 0, -(1 << 22) - 1]]), dict(rots=[4]), dict(offsets=[[0, -(1 << 22), 0]])):
        args = {"offsets": [[0, 0, 0]], "colours": [1], "origins": [[0, 0, 0]], "rots": [0], **bad}
        with pytest.raises(R.BadInput):
            R.stamp(args["offsets"], args["colours"], args["origins"], args["rots"], 5)
    assert len(R.stamp([[0, 0, 0]], [1], [[-(1 << 22), 0, 0]], [3], 5)[1]) == 0  # (in range, and clipped)
