"""Sampling a tree in the node buffer (csrc/svo_sample.hip), CPU side: the entry points are exported with
signatures and declared in the header, SampleParams has the header's layout; the rule for one cell (tests/sample_ref.py:
sample) gives the index and level of the host model's find_voxel on built, edited and mixed-level trees, on the tree's own
grid and on coarser ones; the dense kernel's formulation (sample_bricks) equals the rule on aligned and unaligned boxes at
every depth that takes another path; malformed trees terminate and report the broken pointer's word."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import build_ref as B
import edit_ref as E
import list_ref as L
import sample_ref as S
from conftest import ROOT as REPO
from test_compact_host import base6_voxels, malformed_cases
from test_edit_gpu import edit_voxels
from test_list_host import full_root, mixed_levels, one_leaf_root

NEW = ("svo_nodes_sample", "svo_nodes_sample_dense", "svo_sample_timing")
TOP = (1 << 21) - 1
DEEP_CELL = [TOP - 1, 5, 1234567]  # a depth-21 voxel next to the grid's far x face: all six face neighbours are inside
# (origin, size): aligned, unaligned, one cell, across a brick corner
BOXES = {"aligned": ((4, 8, 0), (8, 4, 12)), "unaligned": ((1, 2, 3), (5, 1, 9)), "one cell": ((6, 1, 5), (1, 1, 1)),
         "brick corner": ((3, 3, 3), (2, 2, 2))}


def deep_cells():
    """the depth-21 voxel, its six face neighbours (all inside the grid, one on its far face), and two cells outside it"""
    c = np.array(DEEP_CELL, dtype=np.int64)
    near = [c + d for axis in range(3) for d in (np.eye(3, dtype=np.int64)[axis], -np.eye(3, dtype=np.int64)[axis])]
    inside = [p for p in near if (p >= 0).all() and (p <= TOP).all()]
    return np.array([c] + inside + [[1 << 21, 5, 7], [0xFFFFFFFF] * 3], dtype=np.int64)


def fitted(box, depth):
    """the box cut to the depth grid: its origin moved inside, its size cut at the far faces"""
    side = 1 << depth
    origin = tuple(min(o, side - 1) for o in box[0])
    return origin, tuple(min(s, side - o) for o, s in zip(origin, box[1]))


@pytest.fixture(scope="module")
def trees():
    """{name: (words, depth)}: base6, base6 edited with 4 097 voxels in put order, the mixed-level tree"""
    a = base6_voxels()
    b = edit_voxels(np.random.default_rng(4097), 6, 4097, a[0], 0)
    base = B.build(a[0], 6, a[1])
    return {"base6": (base, 6), "edited": (E.edit(base, base.size, b[0], 6, b[1]), 6), "mixed levels": (mixed_levels(), 6)}


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_sample.argtypes) == 7 and len(lib.svo_nodes_sample_dense.argtypes) == 5
    assert len(lib.svo_sample_timing.argtypes) == 2
    assert callable(pkg.Render.sample_voxels) and callable(pkg.Render.sample_dense) and callable(pkg.Gpu.sample_timing)
    assert (pkg.SAMPLE_FINER, pkg.SAMPLE_OUTSIDE, pkg.SAMPLE_BROKEN) == (S.FINER, S.OUTSIDE, S.BROKEN) == (1 << 28, 1 << 29, 1 << 30)


def test_sample_params_have_the_headers_layout(pkg):
    P = pkg._lib.SampleParams
    assert C.sizeof(P) == 16
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [("flags", 0, 4), ("depth", 4, 4), ("n_words", 8, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_sample_params \{(.*?)\} svo_sample_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [("uint32_t", "flags"), ("uint32_t", "depth"), ("uint64_t", "n_words")]


def test_the_header_declares_the_functions_and_the_marks():
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    assert "the tree in the node buffer sampled on the device (DESIGN.md 19)" in header
    assert re.search(r"int svo_nodes_sample\(svo_ctx \*ctx, const svo_sample_params \*p, const uint32_t \*xyz_dev, size_t n,\s*"
                     r"uint32_t \*value_out_dev, uint32_t \*level_out_dev[^,]*, uint32_t \*index_out_dev[^,)]*\);", header)
    assert re.search(r"int svo_nodes_sample_dense\(svo_ctx \*ctx, const svo_sample_params \*p, const uint32_t origin\[3\], "
                     r"const uint32_t size\[3\],\s*uint32_t \*grid_out_dev\);", header)
    assert re.search(r"#define SVO_SAMPLE_TIMES 2\b[^\n]*\nint svo_sample_timing\(svo_ctx \*ctx, float ms_out\[SVO_SAMPLE_TIMES\]\);", header)
    for name, bit in (("FINER", 28), ("OUTSIDE", 29), ("BROKEN", 30)):
        assert re.search(rf"#define SVO_SAMPLE_{name}\s+\(1u << {bit}\)", header)


def assert_host_model_agrees(pkg, words, cells, depth, got, what):
    """find_voxel at the cell's centre, stopped at `depth`, ends on the word and level that sample reports"""
    octree = pkg.Octree.from_words(words)
    scale = 2.0 / (1 << depth)  # (centres and the walk's midpoints are exact in f32 up to depth 21)
    for cell, level, index in zip(cells, got[1], got[2]):
        found, found_level, _ = octree.find_voxel(((cell + 0.5) * scale - 1.0).tolist(), max_depth=depth)
        assert (found, found_level) == (int(index), int(level)), f"{what}: cell {cell}: host {(found, found_level)}, sample {(index, level)}"


def test_the_rule_agrees_with_the_host_model(pkg, trees):
    rng = np.random.default_rng(19)
    for name, (words, depth) in trees.items():
        xyz, value, level = L.list_voxels(words, words.size, depth)
        for d in (depth, depth - 1, depth - 2):
            cells = np.concatenate([xyz.astype(np.int64) >> (depth - d), rng.integers(0, 1 << d, (5000, 3))])
            got = S.sample(words, words.size, cells, d)
            assert all(a.dtype == np.uint32 and a.shape == (len(cells),) for a in got)
            assert_host_model_agrees(pkg, words, cells, d, got, f"{name} on the depth-{d} grid")
            # a value is the word's, a mark says why there is none; the level never passes the grid's depth
            at = words[got[2]] >> 4
            leaf = at >= B.VOXEL_OFFSET
            assert np.array_equal(got[0][leaf], (at[leaf] - B.VOXEL_OFFSET).astype(np.uint32))
            assert (got[0][~leaf] == S.FINER).all() and (got[1][~leaf] == d).all() and (got[1] >= 1).all() and (got[1] <= d).all()
            if d == depth:  # every listed voxel samples to its colour at its level
                n = len(xyz)
                assert np.array_equal(got[0][:n], value) and np.array_equal(got[1][:n], level)
            else:
                assert (got[0] == S.FINER).any(), f"{name}: no FINER on the depth-{d} grid"
    # counters never matter
    words = trees["edited"][0]
    counted = words | rng.integers(0, 16, words.size).astype(np.uint32)
    cells = rng.integers(0, 64, (5000, 3))
    assert all(np.array_equal(a, b) for a, b in zip(S.sample(counted, words.size, cells, 6), S.sample(words, words.size, cells, 6)))


def test_the_depth_21_voxel_and_the_cells_outside(pkg):
    words = B.build([DEEP_CELL], 21, [0x00FF00])
    cells = deep_cells()
    value, level, index = S.sample(words, words.size, cells, 21)
    assert value[0] == 0x00FF00 and level[0] == 21 and index[0] == words.size - 8 + (0 * 4 + 1 * 2 + 1)
    inside = len(cells) - 2
    assert inside == 7 and (value[1:inside] == 0).all() and (level[1:inside] >= 1).all()
    assert (value[inside:] == S.OUTSIDE).all() and (level[inside:] == 0).all() and (index[inside:] == S.NO_INDEX).all()
    assert_host_model_agrees(pkg, words, cells[:inside], 21, (value, level, index), "depth 21")
    # one coordinate outside is enough, on any axis; 2^depth - 1 is inside
    for axis in range(3):
        cell = [0, 0, 0]
        cell[axis] = 1 << 5
        assert S.sample(full_root(), 8, [cell], 5)[0][0] == S.OUTSIDE
        cell[axis] = (1 << 5) - 1
        assert S.sample(full_root(), 8, [cell], 5)[0][0] == (full_root()[4 >> axis] >> 4) - B.VOXEL_OFFSET
    # a leaf above the grid's depth covers its cells
    value, level, index = S.sample(one_leaf_root(), 8, [[255, 0, 128], [127, 0, 128]], 8)
    assert value.tolist() == [0xABCDEF, 0] and level.tolist() == [1, 1] and index.tolist() == [5, 1]


def assert_bricks_equal_the_rule(words, depth, box, what):
    origin, size = box
    want = S.sample_dense(words, words.size, origin, size, depth)
    got = S.sample_bricks(words, words.size, origin, size, depth)
    assert got.dtype == np.uint32 and got.shape == tuple(size) == want.shape, what
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} cells differ"
    return want


def test_bricks_equal_the_rule(trees):
    rng = np.random.default_rng(7)
    # the trees on their own grid, which has a common path of four levels, and on the grids of depth 1, 2 and 3, which
    # have none, none and one
    for name, (words, depth) in trees.items():
        for d in (1, 2, 3, 6):
            side = 1 << d
            assert_bricks_equal_the_rule(words, d, ((0, 0, 0), (side,) * 3), f"{name}, the depth-{d} grid")
            for box_name, box in BOXES.items():
                assert_bricks_equal_the_rule(words, d, fitted(box, d), f"{name}, depth {d}, {box_name}")
    # trees built at the depths 1, 2 and 3: values instead of FINER
    for d in (1, 2, 3):
        side = 1 << d
        words = B.build(rng.integers(0, side, (side * side, 3)), d, rng.integers(1, 1 << 24, side * side))
        whole = assert_bricks_equal_the_rule(words, d, ((0, 0, 0), (side,) * 3), f"built at depth {d}")
        assert (whole != 0).any() and (whole < S.FINER).all()
        for box_name, box in BOXES.items():
            assert_bricks_equal_the_rule(words, d, fitted(box, d), f"built at depth {d}, {box_name}")
    # mixed levels below and above the tree's depth: bricks under coarse leaves, leaves above the grid, FINER
    mixed = trees["mixed levels"][0]
    fine = assert_bricks_equal_the_rule(mixed, 8, ((37, 50, 61), (70, 33, 67)), "mixed levels on the depth-8 grid")
    assert (fine != 0).any() and (fine < S.FINER).all()
    coarse = assert_bricks_equal_the_rule(mixed, 4, ((0, 0, 0), (16, 16, 16)), "mixed levels on the depth-4 grid")
    assert (coarse == S.FINER).any() and ((coarse != 0) & (coarse < S.FINER)).any()
    for box_name, box in BOXES.items():
        assert_bricks_equal_the_rule(mixed, 4, fitted(box, 4), f"mixed levels, depth 4, {box_name}")
    # a size with a 0 has no cells
    assert S.sample_bricks(mixed, mixed.size, (1, 2, 3), (4, 0, 4), 6).shape == (4, 0, 4)


def test_malformed_trees_terminate_and_report_the_pointer():
    cases = malformed_cases()
    whole5 = S.box_cells((0, 0, 0), (32, 32, 32))
    chain = np.array([[TOP, 0, TOP], [TOP, 0, TOP - 1], [0, 0, 0]])  # the 32-level chain goes down child 5
    for name, words in cases.items():
        ptr = words.astype(np.int64) >> 4
        bad = np.flatnonzero((ptr < B.VOXEL_OFFSET) & ((ptr % 8 != 0) | (ptr + 8 > words.size)))
        for depth, cells in ((4, whole5 >> 1), (5, whole5), (21, np.concatenate([whole5 << 16, chain]))):
            value, level, index = S.sample(words, words.size, cells, depth)  # (asserts that no word outside is read)
            assert (level <= depth).all() and (index < words.size).all()
            broken = value == S.BROKEN
            assert set(index[broken].tolist()) <= set(bad.tolist()), name
            if depth > 4 and name in ("a pointer with pointer + 8 > n_words", "an unaligned pointer"):
                assert bad.size == 1 and broken.any() and (index[broken] == bad[0]).all(), name
            if depth == 5:
                side = 1 << depth
                assert np.array_equal(S.sample_bricks(words, words.size, (0, 0, 0), (side,) * 3, depth),
                                      value.reshape((side,) * 3)), name
    # the chain has an interior word at every level: its cell is FINER at level 21
    value, level, index = S.sample(cases["32 levels"], 8 * 32, chain, 21)
    assert value.tolist() == [S.FINER, 0, 0] and level.tolist() == [21, 21, 1] and index.tolist() == [20 * 8 + 5, 20 * 8 + 4, 0]
    # the cycle through the root is walked `depth` times at the most
    value, level, index = S.sample(cases["a cycle through the root"], cases["a cycle through the root"].size, whole5 << 16, 21)
    assert (level <= 21).all()


def test_what_the_reference_refuses(trees):
    words = trees["base6"][0]
    for depth in (0, 22):
        with pytest.raises(ValueError):
            S.sample(words, words.size, [[0, 0, 0]], depth)
        with pytest.raises(ValueError):
            S.sample_bricks(words, words.size, (0, 0, 0), (1, 1, 1), depth)
    for n in (0, 12, words.size + 8):
        with pytest.raises(ValueError):
            S.sample(words, n, [[0, 0, 0]], 6)
    for f in (S.sample_dense, S.sample_bricks):
        with pytest.raises(ValueError):
            f(words, words.size, (60, 0, 0), (5, 1, 1), 6)
        with pytest.raises(ValueError):
            f(words, words.size, (0, 0, 0), (2048, 1024, 1024), 21)
    assert S.sample(words, words.size, np.zeros((0, 3), dtype=np.int64), 6)[0].shape == (0,)
