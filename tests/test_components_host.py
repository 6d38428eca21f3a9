"""The connected components of a tree in the node buffer (csrc/svo_components.hip), CPU side: the entry points
are exported and ComponentsParams has the header's layout; the two restatements of tests/components_ref.py, the walk per
face with a union-find and scipy's labelling of the expanded grid, induce the same partition of the cells on every tree the
GPU tests use, with and without SAME_VALUE; labels are first entries and fixed points, ids ascend by first entry; the
percolation tree is no trivial input; drop_floating on a grid."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import build_ref as B
import components_ref as R
import simplify_ref as S
from conftest import ROOT as REPO
from pass_frame import tree7_base
from test_list_host import EMPTY_ROOT, full_root, mixed_levels
from test_surface_host import ball

NEW = ("svo_nodes_label_components", "svo_components_timing", "svo_nodes_scatter_device")


@pytest.fixture(autouse=True)
def the_pass_exists(pkg):
    """the restatements restate a pass of the library: without it every test here fails"""
    assert all(name in pkg._lib.DEVICE_SYMBOLS for name in NEW)


@functools.lru_cache(maxsize=None)
def percolation(one_colour=False):
    """a 32^3 grid filled at random with probability 0.31, built at depth 5, in three colours (or one)"""
    fill = np.random.default_rng(91).random((32, 32, 32)) < 0.31
    coords = np.argwhere(fill)
    colours = np.full(len(coords), 0x808080) if one_colour else 1 + (coords.sum(axis=1) % 3) * 0x010101
    return coords, colours, B.build(coords, 5, colours)


def checkerboard():
    """every second cell of the depth-4 grid: 2 048 voxels, no two of which share a face"""
    cells = np.argwhere(np.indices((16, 16, 16)).sum(axis=0) % 2 == 0)
    return B.build(cells, 4, 1 + (cells[:, 0] & 1))


def serpentine(n=32):
    """the 2 n^3 - 1 cells of an induced path: the lattice points at even coordinates visited boustrophedon and the cells
    between consecutive points"""
    points, back_j, back_k = [], False, False
    for i in range(n):
        for j in (range(n - 1, -1, -1) if back_j else range(n)):
            points += [(i, j, k) for k in (range(n - 1, -1, -1) if back_k else range(n))]
            back_k = not back_k
        back_j = not back_j
    p = 2 * np.array(points, dtype=np.int64)
    assert (np.abs(np.diff(p, axis=0)).sum(axis=1) == 2).all()
    cells = np.empty((2 * len(p) - 1, 3), dtype=np.int64)
    cells[0::2], cells[1::2] = p, (p[1:] + p[:-1]) // 2
    return cells


@functools.lru_cache(maxsize=None)
def path6():
    cells = serpentine()
    return B.build(cells, 6, 1 + (np.arange(len(cells)) % 5))


@functools.lru_cache(maxsize=None)
def merged(name):
    """(the one-coloured ball or percolation tree, its lossless merge, depth)"""
    if name == "ball":
        coords, depth = np.argwhere(ball(64, 20) != 0), 6
    else:
        coords, depth = percolation(True)[0], 5
    words = B.build(coords, depth, np.full(len(coords), 0x808080))
    return words, S.simplify(words, words.size)[0], depth


def pair21(axis, offset=0):
    """two voxels either side of the middle plane along `axis` at depth 21; offset: the second one moved that far along the
    next axis"""
    half = 1 << 20
    a, b = [5, 1234567, 777], [5, 1234567, 777]
    a[axis], b[axis] = half - 1, half
    b[(axis + 1) % 3] += offset
    return B.build([a, b], 21, [0x00FF00, 0x0000FF])


DENSE_TREES = ("empty root", "full root", "full root on the depth-3 grid", "mixed levels", "edited depth 7 with counters", "checkerboard",
               "percolation", "path", "merged ball", "merged percolation")


@functools.lru_cache(maxsize=None)
def dense_trees():
    """name -> (words, depth): the trees small enough to expand; nobody writes to the arrays"""
    counted = tree7_base()["words"]
    return {
        "empty root": (EMPTY_ROOT, 1), "full root": (full_root(), 1), "full root on the depth-3 grid": (full_root(), 3),
        "mixed levels": (mixed_levels(), 6), "edited depth 7 with counters": (counted | np.random.default_rng(6).integers(0, 16, counted.size).astype(np.uint32), 7),
        "checkerboard": (checkerboard(), 4), "percolation": (percolation()[2], 5), "path": (path6(), 6),
        "merged ball": (merged("ball")[1], 6), "merged percolation": (merged("percolation")[1], 5),
    }


def check_labelling(label, ids, n_components, what):
    n = label.size
    assert (label <= np.arange(n)).all(), f"{what}: a label behind its entry"
    assert np.array_equal(label[label], label), f"{what}: a label that is no fixed point"
    roots = np.flatnonzero(label == np.arange(n))
    assert roots.size == n_components and np.array_equal(ids[roots], np.arange(n_components)), f"{what}: ids do not ascend by first entry"
    assert np.array_equal(ids, ids[label]), f"{what}: an entry's id is not its root's"


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_label_components.argtypes) == 7 and len(lib.svo_components_timing.argtypes) == 3
    assert len(lib.svo_nodes_scatter_device.argtypes) == 6
    for method in ("label_components", "scatter_nodes_device", "drop_floating"):
        assert callable(getattr(pkg.Render, method))
    assert callable(pkg.Gpu.components_timing)


def test_components_params_have_the_headers_layout(pkg):
    P = pkg._lib.ComponentsParams
    assert C.sizeof(P) == 24
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("flags", 0, 4), ("depth", 4, 4), ("n_words", 8, 8), ("max_entries", 16, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_components_params \{(.*?)\} svo_components_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [("uint32_t", "flags"), ("uint32_t", "depth"), ("uint64_t", "n_words"),
                                                             ("uint64_t", "max_entries")]
    assert re.search(r"int svo_nodes_label_components\(svo_ctx \*ctx, const svo_components_params \*p, uint32_t \*label_out_dev,\s*"
                     r"uint32_t \*id_out_dev[^,]*, uint32_t \*index_out_dev[^,]*, uint64_t \*n_out,\s*uint64_t \*n_components_out\);", header)
    assert re.search(r"#define SVO_COMPONENTS_TIMES 6\nint svo_components_timing\(svo_ctx \*ctx, float ms_out\[SVO_COMPONENTS_TIMES\], "
                     r"uint32_t \*rounds_out[^,)]*\);", header)
    assert re.search(r"int svo_nodes_scatter_device\(svo_ctx \*ctx, const uint32_t \*index_dev, const uint32_t \*words_dev[^,]*, uint32_t fill,\s*"
                     r"size_t n, uint64_t n_words\);", header)
    assert re.search(rf"#define SVO_COMPONENTS_SAME_VALUE\s+{R.SAME_VALUE}u", header)
    assert "6-connectivity" in header


@pytest.mark.parametrize("name", DENSE_TREES)
def test_the_two_restatements_agree(name):
    assert set(dense_trees()) == set(DENSE_TREES)
    words, depth = dense_trees()[name]
    for same in (False, True):
        label, ids, n, index = R.labels(words, words.size, depth, same)
        check_labelling(label, ids, n, f"{name}, same_value {same}")
        assert np.array_equal((words[index] >> 4) > B.VOXEL_OFFSET, np.ones(label.size, dtype=bool))
        if same and np.unique(words[words >> 4 > B.VOXEL_OFFSET] >> 4).size > 100:
            continue  # (scipy labels per value: the trees of random colours are compared without the flag only)
        comp, entries = R.dense_labels(words, words.size, depth, same)
        held = entries >= 0
        assert held.sum() > 0 or label.size == 0
        assert R.same_partition(label[entries[held]], comp[held]), f"{name}, same_value {same}: the partitions differ"
        assert len(np.unique(comp[held])) == n


def test_the_percolation_tree_is_no_trivial_input():
    coords, colours, words = percolation()
    label, ids, n, _ = R.labels(words, words.size, 5)
    sizes = np.bincount(ids, minlength=n)
    assert (label.size, n, int((sizes >= 2).sum()), int(sizes.max())) == (10187, 1908, 717, 3093)
    assert n >= 1000 and (sizes >= 2).sum() >= 500 and sizes.max() >= 2000
    # per colour there are more components, none larger than before
    _, ids3, n3, _ = R.labels(words, words.size, 5, True)
    assert n3 > n and np.bincount(ids3).max() < sizes.max()


def test_small_cases_spelled_out():
    for depth in (1, 21):
        assert R.labels(EMPTY_ROOT, 8, depth)[2] == 0
        label, ids, n, index = R.labels(full_root(), 8, depth)
        assert n == 1 and not label.any() and index.tolist() == list(range(8))
        assert R.labels(full_root(), 8, depth, True)[2] == 8
    for axis in range(3):
        pair, apart = pair21(axis), pair21(axis, 1)
        assert pair.size == apart.size == 8 * 41
        assert R.labels(pair, pair.size, 21)[0].tolist() == [0, 0]  # the carry crosses every level
        assert R.labels(pair, pair.size, 21, True)[0].tolist() == [0, 1]
        assert R.labels(apart, apart.size, 21)[0].tolist() == [0, 1]  # they share an edge only
    assert R.labels(checkerboard(), checkerboard().size, 4)[2] == 2048
    words = path6()
    label, ids, n, _ = R.labels(words, words.size, 6)
    assert label.size == 2 * 32 ** 3 - 1 == 65535 and n == 1
    u, v, _, _ = R.links(words, words.size, 6)
    assert np.bincount(np.concatenate([u, v])).tolist().count(2) == 2 and u.size == 2 * 65534  # an induced path: two ends, each link from both sides


def test_the_lossless_merge_keeps_the_partition_of_the_cells():
    for name in ("ball", "percolation"):
        words, small, depth = merged(name)
        assert small.size < words.size
        before, after = R.labels(words, words.size, depth), R.labels(small, small.size, depth)
        cells_before, cells_after = R.entry_grid(words, words.size, depth)[0], R.entry_grid(small, small.size, depth)[0]
        held = cells_before >= 0
        assert np.array_equal(held, cells_after >= 0)
        assert R.same_partition(before[0][cells_before[held]], after[0][cells_after[held]]), name
        assert before[2] == after[2]


def test_drop_floating_on_a_grid():
    grid = np.zeros((8, 8, 8), dtype=np.int64)
    grid[:, 0, :] = 1          # the floor
    grid[2, 1:4, 2] = 2        # a pillar on it
    grid[5, 3:5, 5] = 3        # floats
    grid[0, 1, 7] = 0
    grid[6:8, 6:8, 6:8] = 4    # floats
    got, n, dropped = R.drop_floating(grid)
    want = grid.copy()
    want[5, 3:5, 5] = 0
    want[6:8, 6:8, 6:8] = 0
    assert np.array_equal(got, want) and (n, dropped) == (3, 2)
    got, n, dropped = R.drop_floating(grid, ((5, 4, 5), (6, 5, 6)))
    assert (got != 0).sum() == 2 and (got[5, 3:5, 5] == 3).all() and (n, dropped) == (3, 2)
    # per value the pillar is a component of its own, held by nothing on the floor layer
    got, n, dropped = R.drop_floating(grid, same_value=True)
    assert (n, dropped) == (4, 3) and np.array_equal(got != 0, grid == 1)
