"""Listing the voxels of a tree in the node buffer (csrc/svo_list.hip), CPU side: the entry points are
exported with signatures and declared in the header, ListParams has the header's layout; the sequential restatement
(tests/list_ref.py: list_voxels) inverts the builder's reference; the kernels' formulation (list_parallel) equals the
sequential one on built, edited, orphaned, counter-carrying and mixed-level trees, natively and expanded, and refuses
what it refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import build_ref as B
import compact_ref as K
import edit_ref as E
import list_ref as L
from conftest import ROOT as REPO
from test_compact_host import base6_voxels, malformed_cases, orphaned, survivors
from test_edit_gpu import edit_voxels

NEW = ("svo_nodes_list_voxels", "svo_list_timing")
EMPTY_ROOT = np.full(8, B.EMPTY, dtype=np.uint32)


def leaf_words(values):
    return ((B.VOXEL_OFFSET + np.asarray(values, dtype=np.int64)) << 4).astype(np.uint32)


def full_root():
    """a root group of 8 coloured words"""
    return leaf_words(np.arange(1, 9) * 0x010203)


def one_leaf_root(value=0xABCDEF, child=5):
    """one level-1 voxel"""
    w = EMPTY_ROOT.copy()
    w[child] = leaf_words([value])[0]
    return w


def word_levels(canonical):
    """the level of every word of a canonical breadth-first tree"""
    levels = np.zeros(canonical.size, dtype=np.int64)
    lo, hi, level = 0, 1, 1
    while hi > lo:
        levels[8 * lo:8 * hi] = level
        n = int((canonical[8 * lo:8 * hi] >> 4 < B.VOXEL_OFFSET).sum())
        lo, hi, level = hi, hi + n, level + 1
    return levels


def mixed_levels():
    """a depth-6 build of 3 000 random voxels in which about 40 interior words of the levels 2 to 5 were overwritten by
    coloured leaf words: leaves at mixed levels, orphaned groups behind them"""
    rng = np.random.default_rng(63)
    words = B.build(rng.integers(0, 64, (3000, 3)), 6, rng.integers(1, 1 << 24, 3000))
    levels = word_levels(words)
    interior = words >> 4 < B.VOXEL_OFFSET
    for level in (2, 3, 4, 5):
        at = rng.choice(np.flatnonzero(interior & (levels == level)), 10, replace=False)
        words[at] = leaf_words(rng.integers(1, 1 << 24, 10))
    return words


def voxel_list(depth, coords, colours):
    """what the list of build(coords, colours) must be: last wins, colour 0 dropped, sorted by Morton key"""
    c, col = survivors(depth, (coords, colours))
    by_key = np.argsort(B.morton(c, depth), kind="stable")
    return c[by_key].astype(np.uint32), (col[by_key] & 0xFFFFFF).astype(np.uint32)


def assert_lists_equal(got, want, what=""):
    for g, w, name in zip(got, want, ("xyz", "value", "level")):
        assert g.dtype == np.uint32 and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name}"


@pytest.fixture(scope="module")
def edited():
    """test_compact_host's: base6 edited with 4 097 voxels at its depth: (A, B, the words in put order)"""
    a = base6_voxels()
    b = edit_voxels(np.random.default_rng(4097), 6, 4097, a[0], 0)
    base = B.build(a[0], 6, a[1])
    return a, b, E.edit(base, base.size, b[0], 6, b[1])


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_list_voxels.argtypes) == 6 and len(lib.svo_list_timing.argtypes) == 2
    assert callable(pkg.Render.list_voxels) and callable(pkg.Gpu.list_timing) and callable(pkg.World.save_nodes)


def test_list_params_have_the_headers_layout(pkg):
    P = pkg._lib.ListParams
    assert C.sizeof(P) == 24
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("flags", 0, 4), ("depth", 4, 4), ("n_words", 8, 8), ("max_voxels", 16, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_list_params \{(.*?)\} svo_list_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [("uint32_t", "flags"), ("uint32_t", "depth"), ("uint64_t", "n_words"),
                                                             ("uint64_t", "max_voxels")]


def test_the_header_declares_both_functions():
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    assert re.search(r"int svo_nodes_list_voxels\(svo_ctx \*ctx, const svo_list_params \*p, uint32_t \*xyz_out_dev, "
                     r"uint32_t \*value_out_dev,\s*uint32_t \*level_out_dev[^,]*, uint64_t \*n_out\);", header)
    assert re.search(r"#define SVO_LIST_TIMES 5\nint svo_list_timing\(svo_ctx \*ctx, float ms_out\[SVO_LIST_TIMES\]\);", header)
    assert "#define SVO_LIST_EXPAND 1u" in header


def test_listing_inverts_the_builder(edited):
    rng = np.random.default_rng(18)
    a = rng.integers(0, 32, (1500, 3)), rng.integers(0, 1 << 24, 1500)
    a[0][1000:] = a[0][:500]  # duplicate cells: the later one wins
    a[1][::7] = 0             # colour 0: an empty leaf on a path that exists
    want = voxel_list(5, *a)
    assert 0 < want[1].size < len(np.unique(B.morton(a[0], 5)))
    for f in (L.list_voxels, L.list_parallel):
        words = B.build(a[0], 5, a[1])
        xyz, value, level = f(words, words.size, 5)
        assert_lists_equal((xyz, value), want, f.__name__)
        assert (level == 5).all()
        # an expansion at the tree's own depth changes nothing; the list rebuilds the pruned tree
        assert_lists_equal(f(words, words.size, 5, expand=True), (xyz, value, level), f.__name__)
        assert np.array_equal(B.build(xyz, 5, value), K.compact(words, words.size, True)[0])
    # an edited tree lists as the surviving voxels, whatever its layout
    a, b, words = edited
    c, col = survivors(6, a, b)
    want = voxel_list(6, c, col)
    for layout in (words, K.compact(words, words.size, False)[0], K.compact(words, words.size, True)[0]):
        assert_lists_equal(L.list_voxels(layout, layout.size, 6)[:2], want)


def test_parallel_equals_sequential(edited, small_words, monu9_words):
    rng = np.random.default_rng(5)
    top = (1 << 21) - 1
    mixed = mixed_levels()
    trees = {
        "empty root": (EMPTY_ROOT, 1, 3), "full root": (full_root(), 1, 4), "one level-1 voxel": (one_leaf_root(), 1, 3),
        "depth 21": (B.build([[top, 5, 1234567]], 21, [0x00FF00]), 21, 21),
        "edited": (edited[2], 6, 7), "orphaned": (orphaned(edited[2], 12, rng), 6, 6), "mixed levels": (mixed, 6, 6),
        "counters": (mixed | rng.integers(0, 16, mixed.size).astype(np.uint32), 6, 6),
        "small": (np.asarray(small_words), None, None), "monu9": (np.asarray(monu9_words), None, None),
    }
    for name, (words, depth, deeper) in trees.items():
        if depth is None:  # a host-layout fixture: its depth is what the walk finds
            depth = deeper = max(L.list_voxels(words, words.size, 21)[2])
        for d in {depth, deeper}:
            for expand in (False, True):
                want = L.list_voxels(words, words.size, d, expand)
                assert_lists_equal(L.list_parallel(words, words.size, d, expand), want, f"{name}, depth {d}, expand {expand}")
                keys = B.morton(want[0], d)
                assert (np.diff(keys.astype(np.int64)) > 0).all(), f"{name}: not in ascending Morton order"
                if expand:
                    assert (want[2] == d).all()
    assert_lists_equal(L.list_voxels(trees["counters"][0], mixed.size, 6), L.list_voxels(mixed, mixed.size, 6))
    # the contract's small cases, spelled out
    xyz, value, level = L.list_voxels(full_root(), 8, 4)
    cells = np.array([[c >> 2 & 1, c >> 1 & 1, c & 1] for c in range(8)], dtype=np.uint32)
    assert np.array_equal(xyz, cells << 3) and np.array_equal(value, np.arange(1, 9) * 0x010203) and (level == 1).all()
    xyz, value, level = L.list_voxels(trees["depth 21"][0], 168, 21)
    assert xyz.tolist() == [[top, 5, 1234567]] and value.tolist() == [0x00FF00] and level.tolist() == [21]
    xyz, value, level = L.list_voxels(one_leaf_root(), 8, 3, expand=True)
    assert xyz.shape == (64, 3) and (value == 0xABCDEF).all() and (level == 3).all()
    assert np.array_equal(xyz, L.demorton(5 * 64 + np.arange(64), 3)) and xyz.min(axis=0).tolist() == [4, 0, 4]
    # mixed levels: levels 2 to 6 occur, the orphans do not count, and the expansion stays small
    levels = L.list_voxels(mixed, mixed.size, 6)[2]
    assert set(levels.tolist()) == {2, 3, 4, 5, 6}
    assert L.list_voxels(mixed, mixed.size, 6, expand=True)[1].size < 200_000
    assert K.compact(mixed, mixed.size, False)[0].size < mixed.size


def test_what_is_refused(edited):
    for name, words in malformed_cases().items():
        for f in (L.list_voxels, L.list_parallel):
            for expand in (False, True):
                with pytest.raises(K.Malformed):
                    f(words, words.size, 21, expand)
    words = edited[2]
    for f in (L.list_voxels, L.list_parallel):
        with pytest.raises(L.TooDeep) as e:
            f(words, words.size, 4)
        assert e.value.level == 6
        for depth in (0, 22):
            with pytest.raises(ValueError):
                f(words, words.size, depth)
        for n in (0, 12, words.size + 8):
            with pytest.raises(ValueError):
                f(words, n, 6)
        with pytest.raises(L.TooMany) as e:
            f(one_leaf_root(), 8, 21, expand=True)
        assert e.value.count == 8 ** 20
        assert f(one_leaf_root(), 8, 21)[0].tolist() == [[1 << 20, 0, 1 << 20]]
    # an all-empty group below `depth` holds no voxel and no interior word: it is not too deep
    gone = E.edit(words, words.size, [[1, 2, 3]], 7, [0])
    assert gone.size > words.size and L.list_voxels(gone, gone.size, 7)[2].max() == 6
    assert_lists_equal(L.list_parallel(gone, gone.size, 6), L.list_voxels(gone, gone.size, 6))
