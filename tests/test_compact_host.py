"""Compaction of a tree in the node buffer (csrc/svo_compact.hip), CPU side: the entry points are exported
with signatures; the sequential restatement (tests/compact_ref.py: compact) equals the host's svo_nodes_relayout without
pruning, and with pruning turns an edited tree into the tree built from the surviving voxels; the kernels' formulation
(compact_parallel) equals the sequential one; counters are kept; malformed trees are refused."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import compact_ref as K
import edit_ref as E
from test_edit_gpu import edit_voxels

NEW = ("svo_nodes_compact", "svo_compact_timing")


def test_new_entry_points_are_exported_with_signatures(pkg):
    L = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(L.svo_nodes_compact.argtypes) == 4 and len(L.svo_compact_timing.argtypes) == 2
    assert C.sizeof(pkg._lib.CompactParams) == 16
    assert callable(pkg.Render.compact_nodes) and callable(pkg.Gpu.compact_timing)


def base6_voxels():
    """the voxels of test_edit_gpu.py's base6: about 2 000 at depth 6, whole level-2 cells left empty"""
    rng = np.random.default_rng(60)
    coords = rng.integers(0, 40, (2000, 3))
    return coords, rng.integers(1, 1 << 24, 2000)


def survivors(depth, *lists):
    """(coords, colours) of the cells that hold a colour after the voxel lists were put one after the other"""
    cells = {}
    for coords, colours in lists:
        for key, colour, index in zip(*E.distinct(coords, depth, colours)):
            cells[int(key)] = (int(colour), np.asarray(coords)[index])
    kept = [(c, xyz) for c, xyz in cells.values() if c]
    return np.array([xyz for _, xyz in kept]).reshape(-1, 3), np.array([c for c, _ in kept], dtype=np.int64)


def orphaned(words, n, rng):
    """n interior words at mixed levels overwritten by the empty word: their subtrees stay behind, unreachable"""
    out = np.array(words, dtype=np.uint32)
    interior = np.flatnonzero(out >> 4 < B.VOXEL_OFFSET)
    out[np.concatenate([interior[:2], rng.choice(interior[2:], n - 2, replace=False)])] = B.EMPTY
    return out


@pytest.fixture(scope="module")
def edited():
    """base6 edited with 4 097 voxels at its depth: (A, B, the words in put order)"""
    a = base6_voxels()
    b = edit_voxels(np.random.default_rng(4097), 6, 4097, a[0], 0)
    base = B.build(a[0], 6, a[1])
    return a, b, E.edit(base, base.size, b[0], 6, b[1])


def assert_both(words, prune, want, want_perm=None):
    for f in (K.compact, K.compact_parallel):
        out, perm = f(words, words.size, prune)
        assert out.dtype == np.uint32 and out.size == want.size and np.array_equal(out, want), f.__name__
        if want_perm is not None:
            assert np.array_equal(perm, want_perm), f.__name__
    return out, perm


def test_without_pruning_it_is_the_hosts_relayout(pkg, small_words, monu9_words, edited):
    rng = np.random.default_rng(3)
    cases = {"small": np.asarray(small_words), "monu9": np.asarray(monu9_words), "edited": edited[2],
             "orphaned": orphaned(edited[2], 12, rng)}
    for name, words in cases.items():
        want, want_perm = pkg.scenes.relayout(words, 32, with_perm=True)
        assert_both(words, False, want, want_perm)
        assert (want.size < words.size) == (name == "orphaned"), name
    # words behind n_words are not the tree's
    padded = np.concatenate([cases["small"], np.arange(64, dtype=np.uint32)])
    want, want_perm = pkg.scenes.relayout(cases["small"], 32, with_perm=True)
    for f in (K.compact, K.compact_parallel):
        out, perm = f(padded, cases["small"].size, False)
        assert np.array_equal(out, want) and np.array_equal(perm, want_perm)


def test_pruning_an_edited_tree_gives_the_tree_of_the_surviving_voxels(edited):
    a, b, words = edited
    coords, colours = survivors(6, a, b)
    assert 0 < len(coords) < len(np.unique(B.morton(np.concatenate([a[0], b[0]]), 6)))  # (some cells were removed)
    want = B.build(coords, 6, colours)
    out, perm = assert_both(words, True, want)
    assert want.size < K.compact(words, words.size, False)[0].size <= words.size
    # a pruned, canonical tree is a fixed point
    assert_both(out, True, out, np.arange(out.size, dtype=np.uint32))
    # every voxel removed: the root group alone
    gone = E.edit(want, want.size, coords, 6, np.zeros(len(coords), dtype=np.int64))
    assert_both(gone, True, np.full(8, B.EMPTY, dtype=np.uint32), np.arange(8, dtype=np.uint32))
    assert K.compact(gone, gone.size, False)[0].size == want.size


def test_counters(edited):
    words = edited[2]
    rng = np.random.default_rng(8)
    counted = words | rng.integers(0, 16, words.size).astype(np.uint32)
    plain, perm = assert_both(words, False, K.compact(words, words.size, False)[0])
    out, perm_c = assert_both(counted, False, plain | (counted[perm] & 15), perm)
    assert np.array_equal(out & 15, counted[perm] & 15)
    plain, perm = K.compact(words, words.size, True)
    cut = (words[perm] >> 4 < B.VOXEL_OFFSET) & (plain == B.EMPTY)  # interior words whose group was dead
    assert cut.sum() > 10
    want = np.where(cut, B.EMPTY, plain | (counted[perm] & 15)).astype(np.uint32)
    assert_both(counted, True, want, perm)


def malformed_cases():
    """{name: (words, part of the message)} over a small canonical tree"""
    rng = np.random.default_rng(2)
    base = B.build(rng.integers(0, 16, (60, 3)), 4, rng.integers(1, 1 << 24, 60))
    interior = np.flatnonzero(base >> 4 < B.VOXEL_OFFSET)
    leaf = np.flatnonzero(base >> 4 >= B.VOXEL_OFFSET)
    cases = {}
    w = base.copy()
    w[leaf[-1]] = base.size << 4
    cases["a pointer with pointer + 8 > n_words"] = w
    w = base.copy()
    w[interior[3]] = ((base[interior[3]] >> 4) + 4) << 4
    cases["an unaligned pointer"] = w
    w = base.copy()
    w[interior[1]] = base[interior[0]]
    cases["two parents sharing one group"] = w
    w = base.copy()
    w[leaf[-1]] = 0 << 4
    cases["a cycle through the root"] = w
    chain = np.full(8 * 32, B.EMPTY, dtype=np.uint32)
    chain[np.arange(31) * 8 + 5] = (np.arange(1, 32) * 8) << 4
    cases["32 levels"] = chain
    return cases


def test_malformed_trees_are_refused(pkg):
    cases = malformed_cases()
    for name, words in cases.items():
        for f in (K.compact, K.compact_parallel):
            for prune in (False, True):
                with pytest.raises(K.Malformed):
                    f(words, words.size, prune)
        with pytest.raises(ValueError):  # (the host's relayout refuses them too)
            pkg.scenes.relayout(words, 32)
    # the shared group is only an error while both parents are reachable; 31 levels are fine
    ok = cases["32 levels"][: 8 * 31].copy()
    ok[30 * 8 + 5] = (B.VOXEL_OFFSET + 7) << 4
    assert K.compact(ok, ok.size, True)[0].size == ok.size
    ok[30 * 8 + 5] = B.EMPTY
    assert K.compact_parallel(ok, ok.size, True)[0].size == 8
    for n in (0, 12, 4, cases["32 levels"].size + 8):
        for f in (K.compact, K.compact_parallel):
            with pytest.raises(ValueError):
                f(cases["32 levels"], n, False)
