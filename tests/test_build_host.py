"""GPU tree builder (csrc/svo_build.hip), CPU side: the new entry points are exported with signatures,
and the numpy restatement of the contract (tests/build_ref.py) equals the host-built tree in canonical breadth-first
order, relayout(words, block_level=32), for every .vox fixture and for random voxel sets."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
from conftest import GOLDEN

NEW = ("svo_nodes_build", "svo_nodes_build_dense", "svo_buffer_write", "svo_build_timing")


def test_new_entry_points_are_exported_with_signatures(pkg):
    L = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(L.svo_nodes_build.argtypes) == 6 and len(L.svo_nodes_build_dense.argtypes) == 4
    assert C.sizeof(pkg._lib.BuildParams) == 16
    for method in ("build_nodes", "build_nodes_dense", "from_voxels"):
        assert callable(getattr(pkg.Render, method))
    assert callable(pkg.Gpu.build_timing)


def host_tree(pkg, size, xyzi, pal):
    return pkg.scenes.relayout(pkg.CpuOctree.from_voxels(size, xyzi, pal).to_octree_words(), block_level=32)


@pytest.mark.parametrize("name", B.FIXTURES)
def test_reference_equals_relayouted_host_tree_on_fixtures(pkg, name):
    for label, size, xyzi, pal in B.fixture_models(GOLDEN, name):
        want = host_tree(pkg, size, xyzi, pal)
        coords, colours, depth = B.vox_voxels(size, xyzi, pal)
        got = B.build(coords, depth, colours)
        assert got.size == want.size, label
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{label}: {bad.size} words differ, first {bad[:5]}"


@pytest.mark.parametrize("size,n", [(2, 5), (4, 40), (16, 3000), (64, 20000), (256, 60000)])
def test_reference_equals_host_tree_on_random_sets(pkg, size, n):
    rng = np.random.default_rng(size * 7 + n)
    xyzi = np.empty((n, 4), dtype=np.uint8)
    xyzi[:, :3] = rng.integers(0, size, (n, 3))
    xyzi[:, 3] = rng.integers(0, 256, n)
    xyzi[n // 2:, :3] = xyzi[: n - n // 2, :3]  # duplicates: the later one wins
    xyzi[-1, 3] = 0  # palette entry 0 (colour 0), and the winner of a duplicate cell
    pal = rng.integers(0, 2**32, 256, dtype=np.uint64).astype(np.uint32)
    pal[rng.integers(0, 256, 16)] = 0xFF000000  # colour 0 (alpha only): empty leaves on existing paths
    pal[0] = 0
    want = host_tree(pkg, size, xyzi, pal)
    coords, colours, depth = B.vox_voxels(size, xyzi, pal)
    got = B.build(coords, depth, colours)
    assert np.array_equal(got, want)
    assert (colours == 0).any()


def test_reference_small_cases_by_hand():
    E = B.EMPTY
    leaf = lambda c: (B.VOXEL_OFFSET + c) << 4  # noqa: E731
    assert B.build(np.zeros((0, 3)), 3).tolist() == [E] * 8
    # depth 1: the root group holds the leaves; (1, 0, 1) is child 4 | 1 = 5; the last of two voxels in one cell wins
    assert B.build([[1, 0, 1], [0, 0, 0], [1, 0, 1]], 1, [1, 2, 3]).tolist() == [leaf(2), E, E, E, E, leaf(3), E, E]
    # depth 2: (3, 3, 3) -> child 7 of the root, child 7 of that
    w = B.build([[3, 3, 3]], 2, colour=0x123456).tolist()
    assert w == [E] * 7 + [8 << 4] + [E] * 7 + [leaf(0x123456)]
    # a dense grid and its non-zero cells
    g = np.zeros((4, 4, 4), dtype=np.uint32)
    g[3, 3, 3] = 0x01123456
    coords, col = B.dense_to_voxels(g)
    assert coords.tolist() == [[3, 3, 3]] and col.tolist() == [0x123456]
