"""In-place tree edits (csrc/svo_edit.hip), CPU side: the entry points are exported with signatures; the
sequential restatement (tests/edit_ref.py: edit) equals the host model's put_in_voxel word for word; and the kernels'
formulation (edit_parallel: plan with l = max(l0, c + 1), scan, fill, link) equals the sequential one."""
import ctypes as C

import numpy as np
import pytest

import edit_ref as E
from build_ref import EMPTY, VOXEL_OFFSET, build, morton
from conftest import load_vox_fixture

NEW = ("svo_nodes_edit", "svo_edit_timing")


def test_new_entry_points_are_exported_with_signatures(pkg):
    L = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(L.svo_nodes_edit.argtypes) == 6 and len(L.svo_edit_timing.argtypes) == 2
    assert C.sizeof(pkg._lib.EditParams) == 24
    assert callable(pkg.Render.edit_nodes) and callable(pkg.Gpu.edit_timing)


def host_put(pkg, tree, coords, depth, colours):
    """put_in_voxel per distinct cell in ascending key order, the last voxel of a cell winning"""
    keys, col, index = E.distinct(coords, depth, colours)
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    for i, v in zip(index, col):
        pos = [float(x) / (1 << depth) * 2 - 1 for x in c[i]]
        tree.put_in_voxel(pos, pkg.Voxel.from_value(int(v)), depth)


def host_base(pkg, coords, depth, colours):
    tree = pkg.CpuOctree.new(0)
    host_put(pkg, tree, coords, depth, colours)
    return tree


def edits(rng, depth, n, near=None):
    """n edit voxels: random cells, some near `near` (existing voxels: overwrites and shared prefixes), duplicate
    cells, colour 0 and colours with only high bits"""
    side = 1 << depth
    coords = rng.integers(0, side, (n, 3))
    if near is not None and len(near) and n >= 4:
        pick = np.asarray(near)[rng.integers(0, len(near), n // 2)]
        coords[: n // 2] = np.clip(pick + rng.integers(-1, 2, (n // 2, 3)), 0, side - 1)
    if n >= 8:
        coords[n - n // 4:] = coords[: n // 4]  # duplicates: the later one wins
    colours = rng.integers(1, 1 << 32, n)
    colours[::5] = 0
    colours[1::9] = 0xFF000000
    return coords, colours


CASES = [  # (base depth, base voxels, edit depth, edit voxels)
    (1, 0, 1, 8), (1, 3, 1, 5), (2, 0, 2, 1), (2, 6, 2, 30), (5, 300, 5, 500), (8, 2000, 8, 3000), (5, 300, 8, 800),
    (2, 5, 8, 300), (8, 500, 8, 0),
]


@pytest.mark.parametrize("base_depth,n_base,depth,n", CASES)
def test_sequential_reference_equals_the_host_model(pkg, base_depth, n_base, depth, n):
    rng = np.random.default_rng(1000 * base_depth + depth + n)
    bc = rng.integers(0, 1 << base_depth, (n_base, 3))
    bcol = rng.integers(0, 1 << 24, n_base)
    tree = host_base(pkg, bc, base_depth, bcol)
    base = tree.to_octree_words()
    coords, colours = edits(rng, depth, n, near=bc * (1 << (depth - base_depth)) if n_base else None)
    if depth == 1:
        coords = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])[:n]
        colours = colours[: len(coords)]
    # cells the base refines below the edit's depth do not occur here: the base is never deeper than the edit
    host_put(pkg, tree, coords, depth, colours)
    want = tree.to_octree_words()
    got = E.edit(base, base.size, coords, depth, colours)
    assert got.size == want.size and np.array_equal(got, want)
    assert np.array_equal(E.edit_parallel(base, base.size, coords, depth, colours), want)


def test_from_voxels_base_and_small_fixture(pkg):
    size, xyzi, pal, n, _ = load_vox_fixture("small")
    tree = pkg.CpuOctree.from_voxels(size, xyzi, pal)
    base = tree.to_octree_words()
    depth = int(size).bit_length() - 1
    rng = np.random.default_rng(4)
    coords, colours = edits(rng, depth, 400)
    host_put(pkg, tree, coords, depth, colours)
    want = tree.to_octree_words()
    assert np.array_equal(E.edit(base, base.size, coords, depth, colours), want)
    assert np.array_equal(E.edit_parallel(base, base.size, coords, depth, colours), want)
    # two levels deeper: coloured leaves split, their children come out empty
    tree = pkg.CpuOctree.from_voxels(size, xyzi, pal)
    coords, colours = edits(rng, depth + 2, 300)
    host_put(pkg, tree, coords, depth + 2, colours)
    want = tree.to_octree_words()
    assert np.array_equal(E.edit(base, base.size, coords, depth + 2, colours), want)
    assert np.array_equal(E.edit_parallel(base, base.size, coords, depth + 2, colours), want)


@pytest.mark.parametrize("seed", range(12))
def test_parallel_formulation_equals_the_sequential_one_on_random_cases(seed):
    rng = np.random.default_rng(seed)
    base_depth = int(rng.integers(1, 7))
    depth = int(rng.integers(base_depth, min(base_depth + 6, 22)))
    if seed == 0:
        base_depth, depth = 3, 21
    n_base = int(rng.integers(0, 400))
    bc = rng.integers(0, 1 << base_depth, (n_base, 3))
    base = build(bc, base_depth, rng.integers(0, 1 << 24, n_base))
    if seed % 3 == 1:  # hit counters on the base: unwritten words keep them, the walk ignores them
        base = base | rng.integers(0, 16, base.size).astype(np.uint32)
    n = int(rng.integers(1, 600))
    coords, colours = edits(rng, depth, n, near=bc * (1 << (depth - base_depth)) if n_base else None)
    if depth > base_depth and n >= 64:  # clusters that share deep prefixes under one cell
        corner = (coords[0] >> 3) << 3
        coords[8:40] = corner + rng.integers(0, 8, (32, 3))
    want = E.edit(base, base.size, coords, depth, colours)
    got = E.edit_parallel(base, base.size, coords, depth, colours)
    assert got.size == want.size and np.array_equal(got, want)
    perm = rng.permutation(len(coords))
    keys = morton(coords, depth)
    if np.unique(keys).size == keys.size:
        assert np.array_equal(E.edit(base, base.size, coords[perm], depth, colours[perm]), want)


def test_reference_small_cases_by_hand():
    leaf = lambda c: (VOXEL_OFFSET + c) << 4  # noqa: E731
    root = np.full(8, EMPTY, dtype=np.uint32)
    # depth 1: root-group writes only; colour 0 removes
    w = E.edit(root, 8, [[1, 0, 1], [0, 0, 0], [1, 0, 1]], 1, [1, 2, 3])
    assert w.tolist() == [leaf(2), EMPTY, EMPTY, EMPTY, EMPTY, leaf(3), EMPTY, EMPTY]
    assert E.edit(w, 8, [[0, 0, 0]], 1, [0]).tolist() == [EMPTY] * 5 + [leaf(3), EMPTY, EMPTY]
    # depth 2 into the depth-1 leaf 5: it splits, the children are empty but for the voxel; counters of other words stay
    w2 = E.edit(w | np.uint32(3), 8, [[3, 0, 3]], 2, [7])
    assert w2.tolist() == [leaf(2) | 3] + [EMPTY | 3] * 4 + [8 << 4, EMPTY | 3, EMPTY | 3] + [EMPTY] * 5 + [leaf(7), EMPTY, EMPTY]
    # the same cell edited at depth 1 is an interior node there: refused, naming the input index
    with pytest.raises(E.Refused) as e:
        E.edit(w2, 16, [[0, 1, 0], [1, 0, 1]], 1, [1, 1])
    assert e.value.index == 1
    with pytest.raises(E.Refused) as e:
        E.edit_parallel(w2, 16, [[0, 1, 0], [1, 0, 1]], 1, [1, 1])
    assert e.value.index == 1
