"""A tree sampled on the GPU (csrc/svo_sample.hip): values, levels and indices of svo_nodes_sample and the
dense array of svo_nodes_sample_dense against the rule's restatement (tests/sample_ref.py: sample), bit for bit, on empty,
full, depth-21, built, edited, compacted, counter-carrying, mixed-level and malformed trees; nothing written behind the
outputs, nothing on any error, the node buffer never; the same bytes on every run and for every layout of a tree; an edit
through a sharing context seen; a device adaptive state no obstacle.

Layouts: the put order and its compaction without pruning are two layouts of one tree and sample identically, levels
included.  Pruning replaces every group that holds nothing by one empty word, which is another tree with the same voxels:
on tree7 59 200 empty cells of the 128^3 grid are then found at a coarser level (the rule over the pruned words gives that
figure on the CPU, and the test asserts it), so for the pruned tree the test asks for identical values everywhere, identical levels wherever the cell holds a
voxel and no deeper level anywhere, next to the bit-for-bit comparison with the rule over the pruned words."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import list_ref as L
import sample_ref as S
from pass_frame import SLACK, SentinelOut, last_error, monu9_world, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, PAD, ROOT, poison, set_base
from test_list_host import full_root, mixed_levels, one_leaf_root
from test_sample_host import BOXES, DEEP_CELL, deep_cells

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
WHOLE7 = ((0, 0, 0), (128, 128, 128))


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def tree7():
    """pass_frame.tree7_base (the base, the edited words in put order) with the words' list and the rule over every cell
    of the 128^3 grid, computed once"""
    t = tree7_base()
    words, cells = t["words"], S.box_cells(*WHOLE7)
    return {**t, "list": L.list_voxels(words, words.size, 7), "cells": cells, "whole": S.sample(words, words.size, cells, 7)}


def device_cells(gpu, cells):
    """(N, 3) cells, u32 bit patterns, as an int32 device tensor"""
    import torch
    c = (np.asarray(cells, dtype=np.int64).reshape(-1, 3) & 0xFFFFFFFF).astype(np.uint32)
    t = torch.as_tensor(c.view(np.int32), device=torch.device("cuda", gpu.device)).contiguous()
    torch.cuda.current_stream(t.device).synchronize()
    return t


class Out(SentinelOut):
    """`arrays` sentinel-filled device outputs of `n` entries and SLACK more"""

    def __init__(self, gpu, n, arrays=3):
        super().__init__(gpu, [n + SLACK] * arrays)
        self.n = n

    def ptr(self, k):
        return self.t[k].data_ptr() if k < len(self.t) else None


def raw_sample(pkg, gpu, depth, n_words, xyz, n, out, flags=0, params=True, give_xyz=True, give_value=True):
    p = pkg._lib.SampleParams()
    p.flags, p.depth, p.n_words = flags, depth, n_words
    rc = pkg._lib.lib().svo_nodes_sample(gpu._h, C.byref(p) if params else None, xyz.data_ptr() if give_xyz else None, n,
                                         out.ptr(0) if give_value else None, out.ptr(1), out.ptr(2))
    gpu.sync()
    return rc


def raw_dense(pkg, gpu, depth, n_words, origin, size, out, flags=0, params=True, give_origin=True, give_size=True, give_grid=True):
    p = pkg._lib.SampleParams()
    p.flags, p.depth, p.n_words = flags, depth, n_words
    rc = pkg._lib.lib().svo_nodes_sample_dense(gpu._h, C.byref(p) if params else None, (C.c_uint32 * 3)(*origin) if give_origin else None,
                                               (C.c_uint32 * 3)(*size) if give_size else None, out.ptr(0) if give_grid else None)
    gpu.sync()
    return rc


def assert_same(got, want, what, name):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} entries differ in {name}, first at {bad[:3]}: got {got[bad[:3]]} want {want[bad[:3]]}")


def loaded(render, words, already):
    if not already:
        set_base(render, words)
    before = render.read_nodes(words.size + PAD)
    assert np.array_equal(before[:words.size], words) and (already or np.array_equal(before[words.size:], poison(PAD)))
    return before


def check_points(pkg, render, words, depth, cells, what, want=None, already=False):
    """the cells sampled on the GPU == the rule, levels and indices included; nothing is written behind n; the node
    buffer, with its poison behind it, reads back unchanged.  Returns the three host arrays."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    n = len(cells)
    want = want if want is not None else S.sample(words, words.size, cells, depth)
    before = loaded(render, words, already)
    out = Out(render.gpu, n)
    rc = raw_sample(pkg, render.gpu, depth, words.size, device_cells(render.gpu, cells), n, out)
    assert rc == 0, f"{what}: status {rc}: {last_error(pkg, render.gpu)}"
    got = out.host()
    for g, w, name in zip(got, want, ("value", "level", "index")):
        assert_same(g[:n], w, what, name)
    assert out.untouched_from(n), f"{what}: written behind n"
    assert np.array_equal(render.read_nodes(words.size + PAD), before), f"{what}: the node buffer was written"
    return tuple(g[:n] for g in got)


def check_box(pkg, render, words, depth, origin, size, what, want=None, already=False):
    """the box sampled on the GPU == the rule over its cells; nothing is written behind the box's cells; the node
    buffer reads back unchanged.  Returns the array, shaped `size`."""
    n = size[0] * size[1] * size[2]
    want = want if want is not None else S.sample_dense(words, words.size, origin, size, depth)
    before = loaded(render, words, already)
    out = Out(render.gpu, n, arrays=1)
    rc = raw_dense(pkg, render.gpu, depth, words.size, origin, size, out)
    assert rc == 0, f"{what}: status {rc}: {last_error(pkg, render.gpu)}"
    got = out.host()[0]
    assert_same(got[:n], np.asarray(want).reshape(-1), what, "the dense values")
    assert out.untouched_from(n), f"{what}: written behind the box"
    assert np.array_equal(render.read_nodes(words.size + PAD), before), f"{what}: the node buffer was written"
    return got[:n].reshape(tuple(size))


def test_empty_and_full_root(pkg, render):
    octants = np.array([[c >> 2 & 1, c >> 1 & 1, c & 1] for c in range(8)])
    full = full_root()
    for depth in (1, 5, 21):
        side = 1 << depth
        value, level, index = check_points(pkg, render, ROOT, depth, octants << (depth - 1), f"empty root, depth {depth}")
        assert (value == 0).all() and (level == 1).all() and index.tolist() == list(range(8))
        value, level, index = check_points(pkg, render, full, depth, octants << (depth - 1), f"full root, depth {depth}")
        assert np.array_equal(value, (full >> 4) - B.VOXEL_OFFSET) and (level == 1).all() and index.tolist() == list(range(8))
        box = ((0, 0, 0), (side,) * 3) if depth < 21 else ((side - 3,) * 3, (3, 3, 3))
        assert (check_box(pkg, render, ROOT, depth, *box, f"empty root, depth {depth}") == 0).all()
        grid = check_box(pkg, render, full, depth, *box, f"full root, depth {depth}")
        if depth < 21:
            half = side // 2
            assert all((grid[x * half:(x + 1) * half, y * half:(y + 1) * half, z * half:(z + 1) * half] == (x * 4 + y * 2 + z + 1) * 0x010203).all()
                       for x, y, z in octants)
        else:
            assert (grid == 8 * 0x010203).all()


def test_depth_21_voxel(pkg, render):
    words = B.build([DEEP_CELL], 21, [0x00FF00])
    cells = deep_cells()
    value, level, index = check_points(pkg, render, words, 21, cells, "depth 21")
    assert value[0] == 0x00FF00 and level[0] == 21 and (value[1:7] == 0).all() and (value[7:] == S.OUTSIDE).all()
    octree = pkg.Octree.from_words(words)
    for cell, l, i in zip(cells[:7], level, index):  # the voxel and its six face neighbours
        found, found_level, _ = octree.find_voxel(((cell + 0.5) * (2.0 / (1 << 21)) - 1.0).tolist(), max_depth=21)
        assert (found, found_level) == (int(i), int(l)), cell
    box = check_box(pkg, render, words, 21, [c - 1 for c in DEEP_CELL[:2]] + [DEEP_CELL[2] - 2], (2, 3, 4), "depth 21, a box round the voxel")
    assert box[1, 1, 2] == 0x00FF00 and (box != 0).sum() == 1
    # the public call: int32 tensors, a negative coordinate comes back OUTSIDE
    got = render.sample_voxels(np.concatenate([cells[:7], [[-1, 0, 0]]]), 21, with_levels=True, with_indices=True)
    assert all(t.dtype.is_signed and t.dtype.itemsize == 4 and t.is_cuda and t.shape == (8,) for t in got)
    assert got[0].cpu().numpy().tolist() == [0x00FF00, 0, 0, 0, 0, 0, 0, S.OUTSIDE]
    assert np.array_equal(got[1].cpu().numpy()[:7].view(np.uint32), level[:7]) and got[2].cpu().numpy()[7] == -1
    alone = render.sample_voxels(cells[:1], 21)
    assert alone.shape == (1,) and int(alone[0]) == 0x00FF00
    assert render.sample_voxels(np.zeros((0, 3), dtype=np.int64), 21).shape == (0,)
    # depth=None: the declared depth, which a build at depth 21 raises to 21
    assert render.build_nodes(cells[:1], 21, [0x00FF00]) == words.size
    assert render.sample_voxels(cells[:8]).tolist() == [0x00FF00, 0, 0, 0, 0, 0, 0, S.OUTSIDE]


def test_edited_tree_whole_grid_partial_waves_and_counters(pkg, render, tree7):
    words, cells, whole = tree7["words"], tree7["cells"], tree7["whole"]
    grid = check_box(pkg, render, words, 7, *WHOLE7, "tree7, the whole grid", whole[0])
    rng = np.random.default_rng(3)
    for n in (1, 63, 65, 100_003):
        pick = rng.integers(0, len(cells), n)
        check_points(pkg, render, words, 7, cells[pick], f"tree7, {n} points", tuple(w[pick] for w in whole), already=True)
    # every listed voxel samples to its listed colour, at its level
    xyz, value, level = tree7["list"]
    got = check_points(pkg, render, words, 7, xyz, "tree7, the listed voxels", already=True)
    assert np.array_equal(got[0], value) and np.array_equal(got[1], level)
    assert np.array_equal(grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]], value) and (grid != 0).sum() == len(value)
    # random counter bits in every word: the same outputs
    counted = words | np.random.default_rng(6).integers(0, 16, words.size).astype(np.uint32)
    check_box(pkg, render, counted, 7, *WHOLE7, "tree7 with counters, the whole grid", whole[0])
    pick = rng.integers(0, len(cells), 5000)
    check_points(pkg, render, counted, 7, cells[pick], "tree7 with counters", tuple(w[pick] for w in whole), already=True)


def test_every_layout_and_every_run_sample_identically(pkg, render, tree7):
    words, cells, whole = tree7["words"], tree7["cells"], tree7["whole"]
    put = check_points(pkg, render, words, 7, cells, "put order", whole)
    again = check_points(pkg, render, words, 7, cells, "put order, second run", whole, already=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(put, again))
    put_box = check_box(pkg, render, words, 7, *WHOLE7, "put order, dense", whole[0], already=True)
    assert put_box.tobytes() == check_box(pkg, render, words, 7, *WHOLE7, "put order, dense, second run", whole[0], already=True).tobytes()
    for prune in (False, True):
        set_base(render, words)
        n, perm = render.compact_nodes(prune=prune, with_perm=True)
        layout = render.read_nodes()
        assert n == layout.size and (n < words.size) == prune
        got = check_points(pkg, render, layout, 7, cells, f"compacted, prune {prune}")
        box = check_box(pkg, render, layout, 7, *WHOLE7, f"compacted, prune {prune}, dense", got[0], already=True)
        assert got[0].tobytes() == put[0].tobytes() and box.tobytes() == put_box.tobytes()
        if not prune:  # another layout of the same tree
            assert got[1].tobytes() == put[1].tobytes()
            assert np.array_equal(perm.cpu().numpy().view(np.uint32)[got[2]], put[2])
        else:  # (see the module's docstring)
            holds = put[0] != 0
            assert np.array_equal(got[1][holds], put[1][holds]) and (got[1] <= put[1]).all()
            assert int((got[1] < put[1]).sum()) == 59_200  # (the rule over the pruned words, on the CPU)


def test_mixed_levels_below_at_and_above_the_grid(pkg, render):
    mixed = mixed_levels()
    whole6 = S.box_cells((0, 0, 0), (64, 64, 64))
    value, level, index = check_points(pkg, render, mixed, 6, whole6, "mixed levels, depth 6")
    assert set(level.tolist()) == {2, 3, 4, 5, 6} and (value < S.FINER).all()
    grid = check_box(pkg, render, mixed, 6, (0, 0, 0), (64, 64, 64), "mixed levels, depth 6, dense", value, already=True)
    assert (grid != 0).sum() == L.list_voxels(mixed, mixed.size, 6, expand=True)[1].size
    # leaves above the grid: the depth-8 grid, a box no brick of which is aligned with it
    fine = check_box(pkg, render, mixed, 8, (37, 50, 61), (100, 128, 77), "mixed levels, depth 8, dense", already=True)
    assert (fine != 0).any() and (fine < S.FINER).all()
    pick = np.random.default_rng(8).integers(0, 256, (5000, 3))
    assert set(check_points(pkg, render, mixed, 8, pick, "mixed levels, depth 8", already=True)[1].tolist()) <= {1, 2, 3, 4, 5, 6}
    # the tree refined below the grid: FINER
    coarse = check_box(pkg, render, mixed, 4, (0, 0, 0), (16, 16, 16), "mixed levels, depth 4, dense", already=True)
    assert (coarse == S.FINER).any() and ((coarse != 0) & (coarse < S.FINER)).any()
    value, level, index = check_points(pkg, render, mixed, 4, S.box_cells((0, 0, 0), (16, 16, 16)), "mixed levels, depth 4", already=True)
    assert np.array_equal(value, coarse.reshape(-1)) and (level[value == S.FINER] == 4).all()
    assert (mixed[index[value == S.FINER]] >> 4 < B.VOXEL_OFFSET).all()
    # one level-1 leaf over a whole octant of the depth-8 grid: every brick settles on its first word
    one = one_leaf_root()
    octant = check_box(pkg, render, one, 8, (120, 0, 120), (16, 9, 16), "one level-1 leaf, depth 8")
    assert (octant[8:, :, 8:] == 0xABCDEF).all() and (octant != 0).sum() == 8 * 9 * 8


def test_boxes(pkg, render, tree7):
    words, whole = tree7["words"], tree7["whole"][0].reshape(128, 128, 128)
    first = True
    for name, (origin, size) in BOXES.items():
        want = whole[tuple(slice(o, o + s) for o, s in zip(origin, size))]
        check_box(pkg, render, words, 7, origin, size, f"tree7, {name}", want, already=not first)
        first = False
    far = check_box(pkg, render, words, 7, (125, 121, 99), (3, 7, 29), "tree7, at the far faces", already=True)
    assert np.array_equal(far, whole[125:, 121:, 99:])
    # a size with a 0 succeeds and writes nothing
    for size in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        out = Out(render.gpu, 0, arrays=1)
        assert raw_dense(pkg, render.gpu, 7, words.size, (1, 2, 3), size, out) == 0, last_error(pkg, render.gpu)
        assert out.untouched_from(0)
        assert tuple(render.sample_dense((1, 2, 3), size, 7).shape) == size
    t = render.sample_dense((1, 2, 3), (5, 1, 9), 7)
    assert t.dtype.is_signed and t.dtype.itemsize == 4 and t.is_cuda and np.array_equal(t.cpu().numpy(), whole[1:6, 2:3, 3:12])


def test_round_trips(pkg, render):
    import torch
    rng = np.random.default_rng(16)
    grid = np.where(rng.random((16, 16, 16)) < 1 / 3, rng.integers(1, 1 << 32, (16, 16, 16)), 0)
    assert 0.25 < (grid != 0).mean() < 0.42
    render.build_nodes_dense(grid)
    got = render.sample_dense((0, 0, 0), (16, 16, 16), 4)
    assert tuple(got.shape) == (16, 16, 16) and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), grid & 0xFFFFFF)
    # an edit of 500 cells, a fifth of them removals: each cell then holds the last colour given for it
    cells = rng.integers(0, 16, (500, 3))
    colours = rng.integers(1, 1 << 24, 500)
    colours[::5] = 0
    render.edit_nodes(cells, 4, colours)
    last = {tuple(c): int(col) for c, col in zip(cells.tolist(), colours)}
    assert len(last) < 500
    want = np.array([last[tuple(c)] for c in cells.tolist()])
    assert np.array_equal(render.sample_voxels(cells, 4).cpu().numpy(), want) and (want == 0).sum() > 50
    after = grid & 0xFFFFFF
    after[cells[:, 0], cells[:, 1], cells[:, 2]] = want
    assert np.array_equal(render.sample_dense((0, 0, 0), (16, 16, 16), 4).cpu().numpy(), after)


def test_malformed_trees(pkg, render):
    whole5 = S.box_cells((0, 0, 0), (32, 32, 32))
    chain = np.array([[(1 << 21) - 1, 0, (1 << 21) - 1], [0, 0, 0]])
    broken = 0
    for name, words in malformed_cases().items():
        # the guard on the CPU first: sample_ref asserts that no word outside the tree is read and stops at `depth`
        want5 = S.sample(words, words.size, whole5, 5)
        deep = np.concatenate([whole5[::7] << 16, chain])
        want21 = S.sample(words, words.size, deep, 21)
        for depth, w in ((5, want5), (21, want21)):  # BROKEN is a bad pointer met above `depth`, and nothing else
            ptr = words[w[2]].astype(np.int64) >> 4
            bad = (ptr < B.VOXEL_OFFSET) & ((ptr % 8 != 0) | (ptr + 8 > words.size))
            assert np.array_equal(w[0] == S.BROKEN, bad & (w[1] < depth)), name
        broken += int((want5[0] == S.BROKEN).any())
        check_points(pkg, render, words, 5, whole5, f"{name}, depth 5", want5)
        check_points(pkg, render, words, 21, deep, f"{name}, depth 21", want21, already=True)
        check_box(pkg, render, words, 5, (0, 0, 0), (32, 32, 32), f"{name}, depth 5, dense", want5[0], already=True)
        check_box(pkg, render, words, 21, (5 << 16, 3 << 16, 9 << 16), (5, 9, 6), f"{name}, depth 21, dense", already=True)
    assert broken == 2  # the two pointer cases


def test_errors_enqueue_nothing(pkg, render, own_gpu, tree7):
    base = tree7["base"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    n = 100
    xyz = device_cells(own_gpu, tree7["cells"][:n])
    out = Out(own_gpu, n)
    size = base.size

    def refused(gpu, code, part, rc):
        return rc == code and part in last_error(pkg, gpu)

    pts = lambda *a, **kw: raw_sample(pkg, own_gpu, *a, **kw)  # noqa: E731
    box = lambda *a, **kw: raw_dense(pkg, own_gpu, *a, **kw)  # noqa: E731
    o, s = (1, 2, 3), (4, 5, 5)
    # 1. null params (before everything else that is wrong)
    assert refused(own_gpu, ERR_ARG, "null params", pts(0, 12, xyz, n, out, flags=1, params=False, give_xyz=False))
    assert refused(own_gpu, ERR_ARG, "null params", box(0, 12, o, s, out, flags=1, params=False, give_grid=False))
    # 2. flags (before the depth)
    for flags in (1, 1 << 31):
        assert refused(own_gpu, ERR_ARG, "flag", pts(0, size, xyz, n, out, flags=flags))
        assert refused(own_gpu, ERR_ARG, "flag", box(22, size, o, s, out, flags=flags))
    # 3. depth (before the arguments)
    for depth in (0, 22):
        assert refused(own_gpu, ERR_ARG, "depth", pts(depth, size, xyz, n, out, give_xyz=False))
        assert refused(own_gpu, ERR_ARG, "depth", box(depth, size, o, s, out, give_origin=False))
    # 4. the arguments (before the tree)
    assert refused(own_gpu, ERR_ARG, "xyz_dev", pts(7, 12, xyz, n, out, give_xyz=False))
    assert refused(own_gpu, ERR_ARG, "value_out_dev", pts(7, 12, xyz, n, out, give_value=False))
    assert refused(own_gpu, ERR_ARG, "2^31", pts(7, 12, xyz, 1 << 31, out))
    assert refused(own_gpu, ERR_ARG, "2^31", pts(7, size, xyz, (1 << 40) + 5, out))
    assert refused(own_gpu, ERR_ARG, "origin", box(7, 12, o, s, out, give_origin=False))
    assert refused(own_gpu, ERR_ARG, "size", box(7, 12, o, s, out, give_size=False))
    assert refused(own_gpu, ERR_ARG, "grid_out_dev", box(7, 12, o, s, out, give_grid=False))
    for origin, sz in (((120, 0, 0), (9, 1, 1)), ((0, 128, 0), (1, 1, 1)), ((0, 0, 0xFFFFFFFF), (1, 1, 2)), ((0, 0, 0), (1, 129, 1))):
        assert refused(own_gpu, ERR_ARG, "leaves the grid", box(7, 12, origin, sz, out))
    assert refused(own_gpu, ERR_ARG, "2^31 or more", box(21, 12, (0, 0, 0), (2048, 1024, 1024), out))
    # 6. n_words
    for bad in (0, 12, size + 4, CAPACITY + 8):
        assert refused(own_gpu, ERR_ARG, "n_words", pts(7, bad, xyz, n, out))
        assert refused(own_gpu, ERR_ARG, "n_words", box(7, bad, o, s, out))
        assert refused(own_gpu, ERR_ARG, "n_words", pts(7, bad, xyz, 0, out))  # (also with nothing to do)
    with pytest.raises(pkg.SvoError):
        render.sample_dense((120, 0, 0), (9, 1, 1), 7)
    with pytest.raises(pkg.SvoError):
        render.sample_voxels([[0, 0, 0]], 22)
    # n == 0 succeeds, with or without pointers, and writes nothing
    assert pts(7, size, xyz, 0, out) == 0 and pts(7, size, xyz, 0, out, give_xyz=False, give_value=False) == 0
    assert out.untouched_from(0)
    assert np.array_equal(render.read_nodes(base.size + PAD), before)
    # 5. no node buffer: behind the arguments, before n_words
    fresh = pkg.Gpu(0)
    try:
        assert refused(fresh, ERR_STATE, "svo_nodes_alloc", raw_sample(pkg, fresh, 7, 12, xyz, n, out))
        assert refused(fresh, ERR_STATE, "svo_nodes_alloc", raw_dense(pkg, fresh, 7, 12, o, s, out))
        assert refused(fresh, ERR_ARG, "xyz_dev", raw_sample(pkg, fresh, 7, 12, xyz, n, out, give_xyz=False))
        assert refused(fresh, ERR_ARG, "leaves the grid", raw_dense(pkg, fresh, 7, 12, (0, 0, 0), (129, 1, 1), out))
        with pytest.raises(pkg.SvoError):
            fresh.sample_timing()  # nothing sampled on it yet
    finally:
        fresh.close()
    assert out.untouched_from(0)


def test_an_edit_through_a_sharing_context_is_seen(pkg, render, own_gpu, tree7):
    import torch
    g2 = pkg.Gpu(0)
    try:
        base = tree7["base"]
        set_base(render, base, 8 * 4097 * 7)
        own_gpu.sync()
        r2 = pkg.Render.share_nodes(g2, render)
        b = tree7["b"]
        dev = torch.device("cuda", 0)
        c, col = torch.as_tensor(b[0], dtype=torch.int32, device=dev), torch.as_tensor(b[1] & 0xFFFFFF, dtype=torch.int32, device=dev)
        pick = np.random.default_rng(10).integers(0, len(tree7["cells"]), 20_000)
        cells = np.concatenate([tree7["cells"][pick], b[0]])
        torch.cuda.synchronize()
        # the edit is enqueued on the second context's stream; the samples on the first follow at once
        p = pkg._lib.EditParams()
        p.depth, p.n_words = 7, base.size
        n_words = C.c_uint64()
        assert pkg._lib.lib().svo_nodes_edit(g2._h, c.data_ptr(), col.data_ptr(), len(b[0]), C.byref(p), C.byref(n_words)) == 0
        render.node_length = n_words.value
        got = render.sample_voxels(cells, 7, with_levels=True, with_indices=True)
        grid = render.sample_dense(*WHOLE7, 7)
        g2.sync()
        assert n_words.value == tree7["words"].size
        want = S.sample(tree7["words"], tree7["words"].size, cells, 7)
        for t, w in zip(got, want):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), w)
        assert np.array_equal(grid.cpu().numpy().view(np.uint32).reshape(-1), tree7["whole"][0])
        del r2
    finally:
        g2.close()


def test_a_device_adaptive_state_is_no_obstacle(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg.Gpu(0)
    try:
        r, device = pkg.Render.from_world(g, (64, 64), monu9_world(pkg), 6, capacity=200_000)
        words = r.read_nodes()
        xyz, value, level = L.list_voxels(words, words.size, 21)
        depth = int(level.max())
        xyz = xyz >> (21 - depth)
        assert value.size > 100
        cells = np.concatenate([xyz, np.random.default_rng(11).integers(0, 1 << depth, (5000, 3))])
        want = S.sample(words, words.size, cells, depth)
        got = r.sample_voxels(cells, depth, with_levels=True, with_indices=True)
        for t, w in zip(got, want):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), w)
        assert np.array_equal(want[0][:value.size], value)
        ms = g.sample_timing()
        assert len(ms) == 2 and all(t >= 0 for t in ms) and ms[1] > 0 and ms == g.sample_timing()
        side = min(1 << depth, 32)
        grid = r.sample_dense((0, 0, 0), (side,) * 3, depth)
        assert np.array_equal(grid.cpu().numpy().view(np.uint32), S.sample_dense(words, words.size, (0, 0, 0), (side,) * 3, depth))
        ms = g.sample_timing()
        assert len(ms) == 2 and all(t >= 0 for t in ms) and ms[1] > 0
        # a refused call leaves the times
        out = Out(g, 8, arrays=1)
        assert raw_dense(pkg, g, depth, words.size, (0, 0, 0), ((1 << depth) + 1, 1, 1), out) == ERR_ARG
        assert raw_sample(pkg, g, 0, words.size, device_cells(g, cells[:8]), 8, out) == ERR_ARG
        assert ms == g.sample_timing() and out.untouched_from(0)
        assert np.array_equal(r.read_nodes(), words)
        del device
    finally:
        g.close()
