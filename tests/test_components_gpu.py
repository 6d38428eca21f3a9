"""The connected components labelled on the GPU (csrc/svo_components.hip): labels, ids and indices byte for
byte against the sequential restatement (tests/components_ref.py), with and without SAME_VALUE, on the smallest trees,
depth-21 pairs whose carry crosses every level, the mixed-level tree, the edited depth-7 tree with counter bits, a
checkerboard, the percolation tree in three layouts, an induced path of 65 535 cells, whose rounds are bounded, and a line
whose chain of parents needs several compress passes; the count
query agrees with the fill, nothing is written behind n, on any error or to the node buffer; the lossless merge keeps the
partition of the cells; svo_nodes_scatter_device; drop_floating against its restatement on a grid."""
import ctypes as C
import math

import numpy as np
import pytest

import build_ref as B
import components_ref as R
import list_ref as L
from pass_frame import SLACK, SentinelOut, last_error, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases
from test_components_host import check_labelling, checkerboard, merged, pair21, path6, percolation, serpentine
from test_edit_gpu import CAPACITY, PAD, ROOT, frame, poison, set_base
from test_list_host import full_root, mixed_levels

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_CAP = -1, -3, -6
SAME = R.SAME_VALUE
NAMES = ("label", "id", "index")
N0, C0 = 12345, 54321  # what *n_out and *n_components_out hold before a call


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


class Out(SentinelOut):
    """sentinel-filled device outputs of `room` entries"""

    def __init__(self, gpu, room):
        super().__init__(gpu, [room, room, room])
        self.label, self.id, self.index = self.t
        self.room = room


def raw_label(pkg, gpu, flags, depth, n_words, out=None, max_entries=None, params=True, n_out=True, n_comp=True, ids=True, index=True):
    p = pkg._lib.ComponentsParams()
    p.flags, p.depth, p.n_words = flags, depth, n_words
    p.max_entries = (out.room if out is not None else 0) if max_entries is None else max_entries
    n, c = C.c_uint64(N0), C.c_uint64(C0)
    ptr = lambda t, given=True: t.data_ptr() if out is not None and given else None  # noqa: E731
    rc = pkg._lib.lib().svo_nodes_label_components(
        gpu._h, C.byref(p) if params else None, ptr(out and out.label), ptr(out and out.id, ids), ptr(out and out.index, index),
        C.byref(n) if n_out else None, C.byref(c) if n_comp else None)
    gpu.sync()
    return rc, n.value, c.value


def check_components(pkg, render, words, depth, what, loaded=False, flags=(0, SAME), refs=None):
    """labels, ids and indices of the words' components on the GPU == the reference, for each flag; the count query agrees
    and writes nothing; nothing is written behind n; the node buffer reads back unchanged.  refs: {flag: labels()' result},
    when the caller has it.  Returns {flag: (label, id, index, n_components)}."""
    if not loaded:
        set_base(render, words)
    before = render.read_nodes(words.size + PAD)
    assert np.array_equal(before[:words.size], words)
    got = {}
    for flag in flags:
        label, ids, n_comp, index = refs[flag] if refs else R.labels(words, words.size, depth, bool(flag))
        name = f"{what}, flags {flag}"
        rc, n, c = raw_label(pkg, render.gpu, flag, depth, words.size)
        assert rc == 0, f"{name}: count query: status {rc}: {last_error(pkg, render.gpu)}"
        assert (n, c) == (label.size, n_comp), f"{name}: counts {(n, c)}, want {(label.size, n_comp)}"
        out = Out(render.gpu, n + SLACK)
        rc, m, k = raw_label(pkg, render.gpu, flag, depth, words.size, out)
        assert rc == 0, f"{name}: status {rc}: {last_error(pkg, render.gpu)}"
        assert (m, k) == (n, c), f"{name}: the fill's counts {(m, k)}, the count query's {(n, c)}"
        host = out.host()
        for g, w, field in zip(host, (label, ids, index), NAMES):
            if not np.array_equal(g[:n], w):
                bad = np.flatnonzero(g[:n] != w)
                raise AssertionError(f"{name}: {bad.size} entries differ in {field}, first at {bad[:3]}: got {g[bad[:3]]} want {w[bad[:3]]}")
        assert out.untouched_from(n), f"{name}: written behind n"
        check_labelling(host[0][:n], host[1][:n], c, name)
        got[flag] = tuple(g[:n] for g in host) + (c,)
    assert np.array_equal(render.read_nodes(words.size + PAD), before), f"{what}: the node buffer was written"
    return got


def test_smallest_trees(pkg, render):
    for depth in (1, 21):
        got = check_components(pkg, render, ROOT, depth, f"empty root, depth {depth}")
        assert all(g[0].size == 0 and g[3] == 0 for g in got.values())
        got = check_components(pkg, render, full_root(), depth, f"full root, depth {depth}")
        assert got[0][3] == 1 and not got[0][0].any() and got[SAME][3] == 8 and got[SAME][0].tolist() == list(range(8))
    # the optional outputs may be missing
    set_base(render, full_root())
    out = Out(render.gpu, 8 + SLACK)
    assert raw_label(pkg, render.gpu, 0, 3, 8, out, ids=False, index=False) == (0, 8, 1)
    label, ids, index = out.host()
    assert not label[:8].any() and (ids == ids[-1]).all() and (index == index[-1]).all() and out.untouched_from(8)


def test_depth_21_pairs(pkg, render):
    for axis in range(3):
        got = check_components(pkg, render, pair21(axis), 21, f"depth 21 pair along axis {axis}")
        assert got[0][0].tolist() == [0, 0] and got[0][3] == 1 and got[SAME][3] == 2
        got = check_components(pkg, render, pair21(axis, 1), 21, f"depth 21 pair along axis {axis}, sharing an edge", flags=(0,))
        assert got[0][0].tolist() == [0, 1] and got[0][3] == 2


def test_mixed_levels(pkg, render):
    mixed = mixed_levels()
    got = check_components(pkg, render, mixed, 6, "mixed levels")
    assert 1 < got[0][3] < got[SAME][3]
    again = check_components(pkg, render, mixed, 8, "mixed levels on the depth-8 grid", flags=(0,))
    assert all(np.array_equal(a, b) for a, b in zip(got[0][:3], again[0][:3]))


def test_edited_tree_in_put_order_with_counter_bits(pkg, render):
    words = tree7_base()["words"]
    counted = words | np.random.default_rng(6).integers(0, 16, words.size).astype(np.uint32)
    got = check_components(pkg, render, counted, 7, "edited depth 7 with counters")
    assert got[0][3] > 1000


def test_checkerboard_has_the_most_roots(pkg, render):
    got = check_components(pkg, render, checkerboard(), 4, "checkerboard")
    assert got[0][3] == 2048 and np.array_equal(got[0][1], np.arange(2048))


def test_every_layout_and_every_run_label_identically(pkg, render):
    coords, colours, canonical = percolation()
    refs = {flag: R.labels(canonical, canonical.size, 5, bool(flag)) for flag in (0, SAME)}
    assert refs[0][2] == 1908
    same = lambda a, b: all(x.tobytes() == y.tobytes() for flag in (0, SAME) for x, y in zip(a[flag][:2], b[flag][:2]))  # noqa: E731
    first = check_components(pkg, render, canonical, 5, "percolation, canonical", refs=refs)
    assert same(first, check_components(pkg, render, canonical, 5, "percolation, second run", loaded=True, refs=refs))
    # put order: the voxels edited into an empty root; the indices are that layout's own
    set_base(render, ROOT, growth=2 * canonical.size)
    order = np.random.default_rng(5).permutation(len(coords))
    for part in np.array_split(order, 3):
        render.edit_nodes(coords[part], 5, colours[part])
    put = render.read_nodes()
    assert put.size >= canonical.size and not np.array_equal(put[:canonical.size], canonical)
    assert same(first, check_components(pkg, render, put, 5, "percolation, put order", loaded=True))
    render.compact_nodes()
    assert same(first, check_components(pkg, render, render.read_nodes(), 5, "percolation, compacted", loaded=True))


def test_a_path_needs_few_rounds(pkg, render, own_gpu):
    words = path6()
    one = {flag: R.labels(words, words.size, 6, bool(flag)) for flag in (0, SAME)}
    got = check_components(pkg, render, words, 6, "path", refs=one)
    n = got[0][0].size
    assert n == 65535 and got[0][3] == 1 and got[SAME][3] == n  # (consecutive cells differ in colour)
    raw_label(pkg, own_gpu, 0, 6, words.size)
    ms, rounds = own_gpu.components_timing()
    # a condition, not a measurement: label propagation would need tens of thousands of rounds
    assert 1 <= rounds <= 2 + math.ceil(math.log2(n)), f"{rounds} rounds"
    assert len(ms) == 6 and all(t >= 0 for t in ms) and all(t > 0 for t in ms[:4]) and ms[5] > 0
    assert (ms, rounds) == own_gpu.components_timing()
    assert raw_label(pkg, own_gpu, 0, 3, words.size)[0] == ERR_ARG  # a refused call leaves the times
    assert (ms, rounds) == own_gpu.components_timing()

    # two such paths at depth 7 that never touch: the second is the first moved into the octant x >= 64, so its entries
    # follow the first's in the listing and are labelled like them
    cells = serpentine()
    colours = 1 + (np.arange(len(cells)) % 5)
    two = B.build(np.concatenate([cells, cells + [64, 0, 0]]), 7, np.concatenate([colours, colours]))
    index = R.walk(two.astype(np.int64), L.list_voxels(two, two.size, 7)[0], np.full(2 * n, 7)).astype(np.uint32)
    refs = {flag: (np.concatenate([label, label + n]), np.concatenate([ids, ids + c]), 2 * c, index) for flag, (label, ids, c, _) in one.items()}
    got = check_components(pkg, render, two, 7, "two paths", refs=refs)
    assert got[0][3] == 2 and got[0][0][n] == n
    assert own_gpu.components_timing()[1] <= 2 + math.ceil(math.log2(2 * n))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_long_line_needs_more_than_one_compress_pass(pkg, render, axis):
    """along a straight line the ranks ascend, so the first hook leaves every voxel under its predecessor: a chain of 999
    parents, far more than one compress pass chases (64)"""
    cells = np.full((1000, 3), 300, dtype=np.int64)
    cells[:, axis] = np.arange(12, 1012)
    words = B.build(cells, 10, 1 + (np.arange(1000) >= 500))
    got = check_components(pkg, render, words, 10, f"a line along axis {axis}")
    assert got[0][3] == 1 and not got[0][0].any() and got[SAME][3] == 2 and got[SAME][0][500] == 500


def first_cell_keys(words, depth, label):
    """per cell of the `depth` grid the Morton key of the first cell of its component, -1 where the cell is empty"""
    xyz = L.list_voxels(words, words.size, depth)[0]
    keys = B.morton(xyz, depth).astype(np.int64)[label]
    cells = R.entry_grid(words, words.size, depth)[0]
    return np.where(cells >= 0, keys[np.maximum(cells, 0)], -1)


@pytest.mark.parametrize("name", ["ball", "percolation"])
def test_the_lossless_merge_keeps_the_partition_of_the_cells(pkg, render, name):
    words, _, depth = merged(name)
    set_base(render, words)
    before = first_cell_keys(words, depth, render.label_components(depth)[0].cpu().numpy())
    render.simplify_nodes()
    small = render.read_nodes()
    labels, ids, n = render.label_components(depth)
    levels = L.list_voxels(small, small.size, depth)[2]
    assert small.size < words.size and (levels < depth).any() and labels.shape == levels.shape
    assert np.array_equal(first_cell_keys(small, depth, labels.cpu().numpy()), before)
    assert n == R.labels(words, words.size, depth)[2]


def test_errors_write_nothing(pkg, render, own_gpu):
    base = tree7_base()["base"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    count = R.labels(base, base.size, 7)[0].size
    out = Out(own_gpu, count + SLACK)
    refused = lambda code, part, *a, **kw: (raw_label(pkg, own_gpu, *a, **kw) == (code, N0, C0)  # noqa: E731
                                            and part in last_error(pkg, own_gpu))
    # the contract's order: each call has every later cause too
    assert refused(ERR_ARG, "null params", 8, 0, 12, out, params=False)
    assert refused(ERR_ARG, "null n_out", 8, 0, 12, out, n_out=False)
    assert refused(ERR_ARG, "null n_out", 8, 0, 12, out, n_comp=False)
    assert refused(ERR_ARG, "unknown flag bits", 8, 0, 12, out)
    assert refused(ERR_ARG, "unknown flag bits", 2, 7, base.size, out)
    assert refused(ERR_ARG, "unknown flag bits", 1 << 31, 7, base.size, out)
    for depth in (0, 22):
        assert refused(ERR_ARG, "depth", 0, depth, 12, out)
    for n in (0, 12, base.size + 4, CAPACITY + 8):
        assert refused(ERR_ARG, "n_words", 0, 6, n, out)
    # the tree is deeper than depth
    for flags in (0, SAME):
        assert refused(ERR_ARG, "level 7", flags, 6, base.size, out, max_entries=0)
        assert refused(ERR_ARG, "level 7", flags, 6, base.size)
    with pytest.raises(pkg.SvoError):
        render.label_components(3)
    with pytest.raises(pkg.SvoError):
        render.drop_floating(3)
    # room for one entry less than there are; a count query does not look at max_entries
    assert refused(ERR_CAP, f"{count} entries", 0, 7, base.size, out, max_entries=count - 1)
    assert raw_label(pkg, own_gpu, 0, 7, base.size, max_entries=0)[:2] == (0, count)
    assert out.untouched_from(0)
    assert np.array_equal(render.read_nodes(base.size + PAD), before)

    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice", "32 levels": "deeper than 31"}
    cases = malformed_cases()
    assert set(cases) == set(causes)
    for name, words in cases.items():
        set_base(render, words)
        before = render.read_nodes(words.size + PAD)
        for flags in (0, SAME):
            for o in (out, None):
                assert raw_label(pkg, own_gpu, flags, 21, words.size, o, max_entries=0) == (ERR_STATE, N0, C0), name
                assert "malformed tree: " in last_error(pkg, own_gpu) and causes[name] in last_error(pkg, own_gpu), f"{name}: {last_error(pkg, own_gpu)}"
        assert np.array_equal(render.read_nodes(words.size + PAD), before), name
    assert out.untouched_from(0)

    fresh = pkg.Gpu(0)
    try:
        assert raw_label(pkg, fresh, 0, 7, 12)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
        assert pkg._lib.lib().svo_nodes_scatter_device(fresh._h, None, None, 0, 0, 8) == ERR_STATE
    finally:
        fresh.close()


def test_python_outputs_and_sizes(pkg, render):
    import torch
    mixed = mixed_levels()
    set_base(render, mixed)
    label, ids, n, index = R.labels(mixed, mixed.size, 6)
    level = L.list_voxels(mixed, mixed.size, 6)[2].astype(np.int64)
    got = render.label_components(6, with_indices=True, with_sizes=True)
    assert [type(g) for g in got] == [torch.Tensor, torch.Tensor, int, torch.Tensor, torch.Tensor] and got[2] == n
    assert all(g.is_cuda for g in got if isinstance(g, torch.Tensor)) and got[4].dtype == torch.int64
    for g, w in zip((got[0], got[1], got[3]), (label, ids, index)):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy().view(np.uint32), w)
    want = np.bincount(ids, weights=8.0 ** (6 - level), minlength=n).astype(np.int64)
    assert np.array_equal(got[4].cpu().numpy(), want) and want.max() >= 8
    labels, none, n3 = render.label_components(6, same_value=True, with_ids=False)
    assert none is None and n3 == R.labels(mixed, mixed.size, 6, True)[2]
    set_base(render, ROOT)
    empty = render.label_components(4, with_indices=True, with_sizes=True)
    assert [tuple(t.shape) for t in (empty[0], empty[1], empty[3], empty[4])] == [(0,)] * 4 and empty[2] == 0
    assert render.drop_floating(4) == (0, 0, 0)


def raw_scatter(pkg, gpu, index, words, fill, n, n_words):
    return pkg._lib.lib().svo_nodes_scatter_device(gpu._h, index.data_ptr() if index is not None else None,
                                                   words.data_ptr() if words is not None else None, fill, n, n_words)


def test_scatter_nodes_device(pkg, render, own_gpu, O):
    import torch
    dev = torch.device("cuda", own_gpu.device)
    grid = np.zeros((16, 16, 16), dtype=np.int64)
    grid[2:14, 2:14, 2:14] = 0x30A0F0
    coords, colours = B.dense_to_voxels(grid)
    words = B.build(coords, 4, colours)
    set_base(render, words)
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    solid = frame(pkg, render, u)
    assert (solid["value"] < words.size).sum() > 300

    # half of the block is emptied; indices behind the tree and the sampler's 0xFFFFFFFF are skipped
    half = coords[coords[:, 0] >= 8]
    index = render.sample_voxels(half, 4, with_indices=True)[1]
    at = index.cpu().numpy()
    skipped = torch.tensor([words.size, words.size + 5, -1, CAPACITY - 1], dtype=torch.int32, device=dev)
    idx = torch.cat([index, skipped])
    new = torch.full((idx.numel(),), -(1 << 31), dtype=torch.int32, device=dev)  # (the empty word's bits)
    torch.cuda.current_stream(dev).synchronize()
    want = words.copy()
    want[at] = B.EMPTY
    assert raw_scatter(pkg, own_gpu, idx, new, 0, idx.numel(), words.size) == 0
    # a frame rendered right behind it sees the change, with no sync in between
    after = frame(pkg, render, u)
    got = render.read_nodes(words.size + PAD)
    assert np.array_equal(got[:words.size], want) and np.array_equal(got[words.size:], poison(PAD))
    seen = O.trace_frame(want, u, threads=4).reshape(-1)
    assert np.array_equal(after["value"], seen["value"]) and np.array_equal(after["t"].view(np.uint32), seen["t"].view(np.uint32))
    assert (after["t"].view(np.uint32) != solid["t"].view(np.uint32)).any()

    # the fill form, through the Python method; numpy indices are taken too
    red = (B.VOXEL_OFFSET + 0xFF0000) << 4
    render.scatter_nodes_device(at[:5], fill=red)
    want[at[:5]] = red
    assert np.array_equal(render.read_nodes(words.size), want)
    render.scatter_nodes_device(index[:3], words=torch.full((3,), 0x12345670, dtype=torch.int32, device=dev))
    want[at[:3]] = 0x12345670
    got = render.read_nodes(words.size + PAD)
    assert np.array_equal(got[:words.size], want) and np.array_equal(got[words.size:], poison(PAD))
    with pytest.raises(ValueError):
        render.scatter_nodes_device(index)
    with pytest.raises(ValueError):
        render.scatter_nodes_device(index, words=new[:2])

    # errors, decided on the host
    assert raw_scatter(pkg, own_gpu, None, None, 0, 3, words.size) == ERR_ARG and "null index_dev" in last_error(pkg, own_gpu)
    assert raw_scatter(pkg, own_gpu, idx, None, 0, 1 << 31, words.size) == ERR_ARG and "2^31" in last_error(pkg, own_gpu)
    for n_words in (0, 12, CAPACITY + 8):
        assert raw_scatter(pkg, own_gpu, idx, None, 0, 1, n_words) == ERR_ARG and "n_words" in last_error(pkg, own_gpu)
    assert raw_scatter(pkg, own_gpu, None, None, 0, 0, words.size) == 0
    own_gpu.sync()
    assert np.array_equal(render.read_nodes(words.size), want)


def test_drop_floating(pkg, render):
    box, ball = pkg.region.box, pkg.region.ball
    scene = [box((0, 0, 0), (32, 2, 64), 1),       # a floor slab
             box((10, 2, 10), (12, 20, 12), 2),    # a pillar on it
             box((4, 20, 4), (20, 22, 20), 3),     # carrying a platform
             ball((40, 40, 40), 6, 4),             # a floating ball
             box((48, 16, 16), (56, 24, 24), 5),   # a floating cube: one leaf of level 3
             box((32, 2, 30), (36, 6, 34), 6)]     # a block that touches the slab's top along the edge x = 32, y = 2 only
    whole = ((0, 0, 0), (64, 64, 64))
    for anchor, kept, dropped in ((None, {1, 2, 3}, 3), (((34, 34, 34), (47, 47, 47)), {4}, 3)):
        set_base(render, ROOT, growth=1 << 18)
        render.edit_region(scene, 6)
        words = render.read_nodes()
        before = render.sample_dense(*whole, 6).cpu().numpy().astype(np.int64)
        assert set(np.unique(before).tolist()) == {0, 1, 2, 3, 4, 5, 6}
        xyz, value, level = L.list_voxels(words, words.size, 6)
        assert level[value == 5].tolist() == [3]
        label, ids, n, index = R.labels(words, words.size, 6)
        behind = render.read_nodes(words.size + PAD)[words.size:]
        assert n == 4
        want, n_grid, dropped_grid = R.drop_floating(before, anchor)
        assert (n_grid, dropped_grid) == (n, dropped) and set(np.unique(want).tolist()) == kept | {0}
        gone = ~np.isin(value, list(kept))
        assert render.drop_floating(6, anchor) == (n, dropped, int(gone.sum()))
        assert np.array_equal(render.sample_dense(*whole, 6).cpu().numpy(), want)
        # the leaves of the dropped components hold the empty word, and no other word changed
        after = render.read_nodes(words.size + PAD)
        expect = words.copy()
        expect[index[gone]] = B.EMPTY
        assert np.array_equal(after[:words.size], expect) and np.array_equal(after[words.size:], behind)
        assert render.node_length == words.size
    # what it left empty is the compaction's to drop
    assert render.compact_nodes(prune=True) < words.size
    assert render.label_components(6)[2] == 1
