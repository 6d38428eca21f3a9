"""Structures scattered over a tree on the GPU (csrc/svo_structure.hip): the column tops, the sites and the
stamped voxel lists against their restatements (tests/structure_ref.py), bit for bit; nothing written behind the outputs,
nothing on any refusal, the node buffer never by the read-only calls; the same bytes on every run and for every layout
of a tree; an edit through a sharing context seen; a device adaptive state no obstacle; scatter_structures end to end
against edit_ref.edit."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import edit_ref as E
import list_ref as L
import sample_ref as S
import structure_ref as R
from pass_frame import SENTINEL, SLACK, SentinelOut, last_error, monu9_world, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, PAD, ROOT, poison, set_base
from test_list_host import full_root, mixed_levels, one_leaf_root
from test_sample_gpu import loaded
from test_structure_host import DEEP, ISLAND_SITES, ODD_RECT, island, small_trees, tree7_tops, tree_structure

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_CAP = -1, -3, -6


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


def device_i32(gpu, a):
    """an integer array's u32 / i32 bit patterns as an int32 device tensor"""
    import torch
    a = (np.asarray(a, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    t = torch.as_tensor(a.view(np.int32), device=torch.device("cuda", gpu.device)).contiguous()
    torch.cuda.current_stream(t.device).synchronize()
    return t


def ptr(t):
    return t.data_ptr() if t is not None else None


def raw_tops(pkg, gpu, depth, n_words, origin, size, out, y=None, flags=0, params=True, give_origin=True, give_size=True, give_top=True,
             give_value=True):
    p = pkg._lib.TopsParams()
    p.flags, p.depth, p.n_words = flags, depth, n_words
    p.y_lo, p.y_hi = y if y is not None else (0, 1 << min(depth, 31))
    rc = pkg._lib.lib().svo_nodes_column_tops(gpu._h, C.byref(p) if params else None, (C.c_uint32 * 2)(*origin) if give_origin else None,
                                              (C.c_uint32 * 2)(*size) if give_size else None, ptr(out.t[0]) if give_top else None,
                                              ptr(out.t[1]) if give_value else None)
    gpu.sync()
    return rc


def check_tops(pkg, render, words, depth, origin, size, what, want=None, already=False, y=None):
    """the tops of the rectangle on the GPU == the rule; nothing is written behind the columns; the node buffer, with its
    poison behind it, reads back unchanged.  Returns (top, value), shaped `size`."""
    n = size[0] * size[1]
    if want is None:
        want = R.column_tops(words, words.size, origin, size, depth, *(y or (0, None)))
    before = loaded(render, words, already)
    out = SentinelOut(render.gpu, [n + SLACK, n + SLACK])
    rc = raw_tops(pkg, render.gpu, depth, words.size, origin, size, out, y)
    assert rc == 0, f"{what}: status {rc}: {last_error(pkg, render.gpu)}"
    got = out.host()
    for g, w, name in zip(got, want, ("top", "value")):
        w = np.asarray(w).reshape(-1)
        bad = np.flatnonzero(g[:n] != w)
        assert not bad.size, f"{what}: {bad.size} columns differ in {name}, first at {bad[:3]}: got {g[bad[:3]]} want {w[bad[:3]]}"
    assert out.untouched_from(n), f"{what}: written behind the columns"
    assert np.array_equal(render.read_nodes(words.size + PAD), before), f"{what}: the node buffer was written"
    return tuple(g[:n].reshape(tuple(size)) for g in got)


def test_small_and_special_trees(pkg, render):
    for name, (words, depth) in small_trees().items():
        side = 1 << depth
        check_tops(pkg, render, words, depth, (0, 0), (side, side), name)
    for depth in (1, 5, 21):
        top, value = check_tops(pkg, render, ROOT, depth, ((1 << depth) - 2, 0), (2, 2), f"empty, depth {depth}",
                                want=(np.full((2, 2), R.TOP_NONE), np.zeros((2, 2))))
        assert (top == R.TOP_NONE).all() and (value == 0).all()
    top, value = check_tops(pkg, render, full_root(), 4, (0, 0), (16, 16), "full root")
    assert (top == 15).all() and (value != 0).all()
    top, value = check_tops(pkg, render, one_leaf_root(), 4, (0, 0), (16, 16), "one leaf")
    assert (top[8:, 8:] == 7).all() and (top != R.TOP_NONE).sum() == 64
    # one deep column at depth 21, the whole height (the skipping form: the rule over 2^21 cells a column is the same array)
    words = B.build([DEEP], 21, [0x00FF00])
    rect = ((DEEP[0] - 1, DEEP[2] - 1), (3, 3))
    top, value = check_tops(pkg, render, words, 21, *rect, "depth 21", want=R.column_tops_skipping(words, words.size, *rect, 21))
    assert top[1, 1] == DEEP[1] and value[1, 1] == 0x00FF00 and (top != R.TOP_NONE).sum() == 1
    check_tops(pkg, render, words, 21, *rect, "depth 21, a window of the height", already=True, y=(DEEP[1] - 2000, DEEP[1] + 1))
    check_tops(pkg, render, words, 21, *rect, "depth 21, a window above the voxel", already=True, y=(DEEP[1] + 1, DEEP[1] + 3000))
    # a value array is optional
    out = SentinelOut(render.gpu, [9 + SLACK, 9 + SLACK])
    assert raw_tops(pkg, render.gpu, 21, words.size, *rect, out, give_value=False) == 0, last_error(pkg, render.gpu)
    assert out.host()[0][4] == DEEP[1] and out.untouched_from(9) and (out.host()[1] == SENTINEL).all()


def test_edited_tree_every_layout_and_every_run(pkg, render):
    words, want = tree7_tops()
    whole = ((0, 0), (128, 128))
    put = check_tops(pkg, render, words, 7, *whole, "tree7, put order", want)
    again = check_tops(pkg, render, words, 7, *whole, "tree7, second run", want, already=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(put, again))
    origin, size = ODD_RECT
    window = tuple(slice(o, o + s) for o, s in zip(origin, size))
    check_tops(pkg, render, words, 7, origin, size, "tree7, a rectangle aligned to nothing", tuple(w[window] for w in want), already=True)
    check_tops(pkg, render, words, 7, (125, 99), (3, 29), "tree7, at the far faces", tuple(w[125:, 99:] for w in want), already=True)
    # random counter bits in every word: the same arrays
    counted = words | np.random.default_rng(6).integers(0, 16, words.size).astype(np.uint32)
    check_tops(pkg, render, counted, 7, *whole, "tree7 with counters", want)
    for prune in (False, True):
        set_base(render, words)
        n = render.compact_nodes(prune=prune)
        layout = render.read_nodes()
        assert n == layout.size and (n < words.size) == prune
        got = check_tops(pkg, render, layout, 7, *whole, f"tree7 compacted, prune {prune}", want)
        if not prune:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, put))
        else:  # wherever the top is a voxel (here: wherever there is one at all)
            holds = put[1] != 0
            assert np.array_equal(got[0][holds], put[0][holds]) and np.array_equal(got[1][holds], put[1][holds])
    # the public call: int32 tensors, TOP_NONE reads -1
    set_base(render, words)
    tops, values = render.column_tops(origin, size, 7, with_values=True)
    assert all(t.dtype.is_signed and t.dtype.itemsize == 4 and t.is_cuda and tuple(t.shape) == size for t in (tops, values))
    assert np.array_equal(tops.cpu().numpy().view(np.uint32), want[0][window]) and np.array_equal(values.cpu().numpy().view(np.uint32), want[1][window])
    assert (tops.cpu().numpy() == pkg.TOP_NONE).sum() == (want[0][window] == R.TOP_NONE).sum()
    alone = render.column_tops((3, 5), (9, 70), 7, y_range=(10, 50))
    assert np.array_equal(alone.cpu().numpy().view(np.uint32), R.column_tops(words, words.size, (3, 5), (9, 70), 7, 10, 50)[0])
    for size in ((0, 4), (4, 0), (0, 0)):  # a size with a 0 succeeds and writes nothing
        out = SentinelOut(render.gpu, [SLACK, SLACK])
        assert raw_tops(pkg, render.gpu, 7, words.size, (1, 2), size, out) == 0, last_error(pkg, render.gpu)
        assert out.untouched_from(0) and tuple(render.column_tops((1, 2), size, 7).shape) == size
    ms = render.gpu.structure_timing()
    assert len(ms) == 3 and all(t >= 0 for t in ms) and ms[2] > 0 and ms[1] == 0


def test_coarse_leaves_y_cuts_and_finer(pkg, render):
    words = B.build([[0, 1, 2]], 2, [0x445566])  # a level-2 leaf: y 8..15 of the depth-5 grid
    first = True
    for y in ((0, 32), (0, 12), (0, 9), (0, 8), (15, 32), (16, 32), (10, 13), (8, 16)):
        top, value = check_tops(pkg, render, words, 5, (0, 14), (9, 11), f"a level-2 leaf, y in {y}", already=not first, y=y)
        first = False
        want = min(y[1], 16) - 1 if y[0] < 16 and y[1] > 8 else R.TOP_NONE
        assert (top[:8, 2:10] == want).all() and (top[8:] == R.TOP_NONE).all()
    mixed = mixed_levels()
    check_tops(pkg, render, mixed, 6, (0, 0), (64, 64), "mixed levels, depth 6")
    check_tops(pkg, render, mixed, 8, (37, 61), (100, 77), "mixed levels, depth 8", already=True, y=(30, 201))
    top, value = check_tops(pkg, render, mixed, 4, (0, 0), (16, 16), "mixed levels, depth 4", already=True)
    assert (value == S.FINER).any() and ((value != 0) & (value < S.FINER)).any()
    tree7 = tree7_base()["words"]
    top, value = check_tops(pkg, render, tree7, 5, (0, 0), (32, 32), "a depth-7 tree asked at depth 5")
    assert (value == S.FINER).sum() > 100


def test_malformed_trees(pkg, render):
    broken = 0
    for name, words in malformed_cases().items():
        top, value = check_tops(pkg, render, words, 5, (0, 0), (32, 32), f"{name}, depth 5")
        broken += int((value == S.BROKEN).any())
        check_tops(pkg, render, words, 21, (5 << 16, 9 << 16), (4, 6), f"{name}, depth 21", already=True, y=((3 << 16) - 100, (3 << 16) + 100))
    assert broken == 2  # the two pointer cases


def test_tops_refusals_in_order_enqueue_nothing(pkg, render, own_gpu):
    base = tree7_base()["base"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    out = SentinelOut(own_gpu, [64 + SLACK, 64 + SLACK])
    size, o, s = base.size, (1, 2), (8, 8)

    def refused(gpu, code, part, rc):
        return rc == code and part in last_error(pkg, gpu)

    tops = lambda *a, **kw: raw_tops(pkg, own_gpu, *a, **kw)  # noqa: E731
    # 1. null params, 2. null outputs and rectangle (before everything else that is wrong)
    assert refused(own_gpu, ERR_ARG, "null params", tops(0, 12, o, s, out, flags=1, params=False, give_top=False))
    assert refused(own_gpu, ERR_ARG, "origin_xz", tops(0, 12, o, s, out, flags=1, give_origin=False, give_size=False))
    assert refused(own_gpu, ERR_ARG, "size_xz", tops(0, 12, o, s, out, flags=1, give_size=False, give_top=False))
    assert refused(own_gpu, ERR_ARG, "top_out_dev", tops(0, 12, o, s, out, flags=1, give_top=False))
    # 3. flags (before the depth), 4. depth (before the y range)
    for flags in (1, 1 << 31):
        assert refused(own_gpu, ERR_ARG, "flag", tops(22, size, o, s, out, flags=flags))
    for depth in (0, 22):
        assert refused(own_gpu, ERR_ARG, "depth", tops(depth, size, o, s, out, y=(5, 5)))
    # 5. the y range (before the rectangle)
    for y in ((5, 5), (6, 5), (0, 129), (128, 128)):
        assert refused(own_gpu, ERR_ARG, "y range", tops(7, 12, (120, 0), (9, 1), out, y=y))
    # 6. the rectangle, 7. its columns (before the tree)
    for origin, sz in (((120, 0), (9, 1)), ((0, 128), (1, 1)), ((0, 0xFFFFFFFF), (1, 2)), ((0, 0), (129, 1))):
        assert refused(own_gpu, ERR_ARG, "leaves the grid", tops(7, 12, origin, sz, out))
    assert refused(own_gpu, ERR_ARG, "2^31 or more", tops(21, 12, (0, 0), (1 << 16, 1 << 15), out))
    # 9. n_words
    for bad in (0, 12, size + 4, CAPACITY + 8):
        assert refused(own_gpu, ERR_ARG, "n_words", tops(7, bad, o, s, out))
        assert refused(own_gpu, ERR_ARG, "n_words", tops(7, bad, o, (0, 5), out))  # (also with nothing to do)
    with pytest.raises(pkg.SvoError):
        render.column_tops((120, 0), (9, 1), 7)
    with pytest.raises(pkg.SvoError):
        render.column_tops((0, 0), (1, 1), 7, y_range=(4, 4))
    assert out.untouched_from(0) and np.array_equal(render.read_nodes(base.size + PAD), before)
    # 8. no node buffer: behind the arguments, before n_words
    fresh = pkg.Gpu(0)
    try:
        assert refused(fresh, ERR_STATE, "svo_nodes_alloc", raw_tops(pkg, fresh, 7, 12, o, s, out))
        assert refused(fresh, ERR_ARG, "leaves the grid", raw_tops(pkg, fresh, 7, 12, (0, 0), (129, 1), out))
        with pytest.raises(pkg.SvoError):
            fresh.structure_timing()  # nothing ran on it yet
    finally:
        fresh.close()
    assert out.untouched_from(0)


def test_an_edit_through_a_sharing_context_is_seen(pkg, render, own_gpu):
    import torch
    t = tree7_base()
    words, want = tree7_tops()
    g2 = pkg.Gpu(0)
    try:
        set_base(render, t["base"], 8 * 4097 * 7)
        own_gpu.sync()
        r2 = pkg.Render.share_nodes(g2, render)
        b = t["b"]
        dev = torch.device("cuda", 0)
        c, col = torch.as_tensor(b[0], dtype=torch.int32, device=dev), torch.as_tensor(b[1] & 0xFFFFFF, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        # the edit is enqueued on the second context's stream; the tops on the first follow at once
        p = pkg._lib.EditParams()
        p.depth, p.n_words = 7, t["base"].size
        n_words = C.c_uint64()
        assert pkg._lib.lib().svo_nodes_edit(g2._h, c.data_ptr(), col.data_ptr(), len(b[0]), C.byref(p), C.byref(n_words)) == 0
        render.node_length = n_words.value
        tops, values = render.column_tops((0, 0), (128, 128), 7, with_values=True)
        g2.sync()
        assert n_words.value == words.size
        assert np.array_equal(tops.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(values.cpu().numpy().view(np.uint32), want[1])
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
        depth = int(L.list_voxels(words, words.size, 21)[2].max())
        side = 1 << depth
        want = R.column_tops_skipping(words, words.size, (0, 0), (side, side), depth)
        assert (want[0] != R.TOP_NONE).sum() > 100
        tops, values = r.column_tops((0, 0), (side, side), depth, with_values=True)
        assert np.array_equal(tops.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(values.cpu().numpy().view(np.uint32), want[1])
        ms = g.structure_timing()
        assert len(ms) == 3 and all(t >= 0 for t in ms) and ms[2] > 0 and ms == g.structure_timing()
        # a refused call leaves the times
        with pytest.raises(pkg.SvoError):
            r.column_tops((0, 0), (side + 1, 1), depth)
        assert ms == g.structure_timing() and np.array_equal(r.read_nodes(), words)
        del device
    finally:
        g.close()


# ---- sites ----

def raw_sites(pkg, gpu, tops, values, origin, size, out, one_in=1, seed=0, on_value=0, lift=1, flags=1, max_sites=0, params=True,
              give_n=True, give_origin=True, give_size=True):
    """(status, count); out: SentinelOut of (origins, rots), or None for a count query"""
    p = pkg._lib.SitesParams()
    p.flags, p.seed, p.one_in, p.on_value, p.lift, p.max_sites = flags, seed, one_in, on_value, lift, max_sites
    n = C.c_uint64(0xAAAA)
    rc = pkg._lib.lib().svo_structures_sites(gpu._h, C.byref(p) if params else None, ptr(tops), ptr(values),
                                             (C.c_uint32 * 2)(*origin) if give_origin else None, (C.c_uint32 * 2)(*size) if give_size else None,
                                             ptr(out.t[0]) if out else None, ptr(out.t[1]) if out else None, C.byref(n) if give_n else None)
    gpu.sync()
    return rc, n.value


def check_sites(pkg, gpu, tops, values, origin, what, **kw):
    """count query and fill == the restatement; nothing written behind the count; the same bytes twice"""
    want_o, want_r = R.sites(tops, values, origin, kw.get("one_in", 1), kw.get("seed", 0), kw.get("on_value", 0), kw.get("lift", 1), kw.get("flags", 1))
    n = len(want_o)
    t, v = device_i32(gpu, tops), device_i32(gpu, values) if values is not None else None
    rc, count = raw_sites(pkg, gpu, t, v, origin, tops.shape, None, **kw)
    assert (rc, count) == (0, n), f"{what}: count query: status {rc}, {count} sites, want {n}: {last_error(pkg, gpu)}"
    runs = []
    for _ in range(2):
        out = SentinelOut(gpu, [3 * (n + SLACK), n + SLACK])
        rc, count = raw_sites(pkg, gpu, t, v, origin, tops.shape, out, max_sites=n, **kw)
        assert (rc, count) == (0, n), f"{what}: status {rc}: {last_error(pkg, gpu)}"
        origins, rots = out.host()
        assert np.array_equal(origins[:3 * n].view(np.int32).reshape(-1, 3), want_o), f"{what}: origins"
        assert np.array_equal(rots[:n], want_r), f"{what}: rotations"
        assert (origins[3 * n:] == SENTINEL).all() and (rots[n:] == SENTINEL).all(), f"{what}: written behind the count"
        runs.append(origins.tobytes() + rots.tobytes())
    assert runs[0] == runs[1]
    return want_o, want_r


def test_sites(pkg, own_gpu):
    rng = np.random.default_rng(5)
    shape = (70, 131)  # 9 170 columns: three tiles, the last one partial
    tops = rng.integers(0, 100, shape).astype(np.uint32)
    tops[rng.random(shape) < 0.2] = R.TOP_NONE
    values = rng.integers(1, 4, shape).astype(np.uint32)
    values[rng.random(shape) < 0.1] = S.FINER
    values[0, 0] = S.BROKEN
    origin = (1000, 7)
    every, _ = check_sites(pkg, own_gpu, tops, values, origin, "one_in = 1", one_in=1)
    assert len(every) == int(((tops != R.TOP_NONE) & (values < 1 << 27)).sum())  # FINER and BROKEN columns are skipped
    picked, rots = check_sites(pkg, own_gpu, tops, values, origin, "one_in = 3, on_value", one_in=3, seed=9, on_value=2, lift=-4)
    assert 0 < len(picked) < len(every) / 3 and set(rots.tolist()) == {0, 1, 2, 3}
    _, rots = check_sites(pkg, own_gpu, tops, values, origin, "no rotation", one_in=2, seed=0xFFFFFFF0, lift=0, flags=0)
    assert (rots == 0).all()
    more, _ = check_sites(pkg, own_gpu, tops, None, origin, "no values", one_in=2, seed=5)
    assert len(more) > 0
    none = np.full(shape, R.TOP_NONE, dtype=np.uint32)
    assert len(check_sites(pkg, own_gpu, none, values, origin, "all NONE")[0]) == 0
    assert len(check_sites(pkg, own_gpu, tops[:1, :1], values[:1, :1], origin, "one column, BROKEN")[0]) == 0
    # SVO_ERR_CAP carries the exact count and writes nothing; refusals in order; an empty rectangle
    t, v = device_i32(own_gpu, tops), device_i32(own_gpu, values)
    out = SentinelOut(own_gpu, [3 * (len(every) + SLACK), len(every) + SLACK])
    rc, count = raw_sites(pkg, own_gpu, t, v, origin, shape, out, max_sites=len(every) - 1)
    assert rc == ERR_CAP and str(len(every)) in last_error(pkg, own_gpu) and count == 0xAAAA and out.untouched_from(0)

    def refused(part, **kw):
        rc, count = raw_sites(pkg, own_gpu, kw.pop("tops", t), kw.pop("values", v), kw.pop("origin", origin), kw.pop("size", shape), out, **kw)
        return rc == ERR_ARG and part in last_error(pkg, own_gpu) and count == 0xAAAA

    assert refused("null params", params=False, give_n=False)
    assert refused("n_out", give_n=False, flags=2)
    assert refused("flag", flags=2, one_in=0)
    assert refused("one_in", one_in=0, give_origin=False)
    assert refused("origin_xz", give_origin=False, give_size=False)
    assert refused("size_xz", give_size=False, tops=None)
    assert refused("2^31", size=(1 << 31, 1), tops=None)
    assert refused("2^31 or more", size=(1 << 16, 1 << 15), tops=None)
    assert refused("top_dev", tops=None, values=None, on_value=1)
    assert refused("value_dev", values=None, on_value=1)
    assert out.untouched_from(0)
    for size in ((0, 9), (9, 0)):
        assert raw_sites(pkg, own_gpu, None, None, origin, size, out) == (0, 0) and out.untouched_from(0)


@pytest.mark.parametrize("columns", (4095, 4096, 4097))
def test_sites_at_the_edges_of_a_scan_tile(pkg, own_gpu, columns):
    """the last thread of a tile, an exactly full tile, one column in a second tile: the shared tile kernels (svo_scan.h)"""
    tops = (np.arange(columns, dtype=np.uint32) * 7) % 90
    tops[::3] = R.TOP_NONE
    tops[[0, 15, 16, 4079, 4080, 4094, columns - 1]] = [5, 6, 7, 8, 9, 10, 11]  # the ends of the first and the last threads' runs
    every, _ = check_sites(pkg, own_gpu, tops.reshape(1, -1), None, (3, 9), f"{columns} columns along z")
    assert len(every) == int((tops != R.TOP_NONE).sum()) and every[-1].tolist() == [3, 12, 9 + columns - 1]
    values = np.where(np.arange(columns) % 5 == 0, S.FINER, 2).astype(np.uint32)
    picked, _ = check_sites(pkg, own_gpu, tops.reshape(-1, 1), values.reshape(-1, 1), (3, 9), f"{columns} columns along x", one_in=2, seed=columns)
    assert 0 < len(picked) < len(every)


def test_sites_over_more_tiles_than_the_top_scan_has_threads(pkg, own_gpu):
    """4 199 425 columns are 1 026 tiles: the one block that scans the tile sums takes more than one per thread"""
    shape = (1025, 4097)
    rng = np.random.default_rng(1025)
    tops = rng.integers(0, 1 << 20, shape).astype(np.uint32)
    tops[rng.random(shape) < 0.1] = R.TOP_NONE
    origins, rots = check_sites(pkg, own_gpu, tops, None, (11, 5), "1 026 tiles", one_in=7)
    assert len(origins) == 539_616 and set(rots.tolist()) == {0, 1, 2, 3}  # (the restatement's count for this seed)


# ---- stamp ----

def raw_stamp(pkg, gpu, offsets, colours, m, origins, rots, k, depth, out, max_voxels=0, flags=0, params=True, give_n=True):
    """(status, count); out: SentinelOut of (xyz, colour, placement or None), or None for a count query"""
    p = pkg._lib.StampParams()
    p.flags, p.depth, p.max_voxels = flags, depth, max_voxels
    n = C.c_uint64(0xAAAA)
    rc = pkg._lib.lib().svo_structures_stamp(gpu._h, C.byref(p) if params else None, ptr(offsets), ptr(colours), m, ptr(origins), ptr(rots), k,
                                             ptr(out.t[0]) if out else None, ptr(out.t[1]) if out else None, ptr(out.t[2]) if out else None,
                                             C.byref(n) if give_n else None)
    gpu.sync()
    return rc, n.value


def check_stamp(pkg, gpu, offsets, colours, origins, rots, depth, what, with_placement=True):
    """count query and fill == the restatement; nothing written behind the count; the same bytes twice"""
    want = R.stamp(offsets, colours, origins, rots, depth)
    n, m, k = len(want[1]), len(offsets), len(origins)
    dev = [device_i32(gpu, a) if a is not None and len(a) else None for a in (offsets, colours, origins, rots)]
    args = (dev[0], dev[1], m, dev[2], dev[3], k, depth)
    rc, count = raw_stamp(pkg, gpu, *args, None)
    assert (rc, count) == (0, n), f"{what}: count query: status {rc}, {count} entries, want {n}: {last_error(pkg, gpu)}"
    runs = []
    for _ in range(2):
        out = SentinelOut(gpu, [3 * (n + SLACK), n + SLACK, n + SLACK if with_placement else None])
        rc, count = raw_stamp(pkg, gpu, *args, out, max_voxels=n)
        assert (rc, count) == (0, n), f"{what}: status {rc}: {last_error(pkg, gpu)}"
        got = out.host()
        assert np.array_equal(got[0][:3 * n].reshape(-1, 3), want[0]), f"{what}: xyz"
        assert np.array_equal(got[1][:n], want[1]), f"{what}: colours"
        assert not with_placement or np.array_equal(got[2][:n], want[2]), f"{what}: placements"
        assert (got[0][3 * n:] == SENTINEL).all() and all((g[n:] == SENTINEL).all() for g in got[1:]), f"{what}: written behind the count"
        runs.append(b"".join(g.tobytes() for g in got))
    assert runs[0] == runs[1]
    return want


def test_stamp_small_clipped_and_rotated(pkg, render, own_gpu):
    one = check_stamp(pkg, own_gpu, [[0, 0, 0]], [0x123456], [[3, 4, 5]], None, 3, "m = 1, k = 1")
    assert one[0].tolist() == [[3, 4, 5]] and one[1].tolist() == [0x123456]
    offsets, _, colours = tree_structure()  # 187 voxels within x -4..5, y 0..13, z -4..4
    side = 1 << 5
    # clipped by each of the six faces, wholly outside, negative origins, every rotation
    origins = [[16, 10, 16], [-2, 10, 16], [side + 2, 10, 16], [16, -5, 16], [16, side - 4, 16], [16, 10, -1], [16, 10, side + 1],
               [-40, 10, 16], [16, 200, 16], [-3, -3, -3], [16, 10, 16], [17, 10, 16], [16, 10, 16]]
    rots = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 1, 2, 3]
    want = check_stamp(pkg, own_gpu, offsets, colours, origins, rots, 5, "tree.vox, clipped and turned")
    per = np.bincount(want[2], minlength=len(origins))
    assert per[0] == per[10] == per[12] == 187 and per[7] == per[8] == 0 and all(0 < per[i] < 187 for i in (1, 2, 3, 4, 5, 6, 9))
    assert not np.array_equal(want[0][want[2] == 0], want[0][want[2] == 10])  # (turned)
    check_stamp(pkg, own_gpu, offsets, colours, origins, None, 5, "tree.vox, no rotations, no placement output", with_placement=False)
    # depth 21: far corner, and the range's ends
    far = (1 << 21) - 1
    check_stamp(pkg, own_gpu, offsets, colours, [[far, far, far], [0, 0, 0], [-(1 << 22), 0, (1 << 22) - 1]], [1, 2, 3], 21, "depth 21")
    # the public call
    structure = pkg.Structure(offsets, np.ones(len(offsets)), colours)
    got = render.stamp_structures(structure, origins, 5, rots, with_placement=True)
    assert all(t.dtype.is_signed and t.dtype.itemsize == 4 and t.is_cuda for t in got) and tuple(got[0].shape) == (len(want[1]), 3)
    for t, w in zip(got, want):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), w)
    assert tuple(render.stamp_structures(structure, np.zeros((0, 3), dtype=np.int64), 5)[0].shape) == (0, 3)


def test_stamp_tree_at_the_island_sites_and_a_scan_tile(pkg, own_gpu):
    offsets, _, colours = tree_structure()
    _, _, words, h, mask = island()
    top, value = R.column_tops_skipping(words, words.size, (0, 0), (128, 128), 7)
    origins, rots = R.sites(top, value, (0, 0), 64, seed=5)
    assert len(origins) == ISLAND_SITES
    want = check_stamp(pkg, own_gpu, offsets, colours, origins, rots, 7, "tree.vox at 163 sites")  # 30 481 entries: 8 tiles, 187 no multiple of 64
    assert len(want[1]) == ISLAND_SITES * 187  # (the island keeps every tree inside the grid)
    # a structure of 4 097 voxels: one past a scan tile, per placement
    rng = np.random.default_rng(4097)
    big = rng.integers(-20, 21, (4097, 3))
    want = check_stamp(pkg, own_gpu, big, rng.integers(0, 1 << 24, 4097), [[30, 30, 30], [5, 60, 1], [64, 64, 64]], [0, 3, 2], 6, "4 097 voxels")
    assert 4097 < len(want[1]) < 3 * 4097


def test_stamp_refusals(pkg, render, own_gpu):
    offsets, _, colours = tree_structure()
    m = len(offsets)
    origins = np.array([[5, 5, 5]] * 9)
    rots = np.zeros(9, dtype=np.int64)
    dev = lambda a: device_i32(own_gpu, a)  # noqa: E731
    o, c, g, r = dev(offsets), dev(colours), dev(origins), dev(rots)
    n = len(R.stamp(offsets, colours, origins, rots, 5)[1])
    out = SentinelOut(own_gpu, [3 * (n + SLACK), n + SLACK, n + SLACK])

    def refused(code, part, rc_count):
        return rc_count[0] == code and part in last_error(pkg, own_gpu) and rc_count[1] == 0xAAAA

    stamp = lambda *a, **kw: raw_stamp(pkg, own_gpu, *a, **kw)  # noqa: E731
    assert refused(ERR_ARG, "null params", stamp(o, c, m, g, r, 9, 0, out, flags=1, params=False, give_n=False))
    assert refused(ERR_ARG, "n_out", stamp(o, c, m, g, r, 9, 0, out, flags=1, give_n=False))
    assert refused(ERR_ARG, "flag", stamp(o, c, m, g, r, 9, 0, out, flags=1))
    for depth in (0, 22):
        assert refused(ERR_ARG, "depth", stamp(None, c, m, g, r, 1 << 31, depth, out))
    # k * m >= 2^31, decided on the host in 64 bits before any launch (the pointers are never followed)
    assert refused(ERR_ARG, "2^31", stamp(None, c, 1 << 16, g, r, 1 << 15, 5, out))
    assert refused(ERR_ARG, "2^31", stamp(o, c, 1 << 33, g, r, 1 << 31, 5, out))
    assert refused(ERR_ARG, "offsets_dev", stamp(None, None, m, None, r, 9, 5, out))
    assert refused(ERR_ARG, "colours_dev", stamp(o, None, m, None, r, 9, 5, out))
    assert refused(ERR_ARG, "origins_dev", stamp(o, c, m, None, r, 9, 5, out))
    no_colour = SentinelOut(own_gpu, [8, None, 8])
    assert refused(ERR_ARG, "colour_out_dev", stamp(o, c, m, g, r, 9, 5, no_colour))
    # checked on the device, the lowest index named: origins, then rotations, then offsets
    bad_origins, bad_rots, bad_offsets = origins.copy(), rots.copy(), offsets.copy()
    bad_origins[4, 1], bad_origins[7, 0] = 1 << 22, -(1 << 22) - 1
    bad_rots[3], bad_rots[8] = 4, 0xFFFFFFFF
    bad_offsets[100, 2], bad_offsets[150, 0] = -(1 << 22), 1 << 22
    assert refused(ERR_ARG, "placement 4 has an origin", stamp(dev(bad_offsets), c, m, dev(bad_origins), dev(bad_rots), 9, 5, out, max_voxels=n))
    assert refused(ERR_ARG, "placement 3 has a rotation", stamp(dev(bad_offsets), c, m, g, dev(bad_rots), 9, 5, out, max_voxels=n))
    assert refused(ERR_ARG, "voxel 100 has an offset", stamp(dev(bad_offsets), c, m, g, r, 9, 5, None))
    # SVO_ERR_CAP carries the exact count; a count query ignores max_voxels
    assert refused(ERR_CAP, str(n), stamp(o, c, m, g, r, 9, 5, out, max_voxels=n - 1))
    assert stamp(o, c, m, g, r, 9, 5, None, max_voxels=0) == (0, n)
    assert out.untouched_from(0)
    # nothing to do
    assert stamp(o, c, m, None, None, 0, 5, out) == (0, 0) and stamp(None, None, 0, g, r, 9, 5, out) == (0, 0) and out.untouched_from(0)
    with pytest.raises(pkg.SvoError):
        render.stamp_structures(pkg.Structure(offsets, np.ones(m), colours), origins, 5, rots + 4)


# ---- end to end ----

def test_scatter_on_the_island_equals_the_sequential_edit(pkg, render):
    offsets, index, colours = tree_structure()
    structure = pkg.Structure(offsets, index, colours)
    coords, island_colours, base, h, mask = island()
    top, value = R.column_tops_skipping(base, base.size, (0, 0), (128, 128), 7)
    want_sites = R.sites(top, value, (0, 0), 64, seed=5)
    xyz, colour, _ = R.stamp(offsets, colours, *want_sites, 7)
    want = E.edit(base, base.size, xyz, 7, colour)
    runs = []
    for run in range(2):
        growth = want.size - base.size
        set_base(render, base, growth)
        origins, rots = render.scatter_structures(structure, (0, 0), (128, 128), 64, seed=5, depth=7)
        assert np.array_equal(origins.cpu().numpy(), want_sites[0]) and np.array_equal(rots.cpu().numpy().view(np.uint32), want_sites[1])
        assert len(origins) == ISLAND_SITES and render.node_length == want.size
        got = render.read_nodes(want.size + PAD)
        bad = np.flatnonzero(got[:want.size] != want)
        assert not bad.size, f"run {run}: {bad.size} words differ, first at {bad[:5]}"
        assert np.array_equal(got[want.size:], poison(growth + PAD)[growth:]), "words behind the new length were written"
        runs.append(got.tobytes())
    assert runs[0] == runs[1]
    # the trees stand on the ground: every site's foot is one above its column's top
    assert np.array_equal(want_sites[0][:, 1], h[want_sites[0][:, 0], want_sites[0][:, 2]] + 1)
    # a tree built from the ground up by from_voxels gives the same tops
    fresh = pkg.Gpu(0)
    try:
        r2 = pkg.Render.from_voxels(fresh, (8, 8), coords, 7, island_colours, capacity=1 << 20)
        assert r2.node_length == base.size
        assert np.array_equal(r2.column_tops((0, 0), (128, 128), 7).cpu().numpy().view(np.uint32), top)
        del r2
    finally:
        fresh.close()


def test_a_later_placement_wins_and_colour_0_removes(pkg, render):
    base = island()[2]
    cube = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)])
    solid = pkg.Structure(cube, np.ones(27), np.full(27, 0x111111))
    set_base(render, base, 8 * 27 * 2 * 7)
    n = render.place_structures(solid, [[60, 50, 60], [61, 51, 61]], 7, [0, 0])
    # the second placement's colours differ by placement through a second structure: put it over the first
    other = pkg.Structure(cube, np.ones(27), np.full(27, 0x222222))
    n = render.place_structures(other, [[61, 51, 61]], 7)
    assert n == render.node_length
    shared, first_only = [[61, 51, 61], [62, 52, 62]], [[60, 50, 60], [60, 52, 62]]
    assert render.sample_voxels(shared, 7).tolist() == [0x222222] * 2 and render.sample_voxels(first_only, 7).tolist() == [0x111111] * 2
    # within one call: placement 1 over placement 0, by the list's order
    both_colours = pkg.Structure(np.concatenate([cube, cube + [1, 1, 1]]), np.ones(54), np.concatenate([np.full(27, 0x333333), np.full(27, 0x444444)]))
    render.place_structures(both_colours, [[90, 50, 60]], 7)
    assert render.sample_voxels([[90, 50, 60], [91, 51, 61], [93, 53, 63]], 7).tolist() == [0x333333, 0x444444, 0x444444]
    words = render.read_nodes()
    xyz, colour, _ = R.stamp(cube, np.full(27, 0x555555), [[70, 50, 60], [71, 51, 61]], None, 7)
    want = E.edit(words, words.size, xyz, 7, np.where(np.arange(54) < 27, 0x555555, 0x666666))
    two = pkg.Structure(cube, np.ones(27), np.full(27, 0x555555))
    coords, colours, placement = render.stamp_structures(two, [[70, 50, 60], [71, 51, 61]], 7, with_placement=True)
    colours = colours + placement * 0x111111  # 0x555555, 0x666666
    render.edit_nodes(coords, 7, colours)
    assert np.array_equal(render.read_nodes(), want)
    assert render.sample_voxels([[71, 51, 61], [70, 50, 60]], 7).tolist() == [0x666666, 0x555555]
    # a colour-0 structure voxel removes the cell there: a hole punched into the first cube, the top of its column moves
    before = int(render.column_tops((60, 60), (1, 1), 7)[0, 0])
    hole = pkg.Structure([[0, 0, 0], [0, -1, 0]], [1, 1], [0, 0])
    render.place_structures(hole, [[60, before, 60]], 7)
    assert render.sample_voxels([[60, before, 60], [60, before - 1, 60], [60, before - 2, 60]], 7).tolist()[:2] == [0, 0]
    assert int(render.column_tops((60, 60), (1, 1), 7)[0, 0]) == before - 2
