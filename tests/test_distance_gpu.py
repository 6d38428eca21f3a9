"""Distance fields of a device tree (csrc/svo_distance.hip): the squared distances and packed sites of
svo_nodes_distance against the rule read literally (tests/distance_ref.py: brute), byte for byte, in the three modes, on the
edited depth-7 tree (the whole grid, which takes two slabs, and small boxes at the origin, in the middle and flush with the
far corner), on every layout of it, on the empty and the full root, on mixed-level, coarse, finer and malformed trees, with
R = 127 and at depth 21; nothing written behind the outputs, nothing on any error, the node buffer never; an edit through a
sharing context seen; a device adaptive state no obstacle; the times; Render.morph_ball against its per-cell contract."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import distance_ref as D
import sample_ref as S
from conftest import assert_hits_equal
from pass_frame import SENTINEL, SLACK, SentinelOut, last_error, monu9_world, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases
from test_distance_host import BOXES7, R127_BOXES, r127_voxels
from test_edit_gpu import CAPACITY, PAD, ROOT, frame, set_base
from test_list_host import full_root, mixed_levels, one_leaf_root
from test_morph_host import scenes

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
MODES = (D.TO_VOXELS, D.TO_EMPTY, D.SIGNED)
SELF = 0x808080  # the packed site of a cell that is its own


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def tree7():
    """pass_frame.tree7_base with the rule's values of every cell of the 128^3 grid, computed once"""
    t = tree7_base()
    words = t["words"]
    return {**t, "grid": S.sample_dense(words, words.size, (0, 0, 0), (128,) * 3, 7)}


class Out(SentinelOut):
    """d2 and sites: sentinel-filled device outputs of `n` entries and SLACK more"""

    def __init__(self, gpu, n):
        super().__init__(gpu, [n + SLACK] * 2)
        self.n = n


def raw(pkg, gpu, depth, n_words, origin, size, R, mode, out, sites=True, flags=0, params=True, give_origin=True, give_size=True, give_d2=True):
    p = pkg._lib.DistanceParams()
    p.flags, p.mode, p.depth, p.max_distance, p.n_words = flags, mode, depth, R, n_words
    rc = pkg._lib.lib().svo_nodes_distance(gpu._h, C.byref(p) if params else None, (C.c_uint32 * 3)(*origin) if give_origin else None,
                                           (C.c_uint32 * 3)(*size) if give_size else None, out.t[0].data_ptr() if give_d2 else None,
                                           out.t[1].data_ptr() if sites else None)
    gpu.sync()
    return rc


def assert_same(got, want, what, name):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} entries differ in {name}, first at {bad[:3]}: got {got[bad[:3]]} want {want[bad[:3]]}")


def check(pkg, render, words, depth, origin, size, R, mode, what, want=None, load=True, sites=True):
    """the box's field on the GPU == the rule, byte for byte; the sentinels stand behind both outputs (in all of the sites'
    without `sites`); with `load` the words are written first and read back unchanged afterwards.  Returns (d2, sites)."""
    n = size[0] * size[1] * size[2]
    want = want if want is not None else D.brute(words, words.size, depth, origin, size, R, mode)
    if load:
        set_base(render, words)
        before = render.read_nodes(words.size + PAD)
    out = Out(render.gpu, n)
    rc = raw(pkg, render.gpu, depth, words.size, origin, size, R, mode, out, sites=sites)
    assert rc == 0, f"{what}: status {rc}: {last_error(pkg, render.gpu)}"
    d2, packed = out.host()
    assert_same(d2[:n], want[0].reshape(-1).view(np.uint32), what, "d2")
    if sites:
        assert_same(packed[:n], want[1].reshape(-1), what, "the sites")
    assert out.untouched_from(n) and (sites or (packed == SENTINEL).all()), f"{what}: written behind the box"
    if load:
        assert np.array_equal(render.read_nodes(words.size + PAD), before), f"{what}: the node buffer was written"
    return d2[:n].view(np.int32).reshape(tuple(size)), packed[:n].reshape(tuple(size))


def test_tree7_the_whole_grid_in_two_slabs(pkg, render, tree7):
    words, grid = tree7["words"], tree7["grid"]
    whole = ((0, 0, 0), (128, 128, 128))
    assert (128 + 2 * 3) * 128 * 128 > 1 << 21  # the y pass's output of the box exceeds a slab: two slabs
    first = True
    for mode in MODES:
        want = D.brute_grid(grid, *whole, 3, mode)
        d2, packed = check(pkg, render, words, 7, *whole, 3, mode, f"tree7, the whole grid, mode {mode}", want, load=first)
        first = False
        if mode == D.SIGNED:
            assert (d2 != 0).all() and ((d2 < 0) == (grid != 0)).all()
            check(pkg, render, words, 7, *whole, 3, mode, "tree7, the whole grid, signed, no sites", want, load=False, sites=False)
    # a second run gives the same bytes
    again = check(pkg, render, words, 7, *whole, 3, D.SIGNED, "tree7, second run", want, load=False)
    assert again[0].tobytes() == d2.tobytes() and again[1].tobytes() == packed.tobytes()


def test_tree7_boxes(pkg, render, tree7):
    words, grid = tree7["words"], tree7["grid"]
    set_base(render, words)
    before = render.read_nodes(words.size + PAD)
    for name, (origin, size) in BOXES7.items():
        for R in (1, 6):
            for mode in MODES:
                want = D.brute_grid(grid, origin, size, R, mode)
                for sites in (True, False):
                    check(pkg, render, words, 7, origin, size, R, mode, f"tree7, {name}, R {R}, mode {mode}, sites {sites}", want, load=False, sites=sites)
    assert np.array_equal(render.read_nodes(words.size + PAD), before)
    # a size with a 0 succeeds and writes nothing
    for size in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        out = Out(render.gpu, 0)
        assert raw(pkg, render.gpu, 7, words.size, (1, 2, 3), size, 4, 0, out) == 0, last_error(pkg, render.gpu)
        assert out.untouched_from(0)
        assert tuple(render.distance_dense((1, 2, 3), size, 4, 7).shape) == size
    # the public call: int32 device tensors, the helpers of distance.py over them
    origin, size = BOXES7["33x40x7, middle"]
    d2, sites = render.distance_dense(origin, size, 6, 7, with_sites=True)
    want = D.brute_grid(grid, origin, size, 6, D.TO_VOXELS)
    assert all(t.dtype.is_signed and t.dtype.itemsize == 4 and t.is_cuda and tuple(t.shape) == size for t in (d2, sites))
    assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(sites.cpu().numpy().view(np.uint32), want[1])
    cells, valid = pkg.distance.site_cells(sites, origin)
    assert np.array_equal(valid.cpu().numpy(), want[0] != D.FAR) and valid.any() and not valid.all()
    c = cells.cpu().numpy()[valid.cpu().numpy()]
    assert (grid[c[:, 0], c[:, 1], c[:, 2]] != 0).all()  # every site is a voxel
    assert np.array_equal(pkg.distance.within(d2, 3).cpu().numpy(), want[0] <= 9)
    signed = render.distance_dense(origin, size, 6, 7, mode="signed")
    assert np.array_equal(signed.cpu().numpy(), D.brute_grid(grid, origin, size, 6, D.SIGNED)[0])
    with pytest.raises(ValueError):
        render.distance_dense(origin, size, 6, 7, mode="nearest")


def test_every_layout_gives_the_same_bytes(pkg, render, tree7):
    words, grid = tree7["words"], tree7["grid"]
    origin, size, R = (3, 0, 50), (70, 128, 78), 4
    want = D.brute_grid(grid, origin, size, R, D.SIGNED)
    put = check(pkg, render, words, 7, origin, size, R, D.SIGNED, "put order", want)
    layouts = {"compacted": lambda: render.compact_nodes(prune=False), "pruned": lambda: render.compact_nodes(prune=True),
               "simplified": lambda: render.simplify_nodes()}
    for name, make in layouts.items():
        set_base(render, words)
        make()
        layout = render.read_nodes()
        got = check(pkg, render, layout, 7, origin, size, R, D.SIGNED, name, want)
        assert got[0].tobytes() == put[0].tobytes() and got[1].tobytes() == put[1].tobytes()


def test_the_empty_and_the_full_root(pkg, render):
    whole = ((0, 0, 0), (32, 32, 32))
    d2, packed = check(pkg, render, ROOT, 5, *whole, 4, D.TO_VOXELS, "empty root, to voxels")
    assert (d2 == D.FAR).all() and (packed == D.NO_SITE).all()
    d2, packed = check(pkg, render, ROOT, 5, *whole, 4, D.TO_EMPTY, "empty root, to empty", load=False)
    assert (d2 == 0).all() and (packed == SELF).all()
    assert (check(pkg, render, ROOT, 5, *whole, 4, D.SIGNED, "empty root, signed", load=False)[0] == D.FAR).all()
    full = full_root()
    d2, packed = check(pkg, render, full, 5, *whole, 4, D.TO_VOXELS, "full root, to voxels")
    assert (d2 == 0).all() and (packed == SELF).all()
    d2, packed = check(pkg, render, full, 5, *whole, 4, D.TO_EMPTY, "full root, to empty", load=False)
    edge = np.minimum(np.arange(32) + 1, 32 - np.arange(32))  # cells to the nearest cell outside, per axis
    near = np.minimum(np.minimum(edge[:, None, None], edge[None, :, None]), edge[None, None, :])
    assert np.array_equal(d2, np.where(near <= 4, near * near, D.FAR)) and (d2[0] == 1).all() and d2[16, 16, 16] == D.FAR
    assert packed[0, 5, 5] == D.pack((-1, 0, 0)) and packed[31, 31, 31] == D.pack((0, 0, 1)) and packed[5, 5, 31] == D.pack((0, 0, 1))
    d2 = check(pkg, render, full, 5, *whole, 4, D.SIGNED, "full root, signed", load=False)[0]
    assert np.array_equal(d2, -np.where(near <= 4, near * near, D.FAR))
    # depth 1: the grid is smaller than a word of the bit rows
    for mode in MODES:
        check(pkg, render, full, 1, (0, 0, 0), (2, 2, 2), 2, mode, f"full root, depth 1, mode {mode}", load=False)
    for mode in MODES:
        check(pkg, render, one_leaf_root(), 1, (0, 1, 0), (2, 1, 2), 1, mode, f"one leaf, depth 1, mode {mode}", load=mode == 0)


def test_mixed_levels_coarse_leaves_and_finer_cells(pkg, render):
    mixed = mixed_levels()
    first = True
    for mode in MODES:
        check(pkg, render, mixed, 6, (0, 0, 0), (64, 64, 64), 3, mode, f"mixed levels, depth 6, mode {mode}", load=first)
        first = False
        # leaves above the grid are occupied cell by cell: the depth-8 grid, a box that no word is aligned with
        check(pkg, render, mixed, 8, (37, 50, 61), (40, 28, 77), 5, mode, f"mixed levels, depth 8, mode {mode}", load=False)
        # the tree refined below the grid: FINER counts as occupied
        d2, _ = check(pkg, render, mixed, 4, (0, 0, 0), (16, 16, 16), 3, mode, f"mixed levels, depth 4, mode {mode}", load=False)
    coarse = S.sample_dense(mixed, mixed.size, (0, 0, 0), (16, 16, 16), 4)
    assert (coarse == S.FINER).any() and ((d2 < 0) == (coarse != 0)).all()
    one = one_leaf_root()
    for mode in MODES:
        d2, _ = check(pkg, render, one, 8, (120, 0, 120), (16, 9, 16), 4, mode, f"one level-1 leaf, depth 8, mode {mode}", load=mode == 0)
    assert (d2[8:, :, 8:] < 0).all() and (d2[:8] > 0).all()


def test_malformed_trees(pkg, render):
    broken = 0
    for name, words in malformed_cases().items():
        # the guard on the CPU first: sample_ref asserts that no word outside the tree is read and stops at `depth`
        whole5 = S.sample_dense(words, words.size, (0, 0, 0), (32, 32, 32), 5)
        broken += int((whole5 == S.BROKEN).any())
        for mode in MODES:
            want = D.brute_grid(whole5, (0, 0, 0), (32, 32, 32), 3, mode)
            check(pkg, render, words, 5, (0, 0, 0), (32, 32, 32), 3, mode, f"{name}, depth 5, mode {mode}", want, load=mode == 0)
        check(pkg, render, words, 21, (5 << 16, 3 << 16, 9 << 16), (5, 9, 6), 4, D.SIGNED, f"{name}, depth 21", load=False)
        top = (1 << 21) - 6
        check(pkg, render, words, 21, (top, 0, top), (6, 4, 6), 3, D.TO_VOXELS, f"{name}, depth 21, the chain's corner", load=False)
    assert broken == 2  # the two pointer cases


def test_radius_127(pkg, render):
    cells = r127_voxels()
    words = B.build(cells, 9, np.arange(1, len(cells) + 1))
    assert len(cells) <= 64
    first = True
    for origin, size in R127_BOXES:
        want = D.from_sites(cells, origin, size, 127)
        assert (want[0] == D.FAR).any() and (want[0] > 100 * 100).sum() > 100 and (want[0] != D.FAR).sum() > 1000
        check(pkg, render, words, 9, origin, size, 127, D.TO_VOXELS, f"R 127, {size}", want, load=first)
        first = False
    origin, size = R127_BOXES[1]
    assert (size[0] + 254) * size[1] * size[2] > 1 << 21  # more than one slab


def test_depth_21(pkg, render):
    top = 1 << 21
    for origin, voxel in (((top - 16,) * 3, (top - 3, top - 9, top - 1)), (((1 << 20) - 8,) * 3, (1 << 20, (1 << 20) - 1, (1 << 20) + 2))):
        set_base(render, ROOT, 8 * 21)
        render.edit_nodes([voxel], 21, [0x00FF00])
        words = render.read_nodes()
        assert words.size == 8 * 21
        for mode in MODES:
            d2, packed = check(pkg, render, words, 21, origin, (16, 16, 16), 5, mode, f"depth 21 at {origin[0]}, mode {mode}", load=mode == 0)
        at = tuple(v - o for v, o in zip(voxel, origin))
        assert d2[at] == -1 and (d2 < 0).sum() == 1 and d2[at[0] - 3, at[1], at[2]] == 9


def test_every_error_in_order_and_nothing_written(pkg, render, own_gpu, tree7):
    base = tree7["base"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    out = Out(own_gpu, 100)
    size = base.size
    o, s = (1, 2, 3), (4, 5, 5)

    def refused(gpu, code, part, rc):
        return rc == code and part in last_error(pkg, gpu)

    call = lambda *a, **kw: raw(pkg, own_gpu, *a, **kw)  # noqa: E731
    # null params before everything else that is wrong
    assert refused(own_gpu, ERR_ARG, "null params", call(0, 12, o, s, 0, 3, out, flags=1, params=False, give_d2=False))
    for flags in (1, 1 << 31):  # flags before the depth
        assert refused(own_gpu, ERR_ARG, "flag", call(22, size, o, s, 4, 0, out, flags=flags))
    for depth in (0, 22):  # depth before the mode
        assert refused(own_gpu, ERR_ARG, "depth", call(depth, size, o, s, 4, 3, out))
    for mode in (3, 0xFFFFFFFF):  # mode before the radius
        assert refused(own_gpu, ERR_ARG, "mode", call(7, size, o, s, 0, mode, out))
    for R in (0, 128, 0xFFFFFFFF):  # the radius before the pointers
        assert refused(own_gpu, ERR_ARG, "max_distance", call(7, size, o, s, R, 0, out, give_origin=False))
    assert refused(own_gpu, ERR_ARG, "origin", call(7, 12, o, s, 4, 0, out, give_origin=False, give_size=False))
    assert refused(own_gpu, ERR_ARG, "size", call(7, 12, o, s, 4, 0, out, give_size=False, give_d2=False))
    assert refused(own_gpu, ERR_ARG, "d2_out_dev", call(7, 12, (120, 0, 0), (9, 1, 1), 4, 0, out, give_d2=False))
    for origin, sz in (((120, 0, 0), (9, 1, 1)), ((0, 128, 0), (1, 1, 1)), ((0, 0, 0xFFFFFFFF), (1, 1, 2)), ((0, 0, 0), (1, 129, 1))):
        assert refused(own_gpu, ERR_ARG, "leaves the grid", call(7, 12, origin, sz, 4, 0, out))
    assert refused(own_gpu, ERR_ARG, "2^31 or more", call(21, 12, (0, 0, 0), (2048, 1024, 1024), 1, 0, out))
    # the workspace: 255 x 255 rows of 2^21 bits are 17 GB
    assert refused(own_gpu, ERR_ARG, "workspace", call(21, 12, (0, 0, 0), (1, 1, 1 << 21), 127, 0, out))
    assert refused(own_gpu, ERR_ARG, "workspace", call(21, 12, (0, 0, 0), (1 << 15, 1, 1 << 15), 1, 2, out))
    for bad in (0, 12, size + 4, CAPACITY + 8):  # n_words last
        assert refused(own_gpu, ERR_ARG, "n_words", call(7, bad, o, s, 4, 0, out))
        assert refused(own_gpu, ERR_ARG, "n_words", call(7, bad, o, (0, 1, 1), 4, 0, out))  # (also with nothing to do)
    for box in (((120, 0, 0), (9, 1, 1)), ((0, 0, 0), (1, 1, 1 << 21))):
        with pytest.raises(pkg.SvoError):
            render.distance_dense(*box, 127, 21 if box[1][2] > 1 else 7)
    with pytest.raises(pkg.SvoError):
        render.distance_dense(o, s, 128, 7)
    assert out.untouched_from(0)
    assert np.array_equal(render.read_nodes(base.size + PAD), before)
    # no node buffer: behind the arguments, before n_words
    fresh = pkg.Gpu(0)
    try:
        assert refused(fresh, ERR_STATE, "svo_nodes_alloc", raw(pkg, fresh, 7, 12, o, s, 4, 0, out))
        assert refused(fresh, ERR_ARG, "workspace", raw(pkg, fresh, 21, 12, (0, 0, 0), (1, 1, 1 << 21), 127, 0, out))
        with pytest.raises(pkg.SvoError, match="no distance field"):
            fresh.distance_timing()  # nothing computed on it yet
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
        torch.cuda.synchronize()
        # the edit is enqueued on the second context's stream; the field on the first follows at once
        p = pkg._lib.EditParams()
        p.depth, p.n_words = 7, base.size
        n_words = C.c_uint64()
        assert pkg._lib.lib().svo_nodes_edit(g2._h, c.data_ptr(), col.data_ptr(), len(b[0]), C.byref(p), C.byref(n_words)) == 0
        render.node_length = n_words.value
        origin, size = (20, 30, 40), (60, 50, 70)
        d2, sites = render.distance_dense(origin, size, 5, 7, mode="signed", with_sites=True)
        g2.sync()
        assert n_words.value == tree7["words"].size
        want = D.brute_grid(tree7["grid"], origin, size, 5, D.SIGNED)
        assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(sites.cpu().numpy().view(np.uint32), want[1])
        stale = D.brute(base, base.size, 7, origin, size, 5, D.SIGNED)
        assert not np.array_equal(stale[0], want[0])
        del r2
    finally:
        g2.close()


def test_a_device_adaptive_state_is_no_obstacle_and_the_times(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg.Gpu(0)
    try:
        r, device = pkg.Render.from_world(g, (64, 64), monu9_world(pkg), 6, capacity=200_000)
        with pytest.raises(pkg.SvoError, match="no distance field"):
            g.distance_timing()
        words = r.read_nodes()
        side = 32
        for mode, name in enumerate(pkg.distance.MODES):
            d2, sites = r.distance_dense((0, 0, 0), (side,) * 3, 6, 5, mode=name, with_sites=True)
            want = D.brute(words, words.size, 5, (0, 0, 0), (side,) * 3, 6, mode)
            assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(sites.cpu().numpy().view(np.uint32), want[1])
        assert (want[0] < 0).any() and (want[0] > 0).any()
        ms = g.distance_timing()
        assert len(ms) == 5 and all(np.isfinite(t) and t >= 0 for t in ms) and ms[4] > 0 and ms == g.distance_timing()
        # a refused call leaves the times
        out = Out(g, 8)
        assert raw(pkg, g, 5, words.size, (0, 0, 0), (33, 1, 1), 4, 0, out) == ERR_ARG
        assert ms == g.distance_timing() and out.untouched_from(0)
        assert np.array_equal(r.read_nodes(), words)
        del device
    finally:
        g.close()


def sampled(render, depth):
    side = 1 << depth
    return render.sample_dense((0, 0, 0), (side,) * 3, depth).cpu().numpy().view(np.uint32)


def check_ball(render, words, grid, depth, op, radius, origin, size, colour, what):
    """morph_ball on the GPU: the whole grid afterwards == the per-cell contract from brute"""
    set_base(render, words, 2_000_000)
    want_d2, want_sites = D.brute_grid(grid, origin, size, radius, D.TO_VOXELS if op == "grow" else D.TO_EMPTY)
    want, changed = D.morph_ball(grid, origin, size, want_d2, want_sites, op, colour)
    n = render.morph_ball(op, radius, origin, size, colour=colour, depth=depth)
    assert n == render.node_length and n % 8 == 0
    got = sampled(render, depth)
    assert_same(got.reshape(-1), want.reshape(-1), what, "the grid")
    assert changed.sum() > 100 and (got != grid).sum() == changed.sum(), what
    return got


def test_morph_ball_on_tree7(pkg, render, tree7):
    words, grid = tree7["words"], tree7["grid"]
    origin, size = (10, 20, 30), (90, 70, 60)
    check_ball(render, words, grid, 7, "grow", 3, origin, size, 0xABCDEF, "tree7, grow 3, coloured")
    check_ball(render, words, grid, 7, "grow", 5, origin, size, None, "tree7, grow 5, the nearest voxel's colour")
    check_ball(render, words, grid, 7, "shrink", 2, origin, size, None, "tree7, shrink 2")
    # a box in which nothing changes: the words stay
    set_base(render, ROOT)
    assert render.morph_ball("grow", 4, (0, 0, 0), (32, 32, 32), depth=7) == 8 and np.array_equal(render.read_nodes(), ROOT)
    for bad in (dict(op="close"), dict(size=(513, 1, 1)), dict(radius=0), dict(radius=128)):
        with pytest.raises(ValueError):
            render.morph_ball(**{**dict(op="grow", radius=2, origin=(0, 0, 0), size=(8, 8, 8), depth=7), **bad})


def test_morph_ball_on_a_simplified_ball_and_its_frame(pkg, render, O):
    words, grid, depth = scenes()["ball"]
    grid = grid.astype(np.uint32)
    assert (words >> 4 >= B.VOXEL_OFFSET).sum() < (grid != 0).sum() // 4  # coarse leaves hold most of it
    origin, size = (0, 0, 0), (128, 128, 64)  # half of the ball: the other half keeps its coarse leaves and its colours
    check_ball(render, words, grid, depth, "shrink", 6, origin, size, None, "ball, shrink 6")
    check_ball(render, words, grid, depth, "grow", 4, origin, size, 0x123456, "ball, grow 4, coloured")
    check_ball(render, words, grid, depth, "grow", 7, origin, size, None, "ball, grow 7, the nearest voxel's colour")
    grown = render.read_nodes()
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    g = pkg.Gpu(0)  # (a context that never declared a deeper tree)
    try:
        assert_hits_equal(frame(pkg, pkg.Render(g, (64, 64), grown), u), O.trace_frame(grown, u, threads=4), "the grown ball")
    finally:
        g.close()


def test_morph_ball_refuses_a_mark_before_any_write(pkg, render):
    mixed = mixed_levels()
    set_base(render, mixed)
    before = render.read_nodes(mixed.size + PAD)
    coarse = S.sample_dense(mixed, mixed.size, (0, 0, 0), (16, 16, 16), 4)
    assert (coarse == S.FINER).any()
    with pytest.raises(pkg.SvoError, match="mark"):
        render.morph_ball("grow", 2, (0, 0, 0), (16, 16, 16), depth=4)
    assert render.node_length == mixed.size and np.array_equal(render.read_nodes(mixed.size + PAD), before)
