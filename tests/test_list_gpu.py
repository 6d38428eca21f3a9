"""Voxels listed on the GPU (csrc/svo_list.hip): coordinates, values and levels against the sequential
restatement of the contract (tests/list_ref.py) on empty, full, depth-21, built, edited, compacted, counter-carrying and
mixed-level trees, natively and expanded; the same bytes for every layout of a tree and on every run; the list rebuilt
into the pruned tree; nothing written behind n, nothing on any error or count query, the node buffer never; an edit
through a sharing context seen; a device adaptive state no obstacle; World.save_nodes against build_world."""
import ctypes as C
import os

import numpy as np
import pytest

import build_ref as B
import list_ref as L
from pass_frame import SLACK, SentinelOut, last_error, monu9_world, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases, orphaned, survivors
from test_edit_gpu import CAPACITY, PAD, ROOT, frame, poison, set_base
from test_list_host import full_root, mixed_levels, one_leaf_root, voxel_list

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_CAP = -1, -3, -6
EXPAND = 1


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def tree7():
    """pass_frame.tree7_base (the base, the edited words in put order) with both lists' references and the surviving
    voxels, computed once"""
    t = tree7_base()
    base, words = t["base"], t["words"]
    return {**t, "base list": L.list_voxels(base, base.size, 7), "list": L.list_voxels(words, words.size, 7),
            "left": survivors(7, t["a"], t["b"])}


class Out(SentinelOut):
    """sentinel-filled device outputs of `room` entries"""

    def __init__(self, gpu, room, levels=True):
        super().__init__(gpu, [(room, 3), room, room if levels else None])
        self.xyz, self.value, self.level = self.t
        self.room = room


def raw_list(pkg, gpu, flags, depth, n_words, out=None, max_voxels=None, params=True, n_out=True, value=True):
    p = pkg._lib.ListParams()
    p.flags, p.depth, p.n_words = flags, depth, n_words
    p.max_voxels = (out.room if out is not None else 0) if max_voxels is None else max_voxels
    n = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_nodes_list_voxels(
        gpu._h, C.byref(p) if params else None, out.xyz.data_ptr() if out is not None else None,
        out.value.data_ptr() if out is not None and value else None,
        out.level.data_ptr() if out is not None and out.level is not None else None, C.byref(n) if n_out else None)
    gpu.sync()
    return rc, n.value


def check_list(pkg, render, words, depth, expand, what, want=None, loaded=False):
    """the words' list on the GPU == the reference, levels included; the count query agrees and writes nothing; nothing
    is written behind n; the node buffer reads back unchanged.  Returns the list's three host arrays."""
    want = want if want is not None else L.list_voxels(words, words.size, depth, expand)
    if not loaded:
        set_base(render, words)
    before = render.read_nodes(words.size + PAD)
    assert np.array_equal(before[:words.size], words) and (loaded or np.array_equal(before[words.size:], poison(PAD)))
    flags = EXPAND if expand else 0
    rc, n = raw_list(pkg, render.gpu, flags, depth, words.size)
    assert rc == 0, f"{what}: count query: status {rc}: {last_error(pkg, render.gpu)}"
    assert n == want[1].size, f"{what}: count {n}, want {want[1].size}"
    out = Out(render.gpu, n + SLACK)
    rc, m = raw_list(pkg, render.gpu, flags, depth, words.size, out)
    assert rc == 0, f"{what}: status {rc}: {last_error(pkg, render.gpu)}"
    assert m == n, f"{what}: the fill's n {m}, the count query's {n}"
    got = out.host()
    for g, w, name in zip(got, want, ("xyz", "value", "level")):
        if not np.array_equal(g[:n], w):
            bad = np.flatnonzero((g[:n] != w).reshape(n, -1).any(axis=1))
            raise AssertionError(f"{what}: {bad.size} entries differ in {name}, first at {bad[:3]}: got {g[bad[:3]]} want {w[bad[:3]]}")
    assert out.untouched_from(n), f"{what}: written behind n"
    assert np.array_equal(render.read_nodes(words.size + PAD), before), f"{what}: the node buffer was written"
    return tuple(g[:n] for g in got)


def test_empty_and_full_root(pkg, render):
    for depth in (1, 5, 21):
        for expand in (False, True):
            assert check_list(pkg, render, ROOT, depth, expand, f"empty root, depth {depth}")[1].size == 0
    set_base(render, ROOT)
    coords, colours, levels = render.list_voxels(with_levels=True)
    assert coords.shape == (0, 3) and colours.shape == (0,) and levels.shape == (0,)
    full = full_root()
    cells = np.array([[c >> 2 & 1, c >> 1 & 1, c & 1] for c in range(8)], dtype=np.uint32)
    for depth in (1, 9, 21):
        xyz, value, level = check_list(pkg, render, full, depth, False, f"full root, depth {depth}")
        assert np.array_equal(xyz, cells << (depth - 1)) and (level == 1).all() and np.array_equal(value, (full >> 4) - B.VOXEL_OFFSET)
    assert check_list(pkg, render, full, 3, True, "full root expanded to depth 3")[1].size == 8 * 64


def test_depth_21_voxel(pkg, render):
    cell = [[(1 << 21) - 1, 5, 1234567]]
    words = B.build(cell, 21, [0x00FF00])
    for expand in (False, True):
        xyz, value, level = check_list(pkg, render, words, 21, expand, "depth 21")
        assert xyz.tolist() == cell and value.tolist() == [0x00FF00] and level.tolist() == [21]
    coords, colours = render.list_voxels(21)
    assert coords.cpu().numpy().tolist() == cell and colours.dtype == coords.dtype and coords.dtype.is_signed


def test_built_tree_partial_waves_and_scan_tiles(pkg, render, tree7):
    base, a = tree7["base"], tree7["a"]
    xyz, value, level = check_list(pkg, render, base, 7, False, "depth 7", tree7["base list"])
    want = voxel_list(7, *a)
    assert np.array_equal(xyz, want[0]) and np.array_equal(value, want[1]) and (level == 7).all()
    # random counter bits in every word: the same list
    counted = base | np.random.default_rng(6).integers(0, 16, base.size).astype(np.uint32)
    check_list(pkg, render, counted, 7, False, "depth 7 with counters", tree7["base list"])
    check_list(pkg, render, counted, 8, True, "depth 7 with counters, expanded one level")
    # interior words overwritten by the empty word: what hangs below them is not listed
    cut = orphaned(base, 50, np.random.default_rng(50))
    assert check_list(pkg, render, cut, 7, False, "orphans")[1].size < want[1].size


def test_every_layout_and_every_run_list_identically(pkg, render, tree7):
    words, want = tree7["words"], tree7["list"]
    put = check_list(pkg, render, words, 7, False, "edited, put order", want)
    again = check_list(pkg, render, words, 7, False, "edited, second run", want, loaded=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(put, again))
    for prune in (False, True):
        set_base(render, words)
        n = render.compact_nodes(prune=prune)
        layout = render.read_nodes()
        assert n < words.size or not prune
        got = check_list(pkg, render, layout, 7, False, f"compacted, prune {prune}", want)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(put, got))
    pruned = layout
    left = voxel_list(7, *tree7["left"])
    assert np.array_equal(put[0], left[0]) and np.array_equal(put[1], left[1])
    # the list, as the public call returns it, rebuilds the pruned tree word for word
    set_base(render, words)
    coords, colours = render.list_voxels(7)
    assert np.array_equal(coords.cpu().numpy().view(np.uint32), put[0])
    assert render.build_nodes(coords, 7, colours) == pruned.size
    assert np.array_equal(render.read_nodes(), pruned)


def value_image(hits, words):
    """per pixel the leaf word's value (word >> 4) at the hit's node index; a miss keeps its marker, out of the words' range"""
    v = hits["value"].astype(np.int64)
    return np.where(v < words.size, (words[np.minimum(v, words.size - 1)] >> 4).astype(np.int64), v + (1 << 32))


def test_mixed_levels_native_and_expanded(pkg, render, own_gpu, O):
    mixed = mixed_levels()
    native = check_list(pkg, render, mixed, 6, False, "mixed levels")
    assert set(native[2].tolist()) == {2, 3, 4, 5, 6}
    want = L.list_voxels(mixed, mixed.size, 6, True)
    assert want[1].size < 200_000 and want[1].size > native[1].size + 4096
    check_list(pkg, render, mixed, 6, True, "mixed levels, expanded", want)
    check_list(pkg, render, mixed, 8, False, "mixed levels on the depth-8 grid")
    # the tree of the expanded list shows the same values as the coarse tree from one camera.  A hit record's `value` is
    # the index of the leaf word, which depends on the layout: the image compared is that word's value (a miss keeps its
    # marker), and t, which does not depend on the depth of the hit
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    set_base(render, mixed)
    coarse = frame(pkg, render, u)
    coords, colours, levels = render.list_voxels(6, expand=True, with_levels=True)
    assert bool((levels == 6).all())
    render.build_nodes(coords, 6, colours)
    fine, fine_words = frame(pkg, render, u), render.read_nodes()
    assert (coarse["value"] < mixed.size).sum() > 2000  # (the oracle's frame of this tree hits in 2 958 pixels)
    assert np.array_equal(value_image(coarse, mixed), value_image(fine, fine_words))
    assert np.array_equal(coarse["t"], fine["t"])
    # one record of 2 097 152 cells: the emit is balanced over the entries
    one = one_leaf_root()
    set_base(render, one)
    coords, colours = render.list_voxels(8, expand=True)
    assert coords.shape == (1 << 21, 3) and bool((colours == 0xABCDEF).all())
    assert np.array_equal(coords.cpu().numpy().view(np.uint32), L.demorton((5 << 21) + np.arange(1 << 21), 8))
    assert np.array_equal(render.read_nodes(8), one)


def test_errors_write_nothing(pkg, render, own_gpu, tree7):
    base = tree7["base"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    count = tree7["base list"][1].size
    out = Out(own_gpu, count + SLACK)
    refused = lambda code, part, *a, **kw: (raw_list(pkg, own_gpu, *a, **kw) == (code, 12345)  # noqa: E731
                                            and part in last_error(pkg, own_gpu))
    assert refused(ERR_ARG, "null", 0, 7, base.size, out, params=False)
    assert refused(ERR_ARG, "null", 0, 7, base.size, out, n_out=False)
    assert refused(ERR_ARG, "flag", 2, 7, base.size, out)
    assert refused(ERR_ARG, "flag", 1 | 1 << 31, 7, base.size, out)
    for depth in (0, 22):
        assert refused(ERR_ARG, "depth", 0, depth, base.size, out)
    assert refused(ERR_ARG, "value_out_dev", 0, 7, base.size, out, value=False)
    for n in (0, 12, base.size + 4, CAPACITY + 8):
        assert refused(ERR_ARG, "n_words", 0, 7, n, out)
    # the tree is deeper than depth
    for flags in (0, EXPAND):
        assert refused(ERR_ARG, "level 7", flags, 6, base.size, out)
        assert refused(ERR_ARG, "level 7", flags, 6, base.size)
    with pytest.raises(pkg.SvoError):
        render.list_voxels(3)
    # room for one entry less than there are; a count query does not look at max_voxels
    assert refused(ERR_CAP, f"{count} entries", 0, 7, base.size, out, max_voxels=count - 1)
    assert raw_list(pkg, own_gpu, 0, 7, base.size, max_voxels=0) == (0, count)
    assert out.untouched_from(0)
    assert np.array_equal(render.read_nodes(base.size + PAD), before)
    # a level-1 voxel expanded at depth 21: 8^20 cells, counted in 64 bits
    set_base(render, one_leaf_root())
    assert refused(ERR_CAP, f"{8 ** 20} entries", EXPAND, 21, 8, out)
    assert refused(ERR_CAP, f"{8 ** 20} entries", EXPAND, 21, 8)
    assert raw_list(pkg, own_gpu, 0, 21, 8) == (0, 1)
    assert refused(ERR_CAP, f"{8 ** 11} entries", EXPAND, 12, 8)  # 2^33: the low 32 bits are 0

    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice", "32 levels": "deeper than 31"}
    cases = malformed_cases()
    assert set(cases) == set(causes)
    for name, words in cases.items():
        set_base(render, words)
        before = render.read_nodes(words.size + PAD)
        for flags in (0, EXPAND):
            for o in (out, None):
                assert raw_list(pkg, own_gpu, flags, 21, words.size, o) == (ERR_STATE, 12345), name
                assert "malformed tree: " in last_error(pkg, own_gpu) and causes[name] in last_error(pkg, own_gpu), f"{name}: {last_error(pkg, own_gpu)}"
        with pytest.raises(pkg.SvoError):
            render.list_voxels(21)
        assert np.array_equal(render.read_nodes(words.size + PAD), before), name
    assert out.untouched_from(0)

    fresh = pkg.Gpu(0)
    try:
        assert raw_list(pkg, fresh, 0, 7, 8)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
    finally:
        fresh.close()


def test_timing(pkg, render, own_gpu, tree7):
    set_base(render, tree7["base"])
    render.list_voxels(7)
    ms = own_gpu.list_timing()
    assert len(ms) == 5 and all(t >= 0 for t in ms) and ms[4] > 0
    assert ms == own_gpu.list_timing()
    assert raw_list(pkg, own_gpu, 0, 3, tree7["base"].size)[0] == ERR_ARG  # a refused call leaves the times
    assert ms == own_gpu.list_timing()


def test_an_edit_through_a_sharing_context_is_seen(pkg, render, own_gpu, tree7):
    g2 = pkg.Gpu(0)
    try:
        base = tree7["base"]
        set_base(render, base, 8 * 4097 * 7)
        own_gpu.sync()
        r2 = pkg.Render.share_nodes(g2, render)
        b = tree7["b"]
        import torch
        dev = torch.device("cuda", 0)
        c, col = torch.as_tensor(b[0], dtype=torch.int32, device=dev), torch.as_tensor(b[1] & 0xFFFFFF, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        # the edit is enqueued on the second context's stream; the list on the first follows at once
        p = pkg._lib.EditParams()
        p.depth, p.n_words = 7, base.size
        n_words = C.c_uint64()
        assert pkg._lib.lib().svo_nodes_edit(g2._h, c.data_ptr(), col.data_ptr(), len(b[0]), C.byref(p), C.byref(n_words)) == 0
        render.node_length = n_words.value
        coords, colours, levels = render.list_voxels(7, with_levels=True)
        g2.sync()
        assert n_words.value == tree7["words"].size
        want = tree7["list"]
        for got, w in zip((coords, colours, levels), want):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), w)
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
        want = L.list_voxels(words, words.size, depth)
        coords, colours, levels = r.list_voxels(depth, with_levels=True)
        assert want[1].size > 100
        for got, w in zip((coords, colours, levels), want):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), w)
        assert np.array_equal(r.read_nodes(), words)
        del device
    finally:
        g.close()


def test_save_nodes_equals_build_world_of_the_surviving_voxels(pkg, render, own_gpu, tree7, tmp_path):
    set_base(render, tree7["words"])
    before = render.read_nodes(tree7["words"].size + PAD)
    saved, built = str(tmp_path / "saved"), str(tmp_path / "built")
    world = pkg.World.save_nodes(saved, render, 7, world_depth=1)
    assert world.chunk_ids()
    coords, colours = tree7["left"]
    pkg.World.build_world(built, own_gpu, coords, 7, colours, world_depth=1)
    files = sorted(os.listdir(built))
    assert files == sorted(os.listdir(saved)) and "0.bin" in files and len(files) > 1
    for name in files:
        assert open(os.path.join(saved, name), "rb").read() == open(os.path.join(built, name), "rb").read(), name
    assert np.array_equal(render.read_nodes(tree7["words"].size + PAD), before)
