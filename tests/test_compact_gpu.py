"""Trees compacted on the GPU (csrc/svo_compact.hip): words and perm against the sequential restatement of
the contract (tests/compact_ref.py) and the host's relayout, on empty, chained, edited, orphaned, host-layout and
counter-carrying trees; the pruned tree against a rebuild of the surviving voxels; the freed tail empty, nothing written
behind n_words or on any error; the same words on every run; frames traced from compacted trees against the oracle,
also when the compaction came through a context that shares the buffer."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import compact_ref as K
from conftest import GOLDEN, assert_hits_equal, load_vox_fixture
from pass_frame import SENTINEL, SentinelOut, assert_words, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases, orphaned, survivors
from test_edit_gpu import CAPACITY, PAD, ROOT, frame, monu9_edits, poison, set_base

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
PRUNE = 1


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def tree7():
    """pass_frame.tree7_base (A, B, the canonical base, the edited words in put order) and the references of both flag
    settings, computed once"""
    t = tree7_base()
    words = t["words"]
    return {**t, False: K.compact(words, words.size, False), True: K.compact(words, words.size, True)}


def raw_compact(pkg, gpu, flags, n_words, perm=None, params=True, out=True):
    p = pkg._lib.CompactParams()
    p.flags, p.n_words = flags, n_words
    n = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_nodes_compact(gpu._h, C.byref(p) if params else None, perm.data_ptr() if perm is not None else None,
                                          C.byref(n) if out else None)
    gpu.sync()
    return rc, n.value


def sentinel_perm(gpu, n):
    return SentinelOut(gpu, [n]).t[0]


def check_compact(pkg, render, words, prune, what, want=None):
    """words -> compacted on the GPU == the reference, words and perm; the freed tail holds the empty word; the words
    behind n_words and the perm behind the new length keep what they held"""
    want, want_perm = want if want is not None else K.compact(words, words.size, prune)
    set_base(render, words)
    perm = sentinel_perm(render.gpu, words.size)
    rc, n = raw_compact(pkg, render.gpu, PRUNE if prune else 0, words.size, perm)
    assert rc == 0, f"{what}: status {rc}: {pkg._lib.lib().svo_last_error(render.gpu._h).decode()}"
    assert n == want.size, f"{what}: length {n}, want {want.size}"
    got = render.read_nodes(words.size + PAD)
    assert_words(got[:n], want, what)
    assert (got[n:words.size] == B.EMPTY).all(), f"{what}: the freed tail is not empty"
    assert np.array_equal(got[words.size:], poison(PAD)), f"{what}: words behind n_words were written"
    perm = perm.cpu().numpy().view(np.uint32)
    assert np.array_equal(perm[:n], want_perm), f"{what}: perm"
    assert (perm[n:] == SENTINEL).all(), f"{what}: perm written behind the new length"
    render.node_length = n
    return want


def test_empty_root_stays_8_words(pkg, render):
    for prune in (False, True):
        assert check_compact(pkg, render, ROOT, prune, f"empty root, prune {prune}").size == 8
        set_base(render, ROOT)
        assert render.compact_nodes(prune=prune) == 8 == render.node_length


def test_depth_21_voxel_put_and_removed(pkg, render):
    cell = [[(1 << 21) - 1, 5, 1234567]]
    set_base(render, ROOT, 160)
    assert render.edit_nodes(cell, 21, [0x00FF00]) == 168
    put = render.read_nodes()
    assert check_compact(pkg, render, put, True, "depth 21, the voxel in place").size == 168
    assert render.edit_nodes(cell, 21, [0]) == 168
    removed = render.read_nodes()
    assert check_compact(pkg, render, removed, False, "depth 21, removed, no pruning").size == 168
    want = check_compact(pkg, render, removed, True, "depth 21, removed, pruned")
    assert want.size == 8 and (want == B.EMPTY).all()
    assert (render.read_nodes(168) == B.EMPTY).all()


def test_edited_tree_partial_waves_and_scan_tiles(pkg, render, tree7):
    words = tree7["words"]
    levels = np.diff(level_starts(tree7[False][0]))
    assert (levels > 4096).any() and (levels[1:] % 8 != 0).any()
    for prune in (False, True):
        want = check_compact(pkg, render, words, prune, f"depth 7 edited, prune {prune}", tree7[prune])
    assert want.size < tree7[False][0].size <= words.size
    # the pruned tree is the tree of the voxels that are left, as the device builds it
    coords, colours = survivors(7, tree7["a"], tree7["b"])
    assert render.build_nodes(coords, 7, colours) == want.size
    assert_words(render.read_nodes(), want, "rebuilt from the surviving voxels")


def level_starts(canonical):
    """group index at which every level of a canonical breadth-first tree starts (and the group count)"""
    starts, lo, hi = [0], 0, 1
    while hi > lo:
        g = canonical[8 * lo:8 * hi]
        n = int((g >> 4 < B.VOXEL_OFFSET).sum())
        starts.append(hi)
        lo, hi = hi, hi + n
    return np.array(starts)


def test_orphaned_groups_are_dropped(pkg, render, tree7):
    base = tree7["base"]
    cut = orphaned(base, 50, np.random.default_rng(50))
    set_base(render, base)
    for i in np.flatnonzero(cut != base):
        render.write_nodes(cut[i:i + 1], offset=int(i))
    assert np.array_equal(render.read_nodes(base.size), cut)
    for prune in (False, True):
        want = check_compact(pkg, render, cut, prune, f"orphans, prune {prune}")
        assert want.size < base.size


def test_host_layout_base_equals_the_hosts_relayout(pkg, render, small_words):
    base = np.asarray(small_words)
    want = pkg.scenes.relayout(base, 32, with_perm=True)
    assert not np.array_equal(base, want[0])
    check_compact(pkg, render, base, False, "small fixture", want)
    set_base(render, base)
    n, perm = render.compact_nodes(prune=False, with_perm=True)
    assert n == want[0].size == render.node_length and np.array_equal(perm.cpu().numpy().view(np.uint32), want[1])


def test_every_run_and_counters(pkg, render, tree7):
    words = tree7["words"]
    for prune in (False, True):
        for _ in range(3):
            set_base(render, words)
            assert render.compact_nodes(prune=prune) == tree7[prune][0].size
            assert np.array_equal(render.read_nodes(), tree7[prune][0])
    rng = np.random.default_rng(6)
    counted = words | rng.integers(0, 16, words.size).astype(np.uint32)
    plain, perm = tree7[False]
    got = check_compact(pkg, render, counted, False, "counters, no pruning", (plain | (counted[perm] & 15), perm))
    assert np.array_equal(got & 15, counted[perm] & 15)
    plain, perm = tree7[True]
    cut = (counted[perm] >> 4 < B.VOXEL_OFFSET) & (plain == B.EMPTY)  # interior words whose group was dead
    assert cut.sum() > 10
    want = np.where(cut, B.EMPTY, plain | (counted[perm] & 15)).astype(np.uint32)
    check_compact(pkg, render, counted, True, "counters, pruned", (want, perm))


def test_errors_write_nothing(pkg, render, own_gpu, tree7):
    last_error = lambda g=own_gpu: pkg._lib.lib().svo_last_error(g._h).decode()  # noqa: E731
    base = tree7["base"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    perm = sentinel_perm(own_gpu, base.size)
    for kw in (dict(params=False), dict(out=False)):
        assert raw_compact(pkg, own_gpu, 0, base.size, perm, **kw)[0] == ERR_ARG and "null" in last_error()
    assert raw_compact(pkg, own_gpu, 2, base.size, perm)[0] == ERR_ARG and "flag" in last_error()
    assert raw_compact(pkg, own_gpu, 1 | 1 << 31, base.size, perm)[0] == ERR_ARG
    for n in (0, 12, base.size + 4, CAPACITY + 8):
        assert raw_compact(pkg, own_gpu, PRUNE, n, perm) == (ERR_ARG, 0) and "n_words" in last_error()
    assert np.array_equal(render.read_nodes(base.size + PAD), before)

    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice", "32 levels": "deeper than 31"}
    cases = malformed_cases()
    assert set(cases) == set(causes)
    for name, words in cases.items():
        set_base(render, words)
        before = render.read_nodes(words.size + PAD)
        for flags in (0, PRUNE):
            assert raw_compact(pkg, own_gpu, flags, words.size, perm) == (ERR_STATE, 0), name
            assert "malformed tree: " in last_error() and causes[name] in last_error(), f"{name}: {last_error()}"
        with pytest.raises(pkg.SvoError):
            render.compact_nodes()
        assert render.node_length == words.size
        assert np.array_equal(render.read_nodes(words.size + PAD), before), name
    assert (perm.cpu().numpy().view(np.uint32) == SENTINEL).all()

    fresh = pkg.Gpu(0)
    try:
        assert raw_compact(pkg, fresh, PRUNE, 8)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(fresh)
    finally:
        fresh.close()
    # a device adaptive state indexes the layout that a compaction would replace
    size, xyzi, pal, _, _ = load_vox_fixture("monu9")
    world = pkg.adaptive.World(pkg.CpuOctree.from_voxels(size, xyzi, pal))
    octree = world.root_octree()
    g = pkg.Gpu(0)
    try:
        g.set_option(pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, 1)
        r = pkg.Render.new(g, (64, 64), octree, capacity=4096)
        attached = pkg.adaptive.DeviceAdaptive(g, r, octree, world)
        before = r.read_nodes()
        assert raw_compact(pkg, g, PRUNE, r.node_length)[0] == ERR_STATE and "adaptive" in last_error(g)
        with pytest.raises(pkg.SvoError):
            r.compact_nodes()
        assert r.node_length == before.size and np.array_equal(r.read_nodes(), before)
        del attached
    finally:
        g.close()


def test_compacted_trees_trace_like_the_oracle(pkg, O):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    (label, size, xyzi, pal), = B.fixture_models(GOLDEN, "monu9")
    coords, colours, depth = B.vox_voxels(size, xyzi, pal)
    box, deeper, deeper_colours = monu9_edits(coords, depth)
    g1, g2 = pkg.Gpu(0), pkg.Gpu(0)
    try:
        r1 = pkg.Render.from_voxels(g1, (64, 64), coords, depth, colours, capacity=CAPACITY)
        u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
        r1.edit_nodes(box, depth, np.zeros(len(box), dtype=np.int64))
        carved = r1.read_nodes()
        want = K.compact(carved, carved.size, True)[0]
        assert want.size < carved.size
        assert r1.compact_nodes() == want.size
        assert_words(r1.read_nodes(), want, "carved and pruned")
        assert (r1.read_nodes(carved.size)[want.size:] == B.EMPTY).all()
        hits = O.trace_frame(want, u, threads=4)
        for variant in (pkg.gpu.VARIANT_STACK, pkg.gpu.VARIANT_RESTART):
            g1.set_option(pkg.gpu.OPT_VARIANT, variant)
            assert_hits_equal(frame(pkg, r1, u), hits, f"carved and pruned, variant {variant}")

        # filled one level deeper, then compacted through a second context that shares the store; traced through the first
        r1.edit_nodes(deeper, depth + 1, deeper_colours)
        filled = r1.read_nodes()
        g1.sync()
        r2 = pkg.Render.share_nodes(g2, r1)
        want = K.compact(filled, filled.size, True)[0]
        assert want.size <= filled.size and not np.array_equal(want, filled[:want.size])  # (put order to breadth-first)
        assert r2.compact_nodes() == want.size
        g2.sync()
        r1.node_length = r2.node_length
        assert_words(r1.read_nodes(), want, "filled and compacted")
        hits = O.trace_frame(want, u, threads=4)
        for variant in (pkg.gpu.VARIANT_RESTART, pkg.gpu.VARIANT_STACK):
            g1.set_option(pkg.gpu.OPT_VARIANT, variant)
            assert_hits_equal(frame(pkg, r1, u), hits, f"compacted through the sharing context, variant {variant}")
        assert_hits_equal(frame(pkg, r2, u), hits, "on the context that compacted")
    finally:
        g2.close()
        g1.close()


def test_timing(pkg, render, own_gpu, tree7):
    set_base(render, tree7["words"])
    render.compact_nodes()
    ms = own_gpu.compact_timing()
    assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[5] > 0
    assert ms == own_gpu.compact_timing()
    # a refused call in between leaves the times of the last compaction that ran, whether they were fetched or not
    render.compact_nodes()
    words = malformed_cases()["two parents sharing one group"]
    set_base(render, words)
    assert raw_compact(pkg, own_gpu, PRUNE, words.size)[0] == ERR_STATE
    after = own_gpu.compact_timing()
    assert len(after) == 6 and all(t >= 0 for t in after) and after[5] > 0
    assert raw_compact(pkg, own_gpu, PRUNE, words.size)[0] == ERR_STATE
    assert after == own_gpu.compact_timing()
