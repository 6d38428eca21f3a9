"""Trees edited in place on the GPU (csrc/svo_edit.hip): word for word against the sequential restatement
of the host model (tests/edit_ref.py) on canonical, host-layout and counter-carrying bases; the same words for any
order of distinct voxels and on every run; nothing written behind the new length or on any error; frames traced from
edited trees against the oracle, also when the edit came through a context that shares the buffer."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import edit_ref as E
from conftest import GOLDEN, assert_hits_equal, load_vox_fixture, set_uniforms_from_oracle
from pass_frame import assert_words, own_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

CAPACITY = 4_000_000
PAD = 4096  # poisoned words behind the base that must stay as they are
ERR_ARG, ERR_STATE, ERR_CAP = -1, -3, -6
ROOT = np.full(8, B.EMPTY, dtype=np.uint32)


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def base6():
    """about 2 000 random voxels at depth 6, clustered so that whole level-2 cells stay empty: (coords, canonical words)"""
    rng = np.random.default_rng(60)
    coords = rng.integers(0, 40, (2000, 3))
    colours = rng.integers(1, 1 << 24, 2000)
    return coords, B.build(coords, 6, colours)


def poison(n):
    return np.arange(0xDEAD0000, 0xDEAD0000 + n, dtype=np.uint32)


def set_base(render, base, growth=0):
    """the base in the node buffer, with poison over the words an edit of `growth` new words may take and PAD more"""
    render.write_nodes(np.concatenate([base, poison(growth + PAD)]))
    render.node_length = base.size


def check_edit(render, base, coords, depth, colours, what, **kw):
    """base -> edit on the GPU == edit_ref.edit, and the words behind the new length keep what they held"""
    want = E.edit(base, base.size, coords, depth, colours, **kw)
    growth = want.size - base.size
    set_base(render, base, growth)
    n = render.edit_nodes(coords, depth, colours, **kw)
    assert n == want.size == render.node_length, f"{what}: length {n}, want {want.size}"
    got = render.read_nodes(n + PAD)
    assert_words(got[:n], want, what)
    assert np.array_equal(got[n:], poison(growth + PAD)[growth:]), f"{what}: words behind the new length were written"
    return want


def edit_voxels(rng, depth, n, near, shift):
    """n edit voxels at `depth`: random cells, cells of and next to the base's voxels (scaled by 2^shift: overwrites,
    shared prefixes), a cluster under one cell that the base leaves empty, duplicate cells, colour 0, high bits only"""
    side = 1 << depth
    coords = rng.integers(0, side, (n, 3))
    pick = (near[rng.integers(0, len(near), n // 2)] << shift) + rng.integers(0, 1 << shift, (n // 2, 3))
    coords[: n // 2] = pick
    coords[n // 2: n // 2 + n // 8] = np.clip(pick[: n // 8] + rng.integers(-1, 2, (n // 8, 3)), 0, side - 1)
    cluster = n // 8
    coords[-cluster:] = (side - 8) + rng.integers(0, 8, (cluster, 3))  # under the far corner's empty level-3 leaf
    coords[n - cluster - n // 8: n - cluster] = coords[: n // 8]  # duplicates: the later one wins
    colours = rng.integers(1, 1 << 32, n)
    colours[::5] = 0
    colours[1::9] = 0xFF000000
    return coords, colours


def test_root_group_writes_only(render):
    cells = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    want = check_edit(render, ROOT, cells, 1, np.arange(1, 9) * 0x010203, "depth 1, all cells")
    assert want.size == 8 and (want != B.EMPTY).all()
    check_edit(render, want, cells[::2], 1, np.zeros(4, dtype=np.int64), "depth 1, four removed")
    check_edit(render, ROOT, cells[:3], 1, None, "depth 1, one colour", colour=0xABCDEF)


def test_one_voxel_in_an_empty_tree(render):
    assert check_edit(render, ROOT, [[3, 0, 2]], 2, [0x123456], "depth 2").size == 16


def test_depth_21_chains(render):
    top = (1 << 21) - 1
    assert check_edit(render, ROOT, [[top, 5, 1234567]], 21, [0x00FF00], "depth 21, one voxel").size == 8 * 21
    two = [[top, 5, 1234567], [top, 5, 1234566]]
    assert check_edit(render, ROOT, two, 21, [1, 2], "depth 21, shared prefix of 20 levels").size == 8 * 21
    far = [[top, 5, 1234567], [0, 5, 1234567], [top, 4, 1234567]]
    assert check_edit(render, ROOT, far, 21, [1, 2, 3], "depth 21, three chains").size == 8 * (1 + 20 + 20)


@pytest.mark.parametrize("n", [4097, 10000])
def test_edits_at_the_base_depth(render, base6, n):
    coords, base = base6
    rng = np.random.default_rng(n)
    ec, ecol = edit_voxels(rng, 6, n, coords, 0)
    want = check_edit(render, base, ec, 6, ecol, f"depth 6, {n} voxels")
    assert want.size > base.size
    # overwrites of leaves that exist: no growth
    same = check_edit(render, base, coords[:500], 6, ecol[:500], "depth 6, overwrites")
    assert same.size == base.size


def test_edits_below_coloured_leaves(render, base6):
    coords, base = base6
    rng = np.random.default_rng(9)
    ec, ecol = edit_voxels(rng, 9, 6000, coords, 3)
    want = check_edit(render, base, ec, 9, ecol, "depth 9 into a depth-6 base")
    # a split leaf's other children are empty: the coarse colour is not carried down
    split = np.flatnonzero((base >> 4 > B.VOXEL_OFFSET) & (want[: base.size] >> 4 < B.VOXEL_OFFSET))
    assert split.size > 100
    kids = (want[split[0]] >> 4) + np.arange(8)
    assert ((want[kids] >> 4 < B.VOXEL_OFFSET) | (want[kids] == B.EMPTY)).all()


def test_host_layout_base(pkg, render, small_words):
    base = np.asarray(small_words)
    assert not np.array_equal(base, pkg.scenes.relayout(base, block_level=32))  # (put order, not breadth-first)
    depth = load_vox_fixture("small")[0].bit_length() - 1
    rng = np.random.default_rng(12)
    side = 1 << (depth + 1)
    coords = rng.integers(0, side, (3000, 3))
    colours = rng.integers(0, 1 << 24, 3000)
    colours[::4] = 0
    check_edit(render, base, coords, depth + 1, colours, "small fixture, one level below")


def test_any_order_and_every_run(render, base6):
    coords, base = base6
    rng = np.random.default_rng(21)
    ec = np.unique(edit_voxels(rng, 8, 8000, coords, 2)[0], axis=0)
    ecol = rng.integers(0, 1 << 24, len(ec))
    first = check_edit(render, base, ec, 8, ecol, "distinct voxels")
    for _ in range(2):
        set_base(render, base)
        assert np.array_equal(render.read_nodes(render.edit_nodes(ec, 8, ecol)), first)
    perm = rng.permutation(len(ec))
    set_base(render, base)
    assert np.array_equal(render.read_nodes(render.edit_nodes(ec[perm], 8, ecol[perm])), first)


def test_untouched_words_keep_their_counters(render, base6):
    coords, base = base6
    rng = np.random.default_rng(33)
    counted = base | rng.integers(1, 16, base.size).astype(np.uint32)
    ec, ecol = edit_voxels(rng, 7, 5000, coords, 1)
    want = check_edit(render, counted, ec, 7, ecol, "base with hit counters")
    kept = want[: base.size] == counted
    assert kept.sum() > base.size // 2 and (want[: base.size][~kept] & 15 == 0).all()


def test_torch_and_numpy_inputs(render, own_gpu, base6):
    import torch
    coords, base = base6
    rng = np.random.default_rng(5)
    ec, ecol = edit_voxels(rng, 7, 3000, coords, 1)
    want = E.edit(base, base.size, ec, 7, ecol)
    dev = torch.device("cuda", own_gpu.device)
    for c, col in ((ec.astype(np.int32), ecol), (torch.from_numpy(ec).to(dev), torch.from_numpy(ecol).to(dev)),
                   (torch.from_numpy(ec).to(dev, torch.int32), torch.from_numpy(ecol & 0xFFFFFF).to(dev, torch.int32))):
        set_base(render, base)
        assert_words(render.read_nodes(render.edit_nodes(c, 7, col)), want, f"{type(c)} {c.dtype}")
    ms = own_gpu.edit_timing()
    assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[1] > 0 and ms[5] > 0


def raw_edit(pkg, gpu, xyz, depth, n_words, max_words=0, n=None):
    p = pkg._lib.EditParams()
    p.depth, p.default_colour, p.n_words, p.max_words = depth, 0xFFFFFF, n_words, max_words
    out = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_nodes_edit(gpu._h, xyz.data_ptr() if xyz is not None else None, None,
                                       xyz.shape[0] if n is None else n, C.byref(p), C.byref(out))
    gpu.sync()
    return rc, out.value


def test_errors_write_nothing(pkg, render, own_gpu, base6):
    import torch
    coords, base = base6
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    dev = torch.device("cuda", own_gpu.device)
    last_error = lambda: pkg._lib.lib().svo_last_error(own_gpu._h).decode()  # noqa: E731
    t = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)  # noqa: E731

    # depth 4 into a region the depth-6 base refines: refused, naming the voxel
    far = [15, 15, 15]  # (the base's voxels lie below 40 = cell 10 at depth 4: an empty leaf)
    refused = np.array([far, coords[7] >> 2, [0, 15, 0]])
    with pytest.raises(E.Refused) as e:
        E.edit(base, base.size, refused, 4)
    assert e.value.index == 1
    assert raw_edit(pkg, own_gpu, t(refused), 4, base.size)[0] == ERR_STATE
    assert "voxel 1 " in last_error() and "interior" in last_error()
    with pytest.raises(pkg.SvoError):
        render.edit_nodes(refused, 4)
    assert render.node_length == base.size

    ok = t([[1, 2, 3], [63, 63, 63]])
    assert raw_edit(pkg, own_gpu, t([[1, 2, 3], [64, 0, 0]]), 6, base.size)[0] == ERR_ARG
    assert "outside" in last_error()
    assert raw_edit(pkg, own_gpu, t([[1, 2, 3], [0, -1, 0]]), 6, base.size)[0] == ERR_ARG
    assert raw_edit(pkg, own_gpu, ok, 0, base.size)[0] == ERR_ARG
    assert raw_edit(pkg, own_gpu, ok, 22, base.size)[0] == ERR_ARG
    assert raw_edit(pkg, own_gpu, ok, 6, 12)[0] == ERR_ARG
    assert raw_edit(pkg, own_gpu, ok, 6, 0)[0] == ERR_ARG
    assert raw_edit(pkg, own_gpu, ok, 6, CAPACITY + 8)[0] == ERR_ARG
    assert raw_edit(pkg, own_gpu, None, 6, base.size, n=5)[0] == ERR_ARG
    assert raw_edit(pkg, own_gpu, ok, 6, base.size, n=1 << 31)[0] == ERR_ARG
    # the cap: one group short fails, exactly reached succeeds (below)
    grow = np.array([[63, 63, 63], [62, 1, 60]])
    want = E.edit(base, base.size, grow, 6)
    assert want.size >= base.size + 16
    assert raw_edit(pkg, own_gpu, t(grow), 6, base.size, max_words=want.size - 8)[0] == ERR_CAP
    assert str(want.size) in last_error()
    with pytest.raises(pkg.SvoError):
        render.edit_nodes(grow, 6, max_words=want.size - 8)
    assert raw_edit(pkg, own_gpu, ok[:0], 6, base.size) == (0, base.size)  # nothing to edit
    assert render.edit_nodes(np.zeros((0, 3), dtype=np.int64), 6) == base.size
    assert render.node_length == base.size
    assert np.array_equal(render.read_nodes(base.size + PAD), before)

    assert raw_edit(pkg, own_gpu, t(grow), 6, base.size, max_words=want.size) == (0, want.size)
    assert_words(render.read_nodes(want.size), want, "the cap exactly reached")
    fresh = pkg.Gpu(0)
    try:
        assert raw_edit(pkg, fresh, ok, 6, 8)[0] == ERR_STATE
    finally:
        fresh.close()


def test_timing_keeps_the_last_edit_that_ran(pkg, render, own_gpu, base6):
    import torch
    coords, base = base6
    rng = np.random.default_rng(77)
    ec, ecol = edit_voxels(rng, 7, 3000, coords, 1)
    set_base(render, base)
    assert render.edit_nodes(ec, 7, ecol) > base.size  # (its times are not fetched)
    # a refused call records the front end's events again: the accepted edit's times are taken before it does
    set_base(render, base)
    refused = torch.tensor(np.array([[15, 15, 15], coords[7] >> 2, [0, 15, 0]]), dtype=torch.int32,
                           device=torch.device("cuda", own_gpu.device))
    assert raw_edit(pkg, own_gpu, refused, 4, base.size)[0] == ERR_STATE
    ms = own_gpu.edit_timing()
    assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[1] > 0 and ms[5] > 0
    assert ms == own_gpu.edit_timing()
    assert raw_edit(pkg, own_gpu, refused, 4, base.size)[0] == ERR_STATE
    assert ms == own_gpu.edit_timing()


def frame(pkg, r, u):
    set_uniforms_from_oracle(r, u)
    got = pkg.render.hits_to_numpy(r.render())
    r.gpu.sync()
    return got


def monu9_edits(coords, depth):
    """a carved block (colour 0 over every cell of a box around the model's middle voxel) and a few hundred voxels one
    level deeper inside the emptied box"""
    mid = np.sort(coords, axis=0)[len(coords) // 2]
    lo = np.clip(mid - 20, 0, (1 << depth) - 40)
    box = np.stack(np.meshgrid(*[np.arange(40)] * 3, indexing="ij"), -1).reshape(-1, 3) + lo
    rng = np.random.default_rng(77)
    deeper = 2 * (lo + 8) + rng.integers(0, 48, (400, 3))
    return box, deeper, rng.integers(1, 1 << 24, 400)


def test_edited_trees_trace_like_the_oracle(pkg, O):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    (label, size, xyzi, pal), = B.fixture_models(GOLDEN, "monu9")
    coords, colours, depth = B.vox_voxels(size, xyzi, pal)
    box, deeper, deeper_colours = monu9_edits(coords, depth)
    g1, g2 = pkg.Gpu(0), pkg.Gpu(0)
    try:
        r1 = pkg.Render.from_voxels(g1, (64, 64), coords, depth, colours, capacity=CAPACITY)
        base = r1.read_nodes()
        u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
        hits_base = O.trace_frame(base, u, threads=4)
        assert_hits_equal(frame(pkg, r1, u), hits_base, "monu9 as built")

        carved = E.edit(base, base.size, box, depth, np.zeros(len(box), dtype=np.int64))
        assert r1.edit_nodes(box, depth, np.zeros(len(box), dtype=np.int64)) == carved.size
        assert_words(r1.read_nodes(), carved, "carved")
        hits_carved = O.trace_frame(carved, u, threads=4)
        assert (hits_carved["value"] != hits_base["value"]).sum() > 50
        for variant in (pkg.gpu.VARIANT_STACK, pkg.gpu.VARIANT_RESTART):
            g1.set_option(pkg.gpu.OPT_VARIANT, variant)
            assert_hits_equal(frame(pkg, r1, u), hits_carved, f"carved, variant {variant}")

        # one level deeper, through a second context that shares the store; traced through the first
        r2 = pkg.Render.share_nodes(g2, r1)
        filled = E.edit(carved, carved.size, deeper, depth + 1, deeper_colours)
        assert r2.edit_nodes(deeper, depth + 1, deeper_colours) == filled.size
        g2.sync()
        r1.node_length = r2.node_length
        assert_words(r1.read_nodes(), filled, "filled")
        hits_filled = O.trace_frame(filled, u, threads=4)
        assert (hits_filled["value"] != hits_carved["value"]).sum() > 10
        for variant in (pkg.gpu.VARIANT_RESTART, pkg.gpu.VARIANT_STACK):
            g1.set_option(pkg.gpu.OPT_VARIANT, variant)
            assert_hits_equal(frame(pkg, r1, u), hits_filled, f"filled through the sharing context, variant {variant}")
        assert_hits_equal(frame(pkg, r2, u), hits_filled, "filled, on the context that edited")
    finally:
        g2.close()
        g1.close()
