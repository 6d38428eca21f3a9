"""Trees shaped by a height map on the GPU (csrc/svo_heightmap.hip): word for word against the rule's restatement
(tests/heightmap_ref.py: edit) and cell for cell against the per-cell contract (apply_cells) on the depth-7 base of the pass
tests; nothing written behind the new length, on an error or by a second identical call; the same bytes on every run; the
min/max pyramid level by level against its restatement, with sentinels behind the output; the edges of the arguments (depth
1, depth 21 with 64-bit layer sums, heights above the grid); a depth-9 terrain made from the empty root and read back by
column_tops; frames traced from a terraformed tree against the oracle, through a context that shares the buffer.
The pyramid of the 512 x 512 map at an odd origin of the depth-10 grid takes two launches: the levels 1..6, then 7..10."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import heightmap_ref as H
import sample_ref as S
from conftest import assert_hits_equal, load_vox_fixture
from pass_frame import SENTINEL, SLACK, SentinelOut, assert_words, last_error, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, ERR_ARG, ERR_CAP, ERR_STATE, PAD, ROOT, frame, poison, set_base
from test_heightmap_host import SHOWS

pytestmark = pytest.mark.gpu

WHOLE7 = ((0, 0, 0), (128, 128, 128))


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def bases():
    """the depth-7 base and the empty root with their whole grids as the sampler's restatement gives them (computed once;
    nobody writes to them)"""
    base = tree7_base()["base"]
    return {"base7": (base, S.sample_dense(base, base.size, *WHOLE7, 7)), "root": (ROOT, np.zeros((128,) * 3, dtype=np.uint32))}


def edit_on_gpu(render, heights, origin, depth, p, **kw):
    return render.edit_heightmap(heights, p["layers"], origin, depth, below=p["below"], above=p["above"], above_colour=p["above_colour"], **kw)


def check_heightmap(render, base, heights, origin, depth, p, what, runs=2):
    """base -> edit_heightmap on the GPU == heightmap_ref.edit, the words behind the new length keep what they held, and a
    second run from the same base gives the same bytes.  Returns (the words, the reference's tallies)"""
    want, tally = H.edit(base, base.size, heights, origin, depth, p)
    growth = want.size - base.size
    assert growth == 8 * tally["splits"]
    for run in range(runs):
        set_base(render, base, growth)
        n = edit_on_gpu(render, heights, origin, depth, p)
        assert n == want.size == render.node_length, f"{what}: length {n}, want {want.size}"
        got = render.read_nodes(n + PAD)
        assert_words(got[:n], want, f"{what}, run {run}")
        assert np.array_equal(got[n:], poison(growth + PAD)[growth:]), f"{what}: words behind the new length were written"
    return want, tally


def sampled(render, depth):
    side = 1 << depth
    return render.sample_dense((0, 0, 0), (side,) * 3, depth).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(SHOWS))
def test_the_table_cases(pkg, render, bases, name):
    which, heights, origin, p = H.table_cases()[name]
    base, grid = bases[which]
    want, tally = check_heightmap(render, base, heights, origin, 7, p, name)
    for key in SHOWS[name]:
        assert tally[key] > 0, (name, key, tally)
    if name == "terraform":
        assert max(tally["level_splits"]) > 4096  # (a level's frontier and its splits go beyond one scan tile)
    if name == "flat":
        assert want.size == 8 and tally["overwrites"] == 4
    assert np.array_equal(sampled(render, 7), H.apply_cells(grid, 7, heights, origin, p)), f"{name}: the cells"
    # an identical second call writes nothing and appends nothing
    whole = render.read_nodes(want.size + PAD)
    assert edit_on_gpu(render, heights, origin, 7, p) == want.size
    assert np.array_equal(render.read_nodes(want.size + PAD), whole)
    ms = render.gpu.heightmap_timing()
    assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[0] > 0 and ms[1] > 0 and ms[5] > 0


@pytest.fixture
def fresh_gpu(pkg, own_gpu):
    """a context for a Render of the test's own: a second Render on own_gpu would replace the module's node buffer"""
    g = pkg.Gpu(0)
    yield g
    g.close()


def test_from_heightmap_and_a_device_tensor(pkg, fresh_gpu, bases):
    import torch
    which, heights, origin, p = H.table_cases()["empty root"]
    want, tally = H.edit(ROOT, 8, heights, origin, 7, p)
    on_device = torch.as_tensor(heights.astype(np.int32), device=fresh_gpu.torch_device)
    r = pkg.Render.from_heightmap(fresh_gpu, (64, 64), on_device, 7, p["layers"], capacity=want.size + PAD)
    assert r.node_length == want.size
    assert_words(r.read_nodes(), want, "from_heightmap")
    assert np.array_equal(sampled(r, 7), H.apply_cells(bases["root"][1], 7, heights, origin, p))


def raw_minmax(pkg, gpu, heights, origin, depth, s, out_ptr, size=None, reserved=0):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(heights).astype(np.uint32).view(np.int32), device=gpu.torch_device)
    torch.cuda.current_stream(gpu.torch_device).synchronize()
    p = pkg._lib.HeightmapParams()
    p.depth, p.reserved = depth, reserved
    p.origin_xz[:] = list(origin)
    p.size_xz[:] = list(heights.shape if size is None else size)
    rc = pkg._lib.lib().svo_heightmap_minmax(gpu._h, C.byref(p), t.data_ptr() if t.numel() else None, s, out_ptr)
    gpu.sync()
    return rc


PYRAMIDS = {"67 x 50": ((67, 50), (5, 9), 7), "60 x 72, rows of whole quads": ((60, 72), (4, 8), 7), "1 x N": ((1, 97), (127, 13), 7),
            "N x 1": ((83, 1), (2, 64), 7), "1 x 1": ((1, 1), (63, 64), 7), "512 x 512 at an odd origin": ((512, 512), (301, 77), 10),
            "512 x 512, aligned": ((512, 512), (0, 512), 10)}


@pytest.mark.parametrize("name", list(PYRAMIDS))
def test_the_pyramid_level_by_level(pkg, render, own_gpu, name):
    (sx, sz), origin, depth = PYRAMIDS[name]
    rng = np.random.default_rng(sx * sz)
    heights = rng.integers(0, (1 << depth) + 40, (sx, sz))
    heights[rng.integers(0, sx), rng.integers(0, sz)] = 0xFFFFFFFF
    for s in range(1, depth + 1):
        want = H.pyramid(heights, origin, depth, s)
        out = SentinelOut(own_gpu, [want.size + SLACK])
        assert raw_minmax(pkg, own_gpu, heights, origin, depth, s, out.t[0].data_ptr()) == 0, last_error(pkg, own_gpu)
        got = out.host()[0]
        assert np.array_equal(got[: want.size].reshape(want.shape), want), (name, s)
        assert out.untouched_from(want.size), (name, s)
    got = render.height_minmax(heights, depth, origin, depth).cpu().numpy().view(np.uint32)
    assert got.shape == (1, 1, 2) and got[0, 0].tolist() == [min(int(heights.min()), 1 << depth), 1 << depth]
    assert np.array_equal(render.height_minmax(heights, 2, origin, depth).cpu().numpy().view(np.uint32), H.pyramid(heights, origin, depth, 2))


def test_the_refusal_names_the_cell_and_set_collapses(pkg, render, own_gpu, bases):
    base, grid = bases["base7"]
    heights = H.terrain(64, 64, 5, 40)
    p = H.params(H.TERRAIN, "empty", None)
    with pytest.raises(H.Refused) as e:
        H.edit(base, base.size, heights, (0, 0), 6, p)
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    with pytest.raises(pkg.SvoError):
        edit_on_gpu(render, heights, (0, 0), 6, p)
    message = last_error(pkg, own_gpu)
    assert "meets cell (%d, %d, %d)" % e.value.cell in message and "interior node at depth 6" in message
    assert render.node_length == base.size and np.array_equal(render.read_nodes(base.size + PAD), before)
    want, tally = check_heightmap(render, base, heights, (0, 0), 6, H.params(H.TERRAIN, "set", "set", 0), "depth 6 over the depth-7 base", runs=1)
    assert tally["collapses"] > 1000 and tally["opened"] > 0


def test_depth_1_and_heights_above_the_grid(pkg, render, bases):
    want, tally = check_heightmap(render, ROOT, np.array([[1]]), (0, 0), 1, H.params([(0, 0x010203)]), "depth 1")
    assert want.size == 8 and tally["overwrites"] == 1 and want[0] == (B.VOXEL_OFFSET + 0x010203) << 4
    base, grid = bases["base7"]
    heights = np.array([[0xFFFFFFFF, 129, 128], [127, 0, 0x80000000]], dtype=np.uint64)
    p = H.params(H.TERRAIN, "set", "set", 0)
    check_heightmap(render, base, heights, (125, 3), 7, p, "heights above the grid", runs=1)
    cells = H.apply_cells(grid, 7, heights, (125, 3), p)
    assert (cells[125, :, 3] != 0).all() and (cells[125, :, 5] != 0).all() and cells[126, 127, 3] == 0 and (cells[126, :, 4] == 0).all()
    assert np.array_equal(sampled(render, 7), cells)


def test_depth_21_with_64_bit_layer_sums(pkg, render):
    top = 1 << 21
    heights = np.array([[64, 3, 17, 0, 1], [2, 40, 5, 64, 9], [33, 0, 7, 12, 21]])
    layers = [(3, 0x00FF00), (0xFFFFFFFF, 0x0000FF), (0xFFFFFFFF, 0xFF0000), (0, 0x777777)]  # (sums of 32 bits would wrap to 2 and 1)
    p = H.params(layers)
    want, tally = check_heightmap(render, ROOT, heights, (top - 3, top - 5), 21, p, "depth 21")
    assert want.size < 100_000 and tally["splits"] >= 20
    i, y, k = (a.reshape(-1) for a in np.meshgrid(np.arange(3), np.arange(70), np.arange(5), indexing="ij"))
    cells = np.stack([top - 3 + i, y, top - 5 + k], axis=1)
    expect = np.where(y < heights[i, k], np.where(heights[i, k] - 1 - y < 3, 0x00FF00, 0x0000FF), 0)
    assert np.array_equal(render.sample_voxels(cells, 21).cpu().numpy(), expect)


def test_a_depth_9_terrain_round_trip(pkg, fresh_gpu):
    heights = H.terrain(512, 512, 20, 300, seed=9)
    heights[100:131, 200:260] = 0
    heights[7, 9] = 512
    p = H.params(H.TERRAIN)
    want, tally = H.edit(ROOT, 8, heights, (0, 0), 9, p)
    r = pkg.Render.from_heightmap(fresh_gpu, (64, 64), heights, 9, p["layers"], capacity=want.size + PAD)
    assert r.node_length == want.size
    assert_words(r.read_nodes(), want, "the depth-9 terrain")
    tops = r.column_tops((0, 0), (512, 512), 9).cpu().numpy()
    assert np.array_equal(tops, heights - 1) and (tops[100:131, 200:260] == pkg.TOP_NONE).all()
    for x0 in (0, 97, 504):
        slab = r.sample_dense((x0, 0, 0), (8, 512, 512), 9).cpu().numpy().view(np.uint32)
        assert np.array_equal(slab, H.apply_columns(np.zeros((8, 512, 512), dtype=np.uint32), 9, heights[x0:x0 + 8], p)), x0


def raw_heightmap(pkg, gpu, heights, origin, depth, n_words, p=None, max_words=0, size=None, reserved=0, modes=None, n_layers=None, params=True, out=True,
                  ptr=True):
    import torch
    p = p or H.params(H.TERRAIN, "set", "set", 0)
    t = torch.as_tensor(np.ascontiguousarray(heights).astype(np.uint32).view(np.int32), device=gpu.torch_device)
    torch.cuda.current_stream(gpu.torch_device).synchronize()
    q = pkg._lib.HeightmapParams()
    q.depth, q.n_words, q.max_words, q.reserved = depth, n_words, max_words, reserved
    q.n_layers = len(p["layers"]) if n_layers is None else n_layers
    q.origin_xz[:] = list(origin)
    q.size_xz[:] = list(heights.shape if size is None else size)
    q.mode_below, q.mode_above = modes or (H.MODES[p["below"]], H.MODES[p["above"]])
    q.colour_above = p["above_colour"]
    for k, (th, colour) in enumerate(p["layers"]):
        q.layers[k].thickness, q.layers[k].colour = th, colour
    n_out = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_nodes_edit_heightmap(gpu._h, C.byref(q) if params else None, t.data_ptr() if ptr and t.numel() else None,
                                                 C.byref(n_out) if out else None)
    gpu.sync()
    return rc, n_out.value


def test_errors_write_nothing(pkg, render, own_gpu, bases):
    base, grid = bases["base7"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    err = lambda: last_error(pkg, own_gpu)  # noqa: E731
    ok = H.terrain(16, 16, 3, 30)

    def refused(code, heights=ok, origin=(0, 0), depth=7, n_words=base.size, **kw):
        assert raw_heightmap(pkg, own_gpu, heights, origin, depth, n_words, **kw)[0] == code, (kw, err())
        return err()

    assert "null params" in refused(ERR_ARG, params=False)
    assert "n_words_out" in refused(ERR_ARG, out=False)
    assert "null heights" in refused(ERR_ARG, ptr=False)
    assert "reserved" in refused(ERR_ARG, reserved=1)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=0)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=22)
    assert "mode" in refused(ERR_ARG, modes=(4, 0))
    assert "mode" in refused(ERR_ARG, modes=(0, 4))
    assert "n_layers" in refused(ERR_ARG, n_layers=9)
    assert "n_layers" in refused(ERR_ARG, n_layers=0)
    assert "axis 0" in refused(ERR_ARG, origin=(113, 0))
    assert "axis 1" in refused(ERR_ARG, origin=(0, 113))
    assert "2^31 columns" in refused(ERR_ARG, depth=21, size=(1 << 16, 1 << 15))
    for n_words in (0, 12, CAPACITY + 8):
        assert "n_words must be a positive multiple of 8" in refused(ERR_ARG, n_words=n_words)
    out = SentinelOut(own_gpu, [64])
    for s in (0, 8):
        assert raw_minmax(pkg, own_gpu, ok, (0, 0), 7, s, out.t[0].data_ptr()) == ERR_ARG and "s must be 1..depth" in err()
    assert raw_minmax(pkg, own_gpu, ok, (0, 0), 7, 1, None) == ERR_ARG and "null minmax_out" in err()
    assert raw_minmax(pkg, own_gpu, ok, (0, 0), 7, 1, out.t[0].data_ptr(), reserved=1) == ERR_ARG
    assert raw_minmax(pkg, own_gpu, ok, (120, 0), 7, 1, out.t[0].data_ptr()) == ERR_ARG
    assert raw_minmax(pkg, own_gpu, ok, (0, 0), 7, 1, out.t[0].data_ptr(), size=(0, 16)) == 0 and out.untouched_from(0)
    # nothing to do: a size with a 0 (no map needed), two modes of 0
    assert raw_heightmap(pkg, own_gpu, ok, (0, 0), 7, base.size, size=(16, 0), ptr=False) == (0, base.size)
    assert raw_heightmap(pkg, own_gpu, ok, (0, 0), 7, base.size, modes=(0, 0)) == (0, base.size)
    assert render.gpu.heightmap_timing() == [0.0] * 6
    # the cap: one group short of the reference's length fails, exactly reached succeeds (below)
    whole = H.table_cases()["raise only"]
    want, _ = H.edit(base, base.size, whole[1], whole[2], 7, whole[3])
    assert want.size > base.size
    assert str(want.size) in refused(ERR_CAP, whole[1], p=whole[3], max_words=want.size - 8)
    with pytest.raises(pkg.SvoError):
        edit_on_gpu(render, whole[1], whole[2], 7, whole[3], max_words=want.size - 8)
    with pytest.raises(ValueError):
        render.edit_heightmap(ok, below="fill")
    with pytest.raises(TypeError):
        render.edit_heightmap(ok.astype(np.float32))
    assert render.node_length == base.size
    assert np.array_equal(render.read_nodes(base.size + PAD), before)
    assert raw_heightmap(pkg, own_gpu, whole[1], whole[2], 7, base.size, p=whole[3], max_words=want.size) == (0, want.size)
    assert_words(render.read_nodes(want.size), want, "the cap exactly reached")

    # malformed trees, with the compaction's wording; a map that repaints over the whole grid opens every interior word
    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice"}
    cases = malformed_cases()
    paint = H.params([(0, 7)], "voxels", "voxels", 9)
    for name, part in causes.items():
        words = cases[name]
        set_base(render, words)
        held = render.read_nodes(words.size + PAD)
        message = refused(ERR_STATE, H.terrain(32, 32, 0, 32), depth=5, n_words=words.size, p=paint)
        assert "malformed tree" in message and part in message, (name, message)
        assert np.array_equal(render.read_nodes(words.size + PAD), held), name

    fresh = pkg.Gpu(0)
    try:
        assert raw_heightmap(pkg, fresh, ok, (0, 0), 7, 8)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
    finally:
        fresh.close()
    # a device adaptive state: subtrees would be cut off under its positions
    size, xyzi, pal, _, _ = load_vox_fixture("monu9")
    world = pkg.adaptive.World(pkg.CpuOctree.from_voxels(size, xyzi, pal))
    octree = world.root_octree()
    g = pkg.Gpu(0)
    try:
        g.set_option(pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, 1)
        r = pkg.Render.new(g, (64, 64), octree, capacity=4096)
        attached = pkg.adaptive.DeviceAdaptive(g, r, octree, world)
        held = r.read_nodes()
        assert raw_heightmap(pkg, g, ok, (0, 0), 7, r.node_length)[0] == ERR_STATE and "adaptive" in last_error(pkg, g)
        assert np.array_equal(r.read_nodes(), held)
        del attached
    finally:
        g.close()


def test_untouched_words_keep_their_counters(pkg, render, bases):
    base, grid = bases["base7"]
    rng = np.random.default_rng(33)
    counted = base | rng.integers(1, 16, base.size).astype(np.uint32)
    which, heights, origin, p = H.table_cases()["rectangle"]
    want, tally = check_heightmap(render, counted, heights, origin, 7, p, "base with hit counters", runs=1)
    kept = want[: base.size] == counted
    assert kept.sum() > base.size // 2 and (~kept).sum() > 1000 and (want[: base.size][~kept] & 15 == 0).all()
    assert (want[base.size:] & 15 == 0).all()


def test_a_terraformed_tree_traces_like_the_oracle(pkg, O, bases):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base, grid = bases["base7"]
    _, heights, origin, p = H.table_cases()["terraform"]
    shaped, _ = H.edit(base, base.size, heights, origin, 7, p)
    _, row, row_origin, row_p = H.table_cases()["row"]
    walled, _ = H.edit(shaped, shaped.size, row, row_origin, 7, row_p)
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    hits_base, hits_shaped, hits_walled = (O.trace_frame(w, u, threads=4) for w in (base, shaped, walled))
    assert (hits_shaped["value"] != hits_base["value"]).sum() > 50
    g1, g2 = pkg.Gpu(0), pkg.Gpu(0)
    try:
        r1 = pkg.Render(g1, (64, 64), base, capacity=CAPACITY)
        assert_hits_equal(frame(pkg, r1, u), hits_base, "the base")
        assert edit_on_gpu(r1, heights, origin, 7, p) == shaped.size
        assert_words(r1.read_nodes(), shaped, "terraformed")
        assert_hits_equal(frame(pkg, r1, u), hits_shaped, "the terraformed tree")
        # the next edit through a second context that shares the store; traced through the first
        r2 = pkg.Render.share_nodes(g2, r1)
        assert edit_on_gpu(r2, row, row_origin, 7, row_p) == walled.size
        g2.sync()
        r1.node_length = r2.node_length
        assert_words(r1.read_nodes(), walled, "edited through the sharing context")
        assert_hits_equal(frame(pkg, r1, u), hits_walled, "on the context that did not edit")
        assert_hits_equal(frame(pkg, r2, u), hits_walled, "on the context that edited")
    finally:
        g2.close()
        g1.close()
