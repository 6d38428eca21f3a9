"""Trees edited by shapes on the GPU (csrc/svo_region.hip): word for word against the rule's restatement
(tests/region_ref.py: edit) and cell for cell against the per-cell contract (apply_cells) on the depth-7 base of the pass
tests; nothing written behind the new length, on an error or by a second identical call; the same bytes on every run; the
edges of the arguments (depth 1, radius 0, 1 024 shapes, depth 21 at the full range of the 64-bit arithmetic); frames traced
from an edited tree against the oracle, also when the edit came through a context that shares the buffer."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import edit_ref as E
import region_ref as R
import sample_ref as S
from conftest import assert_hits_equal, load_vox_fixture
from pass_frame import assert_words, last_error, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, ERR_ARG, ERR_CAP, ERR_STATE, PAD, ROOT, frame, poison, set_base

pytestmark = pytest.mark.gpu

WHOLE7 = ((0, 0, 0), (128, 128, 128))


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def base7():
    """the depth-7 base and its whole grid as the sampler's restatement gives it (computed once; nobody writes to them)"""
    base = tree7_base()["base"]
    return base, S.sample_dense(base, base.size, *WHOLE7, 7)


def to_shapes(pkg, records):
    """the reference's records (half cells) as the package's shapes (cells)"""
    out = []
    for r in R.shapes(records).astype(np.int64).tolist():
        kind, mode = r[0] & 0xFFFF, r[0] >> 16
        if kind == R.BOX:
            out.append(pkg.region.box(r[2:5], r[5:8], r[1], mode))
        else:
            out.append(pkg.region.ball([v / 2 for v in r[2:5]], r[5] / 2, r[1], mode))
    return out


def check_region(pkg, render, base, records, depth, what, runs=2):
    """base -> edit_region on the GPU == region_ref.edit, the words behind the new length keep what they held, and a second
    run from the same base gives the same bytes.  Returns (the words, the reference's tallies)"""
    want, tally = R.edit(base, base.size, R.shapes(records), depth)
    growth = want.size - base.size
    assert growth == 8 * tally["splits"]
    shapes = to_shapes(pkg, records)
    for run in range(runs):
        set_base(render, base, growth)
        n = render.edit_region(shapes, depth)
        assert n == want.size == render.node_length, f"{what}: length {n}, want {want.size}"
        got = render.read_nodes(n + PAD)
        assert_words(got[:n], want, f"{what}, run {run}")
        assert np.array_equal(got[n:], poison(growth + PAD)[growth:]), f"{what}: words behind the new length were written"
    return want, tally


def sampled(render, depth):
    side = 1 << depth
    return render.sample_dense((0, 0, 0), (side,) * 3, depth).cpu().numpy().view(np.uint32)


# the tallies that the case must show (each non-zero in the reference, so the case proves that it happened)
SHOWS = {"carve ball": ("collapses",), "fill ball": ("splits", "collapses", "overwrites"), "paint box": ("overwrites", "opened"),
         "flood box": ("splits", "overwrites"), "stroke": ("splits", "collapses"), "whole grid": ("collapses",)}


@pytest.mark.parametrize("name", list(SHOWS))
def test_the_table_cases(pkg, render, base7, name):
    base, grid = base7
    records = R.table_cases()[name]
    want, tally = check_region(pkg, render, base, records, 7, name)
    for key in SHOWS[name]:
        assert tally[key] > 0, (name, key, tally)
    if name in ("carve ball", "whole grid"):
        assert want.size == base.size
    if name == "flood box":
        assert tally["splits"] > 4096  # (a level's frontier and its splits go beyond one scan tile)
    if name == "whole grid":
        assert tally["collapses"] == 8 and (want[:8] == (B.VOXEL_OFFSET + 0x777777) << 4).all()
    assert np.array_equal(sampled(render, 7), R.apply_cells(grid, 7, R.shapes(records))), f"{name}: the cells"
    if name == "stroke":  # the order of the shapes is part of the input
        back, _ = check_region(pkg, render, base, records[::-1], 7, "stroke, reversed", runs=1)
        assert not np.array_equal(sampled(render, 7), R.apply_cells(grid, 7, R.shapes(records)))


def test_depth_1_and_2_on_the_empty_root(pkg, render):
    want, tally = check_region(pkg, render, ROOT, [R.box((0, 0, 0), (2, 1, 2), 0x010203), R.ball((3, 3, 3), 0, 0x0A0B0C)], 1, "depth 1")
    assert want.size == 8 and tally["overwrites"] == 5
    want, tally = check_region(pkg, render, ROOT, [R.box((1, 0, 2), (3, 4, 4), 0x010203), R.ball((4, 4, 4), 2, 0x0A0B0C, R.MODE_EMPTY)], 2, "depth 2")
    assert tally["splits"] > 0 and np.array_equal(sampled(render, 2), R.apply_cells(np.zeros((4, 4, 4), dtype=np.uint32), 2, R.shapes(
        [R.box((1, 0, 2), (3, 4, 4), 0x010203), R.ball((4, 4, 4), 2, 0x0A0B0C, R.MODE_EMPTY)])))
    # a carve of the whole depth-2 grid takes the root group back to eight empty words
    check_region(pkg, render, want, [R.box((0, 0, 0), (4, 4, 4), 0)], 2, "depth 2, carved")


def test_a_ball_of_radius_0(pkg, render, base7):
    base, grid = base7
    empty = np.argwhere(grid == 0)[1234]
    odd = [R.ball((2 * empty + 1).tolist(), 0, 0x00FF00)]
    want, tally = check_region(pkg, render, base, odd, 7, "radius 0, odd centre")
    cells = R.apply_cells(grid, 7, R.shapes(odd))
    assert (cells != grid).sum() == 1 and cells[tuple(empty)] == 0x00FF00 and np.array_equal(sampled(render, 7), cells)
    even = [R.ball((2 * empty).tolist(), 0, 0x00FF00)]
    want, tally = check_region(pkg, render, base, even, 7, "radius 0, even centre")
    assert np.array_equal(want, base) and tally["splits"] == tally["overwrites"] == tally["collapses"] == 0


def many_shapes(n, depth):
    rng = np.random.default_rng(n)
    side = 1 << depth
    recs = []
    for k in range(n):
        if k % 2:
            lo = rng.integers(0, side - 6, 3)
            recs.append(R.box(lo.tolist(), (lo + rng.integers(1, 7, 3)).tolist(), int(rng.integers(0, 1 << 24)), int(rng.integers(1, 4))))
        else:
            recs.append(R.ball(rng.integers(0, 2 * side + 1, 3).tolist(), int(rng.integers(0, 9)), int(rng.integers(0, 1 << 24)), int(rng.integers(1, 4))))
    return recs


def test_1024_shapes_fill_the_staging_and_1025_are_refused(pkg, render, own_gpu):
    rng = np.random.default_rng(1024)
    base = B.build(rng.integers(0, 8, (100, 3)) * 2, 4, rng.integers(1, 1 << 24, 100))  # a small grid: the shapes are the point
    grid = S.sample_dense(base, base.size, (0, 0, 0), (16,) * 3, 4)
    recs = many_shapes(1024, 4)
    want, tally = check_region(pkg, render, base, recs, 4, "1 024 shapes", runs=1)
    assert tally["splits"] > 0 and tally["overwrites"] > 0 and tally["collapses"] > 0
    assert np.array_equal(sampled(render, 4), R.apply_cells(grid, 4, R.shapes(recs)))
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    assert raw_region(pkg, own_gpu, recs + recs[:1], 4, base.size)[0] == ERR_ARG and "1025" in last_error(pkg, own_gpu)
    assert np.array_equal(render.read_nodes(base.size + PAD), before)


def test_depth_21_at_the_full_range(pkg, render):
    import math
    top = (1 << 21) - 1
    chain = E.edit(ROOT, 8, [[top, 5, 1234567]], 21, [0x00FF00])
    assert chain.size == 8 * 21
    # two balls that cover every cell of the grid, at the limits of the arguments: radius 2^23 around the far corner, and
    # around the near corner the smallest radius that still holds the far corner cell's centre, 3 * (2^22 - 1)^2 <= r^2 (a
    # sum of three terms of 44 bits).  In VOXELS mode they follow the chain down and paint the one voxel, the second last.
    # One box one cell wide splits 20 coarse leaves, another fills the voxel's empty neighbour in its group
    corner = 3 * (2 * top + 1) ** 2
    exact = math.isqrt(corner) + (math.isqrt(corner) ** 2 < corner)
    assert (exact - 1) ** 2 < corner <= exact ** 2 and exact <= 1 << 23
    recs = [R.ball((1 << 22, 1 << 22, 1 << 22), 1 << 23, 0x0000FF, R.MODE_VOXELS), R.ball((0, 0, 0), exact, 0x0000EE, R.MODE_VOXELS),
            R.box((0, 0, 0), (1, 1, 1), 0x123456), R.box((top, 5, 1234566), (top + 1, 6, 1234567), 0xABCDEF, R.MODE_EMPTY)]
    want, tally = check_region(pkg, render, chain, recs, 21, "depth 21")
    assert tally["splits"] == 20 and tally["opened"] == 20 and tally["overwrites"] == 3
    cells = np.array([[top, 5, 1234567], [0, 0, 0], [top, 5, 1234566], [1, 0, 0], [top, 5, 1234565]])
    assert render.sample_voxels(cells, 21).cpu().numpy().tolist() == [0x0000EE, 0x123456, 0xABCDEF, 0, 0]
    # one half cell less and the far corner cell is outside: the same ball is PART at the root and would follow its whole
    # surface down, so it is only classified here, by the reference, against the two deepest cubes at the corner
    short = R.ball((0, 0, 0), exact - 1, 1)
    assert R.classify(short, [[top, top, top]], 0).tolist() == [R.OUT] and R.classify(short, [[top >> 1] * 3], 1).tolist() == [R.PART]
    assert R.classify(recs[1], [[top, top, top]], 0).tolist() == [R.FULL]


def test_untouched_words_keep_their_counters(pkg, render, base7):
    base, grid = base7
    rng = np.random.default_rng(33)
    counted = base | rng.integers(1, 16, base.size).astype(np.uint32)
    want, tally = check_region(pkg, render, counted, R.table_cases()["fill ball"], 7, "base with hit counters", runs=1)
    kept = want[: base.size] == counted
    assert kept.sum() > base.size // 2 and (~kept).sum() > 1000 and (want[: base.size][~kept] & 15 == 0).all()
    assert (want[base.size:] & 15 == 0).all()


def test_an_identical_second_call_writes_nothing(pkg, render, base7):
    base, grid = base7
    records = R.table_cases()["stroke"]
    first, _ = check_region(pkg, render, base, records, 7, "stroke", runs=1)
    whole = render.read_nodes(first.size + PAD)
    assert render.edit_region(to_shapes(pkg, records), 7) == first.size
    assert np.array_equal(render.read_nodes(first.size + PAD), whole)
    ms = render.gpu.region_timing()
    assert len(ms) == 5 and all(t >= 0 for t in ms) and ms[0] > 0 and ms[4] > 0
    assert render.edit_region([], 7) == first.size and render.gpu.region_timing() == [0.0] * 5


def test_compaction_shrinks_the_carved_tree(pkg, render, base7):
    base, grid = base7
    records = R.table_cases()["carve ball"]
    carved, tally = check_region(pkg, render, base, records, 7, "carve ball", runs=1)
    assert render.compact_nodes(prune=True) < carved.size
    coords, colours = render.list_voxels(7, expand=True)
    cells = R.apply_cells(grid, 7, R.shapes(records))
    want = np.argwhere(cells != 0)
    order = np.argsort(B.morton(want, 7), kind="stable")
    assert np.array_equal(coords.cpu().numpy(), want[order]) and np.array_equal(colours.cpu().numpy().view(np.uint32), cells[tuple(want[order].T)])


def raw_region(pkg, gpu, records, depth, n_words, max_words=0, n=None, shapes=True, params=True, out=True):
    sh = R.shapes(records).astype(np.int64).tolist()
    arr = (pkg._lib.RegionShape * max(len(sh), 1))()
    for a, r in zip(arr, sh):
        a.kind, a.mode, a.colour, a.a, a.b = r[0] & 0xFFFF, r[0] >> 16, r[1], (C.c_uint32 * 3)(*r[2:5]), (C.c_uint32 * 3)(*r[5:8])
    p = pkg._lib.RegionParams()
    p.depth, p.n_words, p.max_words = depth, n_words, max_words
    n_out = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_nodes_edit_region(gpu._h, arr if shapes else None, len(sh) if n is None else n, C.byref(p) if params else None,
                                              C.byref(n_out) if out else None)
    gpu.sync()
    return rc, n_out.value


def test_errors_write_nothing(pkg, render, own_gpu, base7):
    base, grid = base7
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    err = lambda: last_error(pkg, own_gpu)  # noqa: E731
    ok = [R.box((0, 0, 0), (8, 8, 8), 1)]

    def refused(code, records, depth=7, n_words=base.size, **kw):
        assert raw_region(pkg, own_gpu, records, depth, n_words, **kw)[0] == code, (records, kw, err())
        return err()

    assert "null params" in refused(ERR_ARG, ok, params=False)
    assert "n_words_out" in refused(ERR_ARG, ok, out=False)
    assert "null shapes" in refused(ERR_ARG, ok, shapes=False)
    assert "depth must be 1..21" in refused(ERR_ARG, ok, depth=0)
    assert "depth must be 1..21" in refused(ERR_ARG, ok, depth=22)
    assert "shape 1: unknown kind 2" in refused(ERR_ARG, ok + [[2 | 3 << 16, 0, 0, 0, 0, 1, 1, 1]])
    assert "shape 0: mode" in refused(ERR_ARG, [[0, 0, 0, 0, 0, 1, 1, 1]])
    assert "mode" in refused(ERR_ARG, [[1 | 4 << 16, 0, 0, 0, 0, 1, 0, 0]])
    assert "lo < hi" in refused(ERR_ARG, [R.box((3, 0, 0), (3, 1, 1), 1)])
    assert "axis 1" in refused(ERR_ARG, [R.box((0, 0, 0), (1, 129, 1), 1)])
    assert "centre" in refused(ERR_ARG, [R.ball((0, 0, 257), 1, 1)])
    assert "radius" in refused(ERR_ARG, [R.ball((0, 0, 256), (1 << 23) + 1, 1)])
    for n_words in (0, 12, CAPACITY + 8):
        assert "n_words must be a positive multiple of 8" in refused(ERR_ARG, ok, n_words=n_words)
    # the tree is interior at depth 5 under a shape that does not replace it: refused, naming the shape and the cell
    paint = [R.box((20, 20, 20), (21, 21, 21), 5, R.MODE_EMPTY), R.box((0, 0, 0), (32, 32, 32), 7, R.MODE_VOXELS)]
    with pytest.raises(R.Refused) as e:
        R.edit(base, base.size, R.shapes(paint), 5)
    assert e.value.shape == 1
    message = refused(ERR_STATE, paint, depth=5)
    assert "shape 1 meets cell (%d, %d, %d)" % e.value.cell in message and "interior node at depth 5" in message
    with pytest.raises(pkg.SvoError):
        render.edit_region(to_shapes(pkg, paint), 5)
    assert render.node_length == base.size
    # the cap: one group short of the reference's length fails, exactly reached succeeds (below)
    fill = R.table_cases()["fill ball"]
    want, _ = R.edit(base, base.size, R.shapes(fill), 7)
    assert want.size > base.size
    assert str(want.size) in refused(ERR_CAP, fill, max_words=want.size - 8)
    with pytest.raises(pkg.SvoError):
        render.edit_region(to_shapes(pkg, fill), 7, max_words=want.size - 8)
    assert raw_region(pkg, own_gpu, [], 7, base.size) == (0, base.size)  # nothing to edit
    assert render.edit_region([pkg.region.box((200, 0, 0), (300, 5, 5), 1)], 7) == base.size  # (clipped away)
    assert render.node_length == base.size
    assert np.array_equal(render.read_nodes(base.size + PAD), before)
    assert raw_region(pkg, own_gpu, fill, 7, base.size, max_words=want.size) == (0, want.size)
    assert_words(render.read_nodes(want.size), want, "the cap exactly reached")

    # malformed trees, with the compaction's wording; a painting box over the whole grid opens every interior word
    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice"}
    cases = malformed_cases()
    for name, part in causes.items():
        words = cases[name]
        set_base(render, words)
        held = render.read_nodes(words.size + PAD)
        message = refused(ERR_STATE, [R.box((0, 0, 0), (32, 32, 32), 7, R.MODE_VOXELS)], depth=5, n_words=words.size)
        assert "malformed tree" in message and part in message, (name, message)
        assert np.array_equal(render.read_nodes(words.size + PAD), held), name

    fresh = pkg.Gpu(0)
    try:
        assert raw_region(pkg, fresh, ok, 7, 8)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
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
        assert raw_region(pkg, g, ok, 7, r.node_length)[0] == ERR_STATE and "adaptive" in last_error(pkg, g)
        assert np.array_equal(r.read_nodes(), held)
        del attached
    finally:
        g.close()


def test_an_edited_tree_traces_like_the_oracle(pkg, O, base7):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base, grid = base7
    fill = R.table_cases()["fill ball"]
    filled, _ = R.edit(base, base.size, R.shapes(fill), 7)
    flooded, _ = R.edit(filled, filled.size, R.shapes(R.table_cases()["flood box"]), 7)
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    hits_base, hits_filled, hits_flooded = (O.trace_frame(w, u, threads=4) for w in (base, filled, flooded))
    assert (hits_filled["value"] != hits_base["value"]).sum() > 50
    g1, g2 = pkg.Gpu(0), pkg.Gpu(0)
    try:
        r1 = pkg.Render(g1, (64, 64), base, capacity=CAPACITY)
        assert_hits_equal(frame(pkg, r1, u), hits_base, "the base")
        assert r1.edit_region(to_shapes(pkg, fill), 7) == filled.size
        assert_words(r1.read_nodes(), filled, "filled")
        assert_hits_equal(frame(pkg, r1, u), hits_filled, "the filled ball")
        # the next edit through a second context that shares the store; traced through the first
        r2 = pkg.Render.share_nodes(g2, r1)
        assert r2.edit_region(to_shapes(pkg, R.table_cases()["flood box"]), 7) == flooded.size
        g2.sync()
        r1.node_length = r2.node_length
        assert_words(r1.read_nodes(), flooded, "flooded through the sharing context")
        assert_hits_equal(frame(pkg, r1, u), hits_flooded, "flooded, on the context that did not edit")
        assert_hits_equal(frame(pkg, r2, u), hits_flooded, "flooded, on the context that edited")
    finally:
        g2.close()
        g1.close()
