"""A step of morphology on the GPU (csrc/svo_morph.hip): word for word against the rule's restatement
(tests/morph_ref.py: morph) and cell for cell against the per-cell contract (cells) on the cases of the host tests, run twice
from the same base with poison behind the new length; 32 seeded depth-1 patterns; the single voxel of a depth-21 grid; a grow
and a shrink under 6 neighbours against six place_nodes calls from one snapshot; morph_nodes' compositions; shell_nodes against
list_surface, and frames of the shelled ball against the solid one's and the oracle's, also through a sharing context; hit
counters; every error in the header's order with the buffer unchanged; the five times."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import combine_ref as X
import morph_ref as R
import sample_ref as S
from conftest import assert_hits_equal, load_vox_fixture
from pass_frame import assert_words, last_error, own_gpu  # noqa: F401
from test_combine_gpu import sampled
from test_combine_host import leaf
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, ERR_ARG, ERR_CAP, ERR_STATE, PAD, ROOT, frame, poison, set_base
from test_morph_host import CASES, COLOUR, IDS, TILE, grid_of, morphed, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


def check_morph(render, scene, want, op, conn, depth, what, colour=0, open_b=False, runs=2):
    """scene -> one step of morph_nodes on the GPU == `want`, the restatement's words; the words behind the new length keep what
    they held, and a second run from the same scene gives the same bytes"""
    growth = want.size - scene.size
    for run in range(runs):
        set_base(render, scene, growth)
        n = render.morph_nodes(op, 1, conn, colour, depth, open_b)
        assert n == want.size == render.node_length, f"{what}: length {n}, want {want.size}"
        got = render.read_nodes(n + PAD)
        assert_words(got[:n], want, f"{what}, run {run}")
        assert np.array_equal(got[n:], poison(growth + PAD)[growth:]), f"{what}: words behind the new length were written"
    return want


@pytest.mark.parametrize("name,scene,op,conn,colour,open_b", CASES, ids=IDS)
def test_the_host_cases(render, name, scene, op, conn, colour, open_b):
    a, grid, depth = scenes()[scene]
    want, tally = morphed(name)
    check_morph(render, a, want, op, conn, depth, name, colour, open_b)
    if name == "ball: grow 26":  # a level's frontier and its splits go beyond one scan tile, and its groups fill no whole wave
        assert any(n > TILE and s > TILE and (n // 8) % 64 for n, s in tally["levels"]), tally["levels"]
    assert np.array_equal(sampled(render, depth), R.cells(grid, op, conn, colour, open_b)), f"{name}: the cells"


def test_32_patterns_of_depth_1(render):
    rng = np.random.default_rng(131)
    patterns = [0, 255, 1, 128] + rng.integers(1, 255, 28).tolist()
    for i, pattern in enumerate(patterns):
        words = np.array([(leaf(0x101010 * (c + 1)) if pattern >> c & 1 else B.EMPTY) | (c + i) % 16 for c in range(8)], dtype=np.uint32)
        grid = grid_of(words, 1)
        conn, open_b = (6, 18, 26)[i % 3], bool(i & 1)
        for op, colour in (("grow", 0), ("grow", COLOUR), ("shrink", 0)):
            want, tally = R.morph(words, 8, op, conn, 1, colour, open_b)
            check_morph(render, words, want, op, conn, 1, f"pattern {pattern}, {op} {conn}", colour, open_b, runs=1)
            assert want.size == 8 and np.array_equal(sampled(render, 1), R.cells(grid, op, conn, colour, open_b)), (pattern, op, conn)
            # counters: an untouched word keeps its own, a written one has 0
            changed = (want >> 4) != (words >> 4)
            assert np.array_equal(want[~changed], words[~changed]) and (want[changed] & 15 == 0).all() and changed.sum() == tally["overwrites"]


def test_a_single_voxel_in_the_middle_of_a_depth_21_grid(render):
    mid, V = 1 << 20, 0x00C0FFEE
    scene = B.build(np.array([[mid, mid, mid]]), 21, np.array([V]))
    want, tally = R.morph(scene, scene.size, "grow", 26, 21)
    assert tally["splits"] == 501 and want.size == 4176
    check_morph(render, scene, want, "grow", 26, 21, "depth 21")
    around = S.box_cells((mid - 2,) * 3, (5, 5, 5))
    got = render.sample_voxels(around, 21).cpu().numpy().reshape(5, 5, 5)
    assert (got[1:4, 1:4, 1:4] == V).all() and (got != 0).sum() == 27
    # the step back: a shrink of the grown tree leaves the voxel, and appends nothing (every cell is of the last level)
    back, tally = R.morph(want, want.size, "shrink", 26, 21)
    check_morph(render, want, back, "shrink", 26, 21, "depth 21, shrunk", runs=1)
    got = render.sample_voxels(around, 21).cpu().numpy().reshape(5, 5, 5)
    assert back.size == want.size and tally["overwrites"] == 26 and (got != 0).sum() == 1 and got[2, 2, 2] == V


def test_untouched_words_keep_their_counters(render):
    a, _, depth = scenes()["ball"]
    rng = np.random.default_rng(133)
    counted = a | rng.integers(1, 16, a.size).astype(np.uint32)
    for op, conn in (("grow", 18), ("shrink", 6)):
        want = R.morph(counted, counted.size, op, conn, depth)[0]
        plain = R.morph(a, a.size, op, conn, depth)[0]
        check_morph(render, counted, want, op, conn, depth, f"{op} with hit counters", runs=1)
        kept = want[: a.size] == counted
        assert kept.sum() > a.size // 2 and (~kept).sum() > 1000 and (want[: a.size][~kept] & 15 == 0).all() and (want[a.size:] & 15 == 0).all()
        assert np.array_equal(want >> 4, plain >> 4)


@pytest.mark.parametrize("colour", (0, COLOUR))
def test_conn_6_against_six_placements_of_a_snapshot(render, colour):
    """cell c takes the value at c + d: the snapshot moved by -d, under the scene for a grow (the first d by priority fills the
    cell, the later ones find it set) and as a mask for a shrink (keep: only where the moved snapshot holds a voxel, and the cells
    that it does not cover, those at the wall, stay).  A fixed colour recolours what the placements added."""
    for scene in ("mixed5", "ball"):
        a, grid, depth = scenes()[scene]
        room = 8 * 60000
        for op, place_op in (("grow", "under"), ("shrink", "keep")):
            if op == "shrink" and colour:
                continue
            set_base(render, a, room)
            snapshot = render.simplify_nodes(out_of_place=True)
            for d in R.offsets(6):
                render.place_nodes(snapshot, place_op, depth, offset=tuple(-v for v in d))
            by_places = sampled(render, depth)
            if colour:
                by_places = np.where((grid == 0) & (by_places != 0), np.uint32(colour), by_places)
            set_base(render, a, room)
            render.morph_nodes(op, 1, 6, colour, depth)
            got = sampled(render, depth)
            assert np.array_equal(got, by_places) and not np.array_equal(got, grid), (scene, op)
            assert np.array_equal(got, R.cells(grid, op, 6, colour))


def test_morph_nodes_compositions(pkg, render):
    a, grid, depth = scenes()["mixed5"]
    for op, steps, conn, colour, open_b in (("grow", 3, 6, 0, False), ("shrink", 2, 18, 0, True), ("close", 2, 26, COLOUR, False), ("open", 1, 6, 0, False),
                                            ("open", 2, 18, COLOUR, True), ("close", 1, 6, 0, True), ("grow", 0, 26, 0, False)):
        set_base(render, a, 8 * 40000)
        n = render.morph_nodes(op, steps, conn, colour or None, depth, open_b)
        assert n == render.node_length and np.array_equal(sampled(render, depth), R.steps(grid, op, steps, conn, colour, open_b)), (op, steps, conn)
    assert np.array_equal(render.read_nodes(a.size), a)  # (no step: nothing written)
    # three steps are three calls, word for word
    set_base(render, a, 8 * 40000)
    render.morph_nodes("grow", 3, 18, depth=depth)
    whole = render.read_nodes()
    w = a
    for _ in range(3):
        w = R.morph(w, w.size, "grow", 18, depth)[0]
    assert_words(whole, w, "three grows")
    for bad in ({"op": "dilate"}, {"op": "grow", "steps": -1}):
        with pytest.raises(ValueError):
            render.morph_nodes(**bad)
    with pytest.raises(pkg.SvoError):
        render.morph_nodes("grow", conn=8, depth=depth)
    ms = render.gpu.morph_timing()
    assert len(ms) == 5 and all(t >= 0 for t in ms) and ms[0] > 0 and ms[4] > 0


def surface_cells(render, depth, **kw):
    """the cells of the leaves that list_surface reports, as a boolean grid"""
    coords, _, _, levels = (t.cpu().numpy() for t in render.list_surface(depth, with_levels=True, **kw))
    out = np.zeros((1 << depth,) * 3, dtype=bool)
    for (x, y, z), level in zip(coords.tolist(), levels.tolist()):
        s = 1 << (depth - level)
        out[x:x + s, y:y + s, z:z + s] = True
    return out


def test_a_shell_is_the_surface(pkg, render):
    """in a tree whose voxels are all cells of the last level, a built one, list_surface's entries are the voxels with an empty
    cell or the wall behind a face: the shell of thickness 1 under 6 neighbours.  (Of a coarse leaf list_surface reports the whole
    leaf, also where only finer solid detail stands behind a face; the shell keeps its cells that touch an empty one.)"""
    cells = np.concatenate([X.ball_cells(5, (29, 33, 40), 27), S.box_cells((0, 0, 20), (9, 5, 12))])
    built = B.build(cells, 5, np.where(cells[:, 1] < 14, 0x20E0A0, 0xD03060))
    grid = grid_of(built, 5)
    wants = {}
    for closed in (False, True):
        set_base(render, built, 8 * 20000)
        want = wants[closed] = surface_cells(render, 5, closed_boundary=closed)
        n = render.shell_nodes(1, 6, 5, closed_boundary=closed)
        got = sampled(render, 5)
        assert n == render.node_length and np.array_equal(got != 0, want) and np.array_equal(got[want], grid[want])
        assert 0 < want.sum() < (grid != 0).sum()
    assert wants[False][0, 0, 25] and not wants[True][0, 0, 25]  # (a cell of the box in the grid's edge: only the wall exposes it)
    # thickness 3 under 18 neighbours, of the merged ball with its coarse leaves: what three shrinks keep is emptied
    a, grid, depth = scenes()["ball"]
    set_base(render, a, 8 * 60000)
    render.shell_nodes(3, 18, depth)
    core = R.steps(grid, "shrink", 3, 18, 0, True)
    assert np.array_equal(sampled(render, depth), np.where(core != 0, 0, grid)) and (core != 0).sum() > 100000
    assert render.simplify_nodes() < a.size + 8 * 60000


def seen_values(hits, words):
    """the voxel value behind every pixel: a hit's `value` is the index of the leaf word that the ray ended in, which moves when a
    coarse leaf at the surface is split, so the frames of two trees compare by the words' values; -1 where the ray left the grid,
    -2 where it ran into the step limit (`value` is a mark then, no index)"""
    hit = (hits["info"] >> 16 & 1) != 0
    at = hit & (hits["value"] < words.size)
    return np.where(at, (words[np.where(at, hits["value"], 0)] >> 4).astype(np.int64) - B.VOXEL_OFFSET, np.where(hit, -2, -1))


def test_a_shelled_ball_traces_like_the_solid_one_and_the_oracle(pkg, O):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a, grid, depth = scenes()["ball"]
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    hits_solid = O.trace_frame(a, u, threads=4)
    g1, g2 = pkg.Gpu(0), pkg.Gpu(0)
    try:
        r1 = pkg.Render(g1, (64, 64), a, capacity=CAPACITY)
        assert_hits_equal(frame(pkg, r1, u), hits_solid, "the solid ball")
        # shelled through a second context that shares the store; traced through the first
        r2 = pkg.Render.share_nodes(g2, r1)
        r2.shell_nodes(2, 6, depth)
        g2.sync()
        r1.node_length = r2.node_length
        shelled = r1.read_nodes()
        assert np.array_equal(grid_of(shelled, depth), np.where(R.steps(grid, "shrink", 2, 6, 0, True) != 0, 0, grid))
        hits_shell = O.trace_frame(shelled, u, threads=4)
        # the same picture: every ray ends at the same distance, on the same face, in a voxel of the same value
        assert np.array_equal(seen_values(hits_shell, shelled), seen_values(hits_solid, a)) and (seen_values(hits_solid, a) > 0).sum() > 50
        for key in ("t", "normal_bits"):
            assert np.array_equal(hits_shell[key], hits_solid[key]), key
        whole_leaves = hits_shell["value"] < a.size  # (the surface's leaves of the last level were never split: the same word)
        assert whole_leaves.sum() > 50 and np.array_equal(hits_shell["value"][whole_leaves], hits_solid["value"][whole_leaves])
        assert_hits_equal(frame(pkg, r1, u), hits_shell, "the shell, on the context that did not make it")
        assert_hits_equal(frame(pkg, r2, u), hits_shell, "the shell, on the context that made it")
        # one more step on the first context: a grown ball is another picture
        r1.morph_nodes("grow", 2, 26, COLOUR, depth)
        grown = r1.read_nodes()
        hits_grown = O.trace_frame(grown, u, threads=4)
        assert (seen_values(hits_grown, grown) == COLOUR).sum() > 50
        assert_hits_equal(frame(pkg, r1, u), hits_grown, "grown")
    finally:
        g2.close()
        g1.close()


def raw_morph(pkg, gpu, op, conn, depth, n_words, flags=0, colour=0, max_words=0, params=True, out=True):
    p = pkg._lib.MorphParams()
    p.op, p.conn, p.depth, p.flags, p.colour, p.n_words, p.max_words = op, conn, depth, flags, colour, n_words, max_words
    n_out = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_nodes_morph(gpu._h, C.byref(p) if params else None, C.byref(n_out) if out else None)
    gpu.sync()
    return rc, n_out.value


def test_errors_write_nothing(pkg, render, own_gpu):
    a = scenes()["base"][0]
    set_base(render, a)
    before = render.read_nodes(a.size + PAD)
    err = lambda: last_error(pkg, own_gpu)  # noqa: E731

    def refused(code, op=0, conn=26, depth=7, n_words=a.size, **kw):
        assert raw_morph(pkg, own_gpu, op, conn, depth, n_words, **kw)[0] == code, (op, conn, depth, kw, err())
        return err()

    # in the header's order; of two causes the earlier one is reported
    assert "null params" in refused(ERR_ARG, params=False)
    assert "n_words_out" in refused(ERR_ARG, out=False, op=9)
    assert "op must be 0 or 1 (got 2)" in refused(ERR_ARG, op=2, conn=7)
    assert "conn must be 6, 18 or 26 (got 7)" in refused(ERR_ARG, conn=7, depth=0)
    assert "conn must be 6, 18 or 26 (got 0)" in refused(ERR_ARG, conn=0)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=0, flags=2)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=22)
    assert "unknown flag bits (got 3)" in refused(ERR_ARG, flags=3, op=1, colour=5)
    assert "colour must be 0" in refused(ERR_ARG, op=1, colour=5, n_words=12)
    for n_words in (0, 12, CAPACITY + 8):
        assert "n_words must be a positive multiple of 8" in refused(ERR_ARG, n_words=n_words)

    # the depth refusal names the cell; the restatement names the same
    for op in R.OPS:
        with pytest.raises(R.Refused) as e:
            R.morph(a, a.size, op, 26, 5)
        message = refused(ERR_STATE, op=R.OPS.index(op), depth=5)
        assert "%s meets cell (%d, %d, %d)" % ((op,) + e.value.cell) in message and "finer than depth 5" in message
    with pytest.raises(pkg.SvoError):
        render.morph_nodes("grow", depth=5)
    assert render.node_length == a.size
    # the cap: one group short of the restatement's length fails, exactly reached succeeds (below)
    want = morphed("base: grow 6")[0]
    assert want.size > a.size
    assert str(want.size) in refused(ERR_CAP, conn=6, max_words=want.size - 8)
    with pytest.raises(pkg.SvoError):
        render.morph_nodes("grow", 1, 6, depth=7, max_words=want.size - 8)
    assert render.node_length == a.size
    assert np.array_equal(render.read_nodes(a.size + PAD), before)

    # malformed trees, with the compaction's wording: every interior word is opened; depth 5 for a depth-4 tree, so that the
    # last level's pointers are followed too
    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice"}
    cases = malformed_cases()
    for name, part in causes.items():
        words = cases[name]
        set_base(render, words)
        held = render.read_nodes(words.size + PAD)
        for op in (0, 1):
            message = refused(ERR_STATE, op=op, conn=6, depth=5, n_words=words.size)
            assert "malformed tree" in message and part in message, (name, message)
        assert np.array_equal(render.read_nodes(words.size + PAD), held), name

    set_base(render, a, want.size - a.size)
    assert raw_morph(pkg, own_gpu, 0, 6, 7, a.size, max_words=want.size) == (0, want.size)
    assert_words(render.read_nodes(want.size), want, "the cap exactly reached")

    # without a node buffer, and with an adaptive state attached: both before n_words is looked at
    fresh = pkg.Gpu(0)
    try:
        assert raw_morph(pkg, fresh, 0, 6, 7, 12)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
        ms = (C.c_float * 5)()
        assert pkg._lib.lib().svo_morph_timing(fresh._h, ms) == ERR_STATE and "no morphology step" in last_error(pkg, fresh)
    finally:
        fresh.close()
    size, xyzi, pal, _, _ = load_vox_fixture("monu9")
    world = pkg.adaptive.World(pkg.CpuOctree.from_voxels(size, xyzi, pal))
    octree = world.root_octree()
    g = pkg.Gpu(0)
    try:
        g.set_option(pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, 1)
        r = pkg.Render.new(g, (64, 64), octree, capacity=4096)
        attached = pkg.adaptive.DeviceAdaptive(g, r, octree, world)
        held = r.read_nodes()
        assert raw_morph(pkg, g, 0, 6, 7, 12)[0] == ERR_STATE and "adaptive" in last_error(pkg, g)
        assert np.array_equal(r.read_nodes(), held)
        del attached
    finally:
        g.close()
