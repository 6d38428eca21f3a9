"""A tree placed at any cell offset and orientation on the GPU (csrc/svo_place.hip): word for word against the
rule's restatement (tests/place_ref.py: place) and cell for cell against the per-cell contract (apply_cells) on the cases of
the host tests; nothing written behind the new length, on an error or by a second identical call; the same bytes on every run;
an aligned placement against combine_nodes; the edges of the arguments (depth 1 at all 27 offsets around the scene, eight
paths of 20 splits at depth 21, sources handed over as tensors and as a Render, a source whose pointers share a group, hit
counters); every error in the header's order; the canonical form after simplification and compaction against a build of the
moved and turned cells; quarter turns against stamp_structures'; frames traced from a placed tree against the oracle, also
when the call came through a context that shares the buffer."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import combine_ref as X
import place_ref as P
import sample_ref as S
from conftest import assert_hits_equal, load_vox_fixture
from pass_frame import assert_words, last_error, own_gpu  # noqa: F401
from pass_session_ops import tree_structure
from test_combine_gpu import on_device, sampled
from test_combine_host import EMPTY_ROOT, leaf, small_source, trees7
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, ERR_ARG, ERR_CAP, ERR_STATE, PAD, ROOT, frame, poison, set_base
from test_place_host import CASES, IDS, TILE, case_named, placed, sources

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def tensors(own_gpu):
    """the shared sources in device memory, uploaded once"""
    return {name: on_device(own_gpu, words) for name, (words, _, _) in sources().items()}


def check_place(render, scene, want, tensor, op, depth, what, offset=(0, 0, 0), orient=0, src_depth=None, runs=2):
    """scene -> place_nodes on the GPU == `want`, the restatement's words; the words behind the new length keep what they
    held, and a second run from the same scene gives the same bytes"""
    growth = want.size - scene.size
    for run in range(runs):
        set_base(render, scene, growth)
        n = render.place_nodes(tensor, op, depth, offset=offset, orient=orient, src_depth=src_depth)
        assert n == want.size == render.node_length, f"{what}: length {n}, want {want.size}"
        got = render.read_nodes(n + PAD)
        assert_words(got[:n], want, f"{what}, run {run}")
        assert np.array_equal(got[n:], poison(growth + PAD)[growth:]), f"{what}: words behind the new length were written"
    return want


@pytest.mark.parametrize("name,source,op,offset,orient", CASES, ids=IDS)
def test_the_host_cases(render, tensors, name, source, op, offset, orient):
    a, grid_a = trees7()["base"]
    b, grid_b, src_depth = sources()[source]
    want, tally = placed(name)
    check_place(render, a, want, tensors[source], op, 7, name, offset, orient, src_depth)
    if (op, source, offset) == ("over", "ball", (1, 1, 1)):
        # a level's frontier and its splits go beyond one scan tile, and its groups fill no whole wave
        assert any(n > TILE and s > TILE and (n // 8) % 64 for n, s in tally["levels"]), tally["levels"]
    assert np.array_equal(sampled(render, 7), P.apply_cells(grid_a, grid_b, op, offset, orient)), f"{name}: the cells"


def test_an_aligned_placement_gives_the_bytes_of_combine_nodes(render, tensors):
    a, ball = trees7()["base"][0], tensors["ball"]
    src = small_source()
    small = on_device(render.gpu, src)
    pasted = trees7()["pasted"][0]
    for scene, op, source, kw_combine, kw_place in (
            (a, "over", ball, {}, {}), (a, "carve", ball, {}, {}), (a, "replace", ball, {}, {}), (a, "under", ball, {}, {}),
            (pasted, "over", small, {"at": (3, 3, 3), "at_level": 3}, {"offset": (48, 48, 48), "src_depth": 4}),
            (pasted, "carve", small, {"at": (3, 3, 3), "at_level": 3}, {"offset": (48, 48, 48), "src_depth": 4}),
            (EMPTY_ROOT, "replace", small, {"at": (5, 2, 7), "at_level": 3}, {"offset": (80, 32, 112), "src_depth": 4})):
        room = 8 * 60000
        set_base(render, scene, room)
        n = render.combine_nodes(source, op, 7, **kw_combine)
        want = render.read_nodes(n + PAD)
        set_base(render, scene, room)
        assert render.place_nodes(source, op, 7, **kw_place) == n > 0
        assert_words(render.read_nodes(n + PAD), want, f"{op}, {kw_place}")


def test_an_identical_second_call_writes_nothing(render, tensors):
    a = trees7()["base"][0]
    for op in ("over", "carve", "keep"):
        name, source, _, offset, orient = case_named(op, "ball", (1, 1, 1))
        first = check_place(render, a, placed(name)[0], tensors[source], op, 7, name, offset, orient, runs=1)
        whole = render.read_nodes(first.size + PAD)
        assert render.place_nodes((tensors[source], sources()[source][0].size), op, 7, offset=offset, orient=orient) == first.size
        assert np.array_equal(render.read_nodes(first.size + PAD), whole), op
    ms = render.gpu.place_timing()
    assert len(ms) == 5 and all(t >= 0 for t in ms) and ms[0] > 0 and ms[4] > 0


def test_untouched_words_keep_their_counters(render, tensors):
    a, b = trees7()["base"][0], sources()["ball"][0]
    rng = np.random.default_rng(33)
    counted = a | rng.integers(1, 16, a.size).astype(np.uint32)
    want = P.place(counted, counted.size, b, "under", 7, (1, 1, 1), 9)[0]
    check_place(render, counted, want, tensors["ball"], "under", 7, "a scene with hit counters", (1, 1, 1), 9, runs=1)
    kept = want[: a.size] == counted
    assert kept.sum() > a.size // 2 and (~kept).sum() > 1000 and (want[: a.size][~kept] & 15 == 0).all() and (want[a.size:] & 15 == 0).all()
    # the source's counters are ignored
    src = b | rng.integers(1, 16, b.size).astype(np.uint32)
    plain = P.place(a, a.size, b, "over", 7, (1, 1, 1), 9)[0]
    check_place(render, a, plain, on_device(render.gpu, src), "over", 7, "a source with hit counters", (1, 1, 1), 9, runs=1)


def test_depth_1_at_all_27_offsets(render):
    scene = np.array([leaf(v) | c for v, c in zip([0, 0, 5, 5, 0x7FFFFFF, 9, 0, 3], range(8))], dtype=np.uint32)
    source = np.array([leaf(v) for v in [0, 7, 0, 7, 1, 0, 0, 0x7FFFFFF]], dtype=np.uint32)
    ga, gb = (S.sample_dense(w, 8, (0, 0, 0), (2,) * 3, 1) for w in (scene, source))
    tensor = on_device(render.gpu, source)
    for i, offset in enumerate((x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)):
        for op in X.OPS:
            orient = (7 * i + X.OPS.index(op)) % 48
            want, tally = P.place(scene, 8, source, op, 1, offset, orient, 1)
            cells = P.apply_cells(ga, gb, op, offset, orient)
            check_place(render, scene, want, tensor, op, 1, f"depth 1, {op} at {offset}", offset, orient, 1, runs=1)
            assert want.size == 8 and np.array_equal(sampled(render, 1), cells), (op, offset)
            assert tally["overwrites"] == (ga != cells).sum()


def test_eight_paths_of_20_splits_at_depth_21(render):
    colours = [0x010203, 0x0A0B0C, 0x111111, 0x222222, 0x333333, 0x444444, 0x555555, 0xFFFFFF]
    source = np.array([leaf(v) for v in colours], dtype=np.uint32)
    tensor = on_device(render.gpu, source)
    mid = (1 << 20) - 1  # the source's eight cells lie around the scene's centre, one in every child of the root
    want, tally = P.place(EMPTY_ROOT, 8, source, "over", 21, (mid,) * 3, 0, 1)
    assert tally["splits"] == 160 and tally["overwrites"] == 8 and tally["levels"] == [(8, 8)] + [(64, 8)] * 19 + [(64, 0)]
    check_place(render, EMPTY_ROOT, want, tensor, "over", 21, "depth 21", (mid,) * 3, 0, 1)
    cells = np.array([[mid + x, mid + y, mid + z] for x in (0, 1) for y in (0, 1) for z in (0, 1)] + [[mid - 1, mid, mid], [0, 0, 0]])
    assert render.sample_voxels(cells, 21).cpu().numpy().tolist() == colours + [0, 0]
    # the same placement again writes nothing; turned upside down about y, the colours swap in pairs
    assert render.place_nodes(tensor, "over", 21, offset=(mid,) * 3, src_depth=1) == want.size
    assert_words(render.read_nodes(), want, "the second call")
    flipped = P.place(want, want.size, source, "replace", 21, (mid,) * 3, 2, 1)[0]
    check_place(render, want, flipped, tensor, "replace", 21, "depth 21, flipped", (mid,) * 3, 2, 1, runs=1)
    assert render.sample_voxels(cells[:8], 21).cpu().numpy().tolist() == [colours[c ^ 2] for c in range(8)]


def test_sources_from_a_simplification_and_from_another_render(pkg, render):
    a = trees7()["base"][0]
    b = sources()["ball"][0]
    name, _, op, offset, orient = case_named("over", "ball", (3, -5, 64))
    want = placed(name)[0]
    other = pkg.Gpu(0)
    try:
        cells = X.ball_cells(7, (128, 128, 128), 100)
        model = pkg.Render.from_voxels(other, (64, 64), cells, 7, np.where(cells[:, 0] < 64, 0x40C0FF, 0xFF8020), capacity=1 << 20)
        pair = model.simplify_nodes(out_of_place=True)
        assert pair[1] == b.size
        set_base(render, a, want.size - a.size)
        assert render.place_nodes(pair, op, 7, offset=offset, orient=orient) == want.size
        assert_words(render.read_nodes(), want, "the pair of simplify_nodes(out_of_place=True)")
        assert model.simplify_nodes() == b.size
        set_base(render, a, want.size - a.size)
        assert render.place_nodes(model, op, 7, offset, orient) == want.size
        assert_words(render.read_nodes(), want, "another Render")
        assert_words(model.read_nodes(), b, "the source, only read")
        set_base(render, a, want.size - a.size)
        assert render.place_nodes(on_device(render.gpu, b), op, 7, offset=offset, orient=orient, src_depth=7) == want.size
        assert_words(render.read_nodes(), want, "a tensor")
        with pytest.raises(ValueError):
            render.place_nodes(model, "above", 7)
        with pytest.raises(ValueError):
            render.place_nodes(model, "over", 7, offset=(1, 2))
    finally:
        other.close()


def test_a_source_whose_pointers_share_a_group(render):
    b = sources()["ball"][0]
    twice = b.copy()
    twice[:8] = twice[int(np.flatnonzero(b[:8] >> 4 < B.VOXEL_OFFSET)[0])]
    want, tally = P.place(EMPTY_ROOT, 8, twice, "over", 7, (0, 0, 0), 17)
    check_place(render, EMPTY_ROOT, want, on_device(render.gpu, twice), "over", 7, "eight pointers to one group", (0, 0, 0), 17)
    got = sampled(render, 7)
    assert tally["splits"] > 8 and np.array_equal(got[:64, :64, :64], got[64:, 64:, 64:]) and (got != 0).any()


def raw_place(pkg, gpu, src, op, depth, n_words, src_words, src_depth=None, orient=0, offset=(0, 0, 0), max_words=0, params=True, out=True):
    """src: a device tensor, an address or None"""
    p = pkg._lib.PlaceParams()
    p.op, p.depth, p.src_depth, p.orient, p.n_words, p.src_words, p.max_words = op, depth, depth if src_depth is None else src_depth, orient, n_words, src_words, max_words
    p.offset[:] = list(offset)
    n_out = C.c_uint64(12345)
    ptr = src.data_ptr() if hasattr(src, "data_ptr") else src
    rc = pkg._lib.lib().svo_nodes_place(gpu._h, ptr, C.byref(p) if params else None, C.byref(n_out) if out else None)
    gpu.sync()
    return rc, n_out.value


def test_errors_write_nothing(pkg, render, own_gpu, tensors):
    a = trees7()["base"][0]
    b = sources()["ball"][0]
    ball = tensors["ball"]
    set_base(render, a)
    before = render.read_nodes(a.size + PAD)
    err = lambda: last_error(pkg, own_gpu)  # noqa: E731

    def refused(code, src=ball, op=0, depth=7, n_words=a.size, src_words=b.size, **kw):
        assert raw_place(pkg, own_gpu, src, op, depth, n_words, src_words, **kw)[0] == code, (op, depth, kw, err())
        return err()

    # in the header's order; of two causes the earlier one is reported
    assert "null params" in refused(ERR_ARG, params=False)
    assert "n_words_out" in refused(ERR_ARG, out=False, op=9)
    assert "null source" in refused(ERR_ARG, src=None, op=9)
    assert "op must be 0..5 (got 6)" in refused(ERR_ARG, op=6, depth=0)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=0, src_depth=0)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=22)
    assert "src_depth must be 1..depth (got 0" in refused(ERR_ARG, src_depth=0, orient=48)
    assert "src_depth must be 1..depth (got 8" in refused(ERR_ARG, src_depth=8, orient=48)
    assert "orient must be 0..47 (got 48)" in refused(ERR_ARG, orient=48, offset=(1 << 22, 0, 0))
    assert "axis 1: 2097153" in refused(ERR_ARG, offset=(0, (1 << 21) + 1, 0), n_words=12)
    assert "axis 2: -2097153" in refused(ERR_ARG, offset=(0, 0, -(1 << 21) - 1), n_words=12)
    for n_words in (0, 12, CAPACITY + 8):
        assert "n_words must be a positive multiple of 8" in refused(ERR_ARG, n_words=n_words, src_words=12)
    for src_words in (0, 12, (1 << 27) + 8):
        assert "src_words must be a positive multiple of 8" in refused(ERR_ARG, src_words=src_words)
    ptr, room = C.c_void_p(), C.c_size_t()
    own_gpu.check(pkg._lib.lib().svo_nodes_device_ptr(own_gpu._h, C.byref(ptr), C.byref(room)))
    assert room.value == CAPACITY
    for address, src_words in ((ptr.value, 8), (ptr.value + 4 * (CAPACITY - 8), 16), (ptr.value - 4 * 8, 16)):
        assert "overlaps the node buffer" in refused(ERR_ARG, src=address, src_words=src_words)
    # the ends of the offset's range are allowed: wholly outside, nothing written
    assert raw_place(pkg, own_gpu, ball, 5, 7, a.size, b.size, offset=(1 << 21, 0, -(1 << 21))) == (0, a.size)

    # the depth refusal names the cell and the tree; the restatement names the same
    seven = np.full(8, leaf(7), dtype=np.uint32)
    for src, source, op, kw, text in ((ball, b, "over", {"offset": (1, 1, 1), "orient": 3}, None),
                                      (ball, b, "over", {}, "the scene and the source are interior nodes"),
                                      (on_device(own_gpu, seven), seven, "paint", {"offset": (-3, 0, 2)}, "the scene is an interior node")):
        with pytest.raises(X.Refused) as e:
            P.place(a, a.size, source, op, 5, kw.get("offset", (0, 0, 0)), kw.get("orient", 0))
        text = text or {"both": "the scene and the source are", "scene": "the scene is", "source": "the source is"}[e.value.finer]
        message = refused(ERR_STATE, src=src, op=X.OPS.index(op), depth=5, src_words=source.size, **kw)
        assert "%s meets cell (%d, %d, %d)" % ((op,) + e.value.cell) in message and text in message and "at depth 5" in message
    with pytest.raises(pkg.SvoError):
        render.place_nodes(ball, "over", 5, offset=(1, 1, 1))
    assert render.node_length == a.size
    # the cap: one group short of the reference's length fails, exactly reached succeeds (below)
    name, _, _, offset, orient = case_named("over", "ball", (4, 0, -8))
    want = placed(name)[0]
    assert want.size > a.size
    assert str(want.size) in refused(ERR_CAP, max_words=want.size - 8, offset=offset, orient=orient)
    with pytest.raises(pkg.SvoError):
        render.place_nodes(ball, "over", 7, offset, orient, max_words=want.size - 8)
    assert render.node_length == a.size
    assert np.array_equal(render.read_nodes(a.size + PAD), before)

    # the source is finer than src_depth where it is pasted into a coarse leaf
    set_base(render, EMPTY_ROOT)
    held = render.read_nodes(8 + PAD)
    with pytest.raises(X.Refused) as e:
        P.place(EMPTY_ROOT, 8, b, "over", 7, (1, 1, 1), 3, 5)
    message = refused(ERR_STATE, n_words=8, src_depth=5, offset=(1, 1, 1), orient=3)
    assert "over meets cell (%d, %d, %d)" % e.value.cell in message and "the source is an interior node" in message
    # a malformed source: only the pointers that the call follows, and before the depth refusal
    bad = b.copy()
    first = int(np.flatnonzero(bad[:8] >> 4 < B.VOXEL_OFFSET)[0])
    bad[first] = (b.size + 8) << 4
    message = refused(ERR_STATE, src=on_device(own_gpu, bad), depth=5, n_words=8, offset=(1, 1, 1))
    assert "malformed source" in message and "leaves the first src_words" in message
    bad[first] = 12 << 4
    unaligned = on_device(own_gpu, bad)
    message = refused(ERR_STATE, src=unaligned, n_words=8, offset=(1, 1, 1))
    assert "malformed source" in message and "not a multiple of 8" in message
    assert np.array_equal(render.read_nodes(8 + PAD), held)
    solid = np.full(8, leaf(0x102030), dtype=np.uint32)
    set_base(render, solid)
    assert raw_place(pkg, own_gpu, unaligned, X.UNDER, 7, 8, b.size, offset=(1, 1, 1)) == (0, 8)  # (never looked at)
    assert np.array_equal(render.read_nodes(8), solid)

    # malformed scenes, with the compaction's wording; a paint by one voxel over the whole grid opens every interior word
    paint = on_device(own_gpu, solid)
    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice"}
    cases = malformed_cases()
    for name, part in causes.items():
        words = cases[name]
        set_base(render, words)
        held = render.read_nodes(words.size + PAD)
        message = refused(ERR_STATE, src=paint, op=X.PAINT, depth=5, n_words=words.size, src_words=8, orient=5)
        assert "malformed tree" in message and part in message, (name, message)
        assert np.array_equal(render.read_nodes(words.size + PAD), held), name

    set_base(render, a, want.size - a.size)
    assert raw_place(pkg, own_gpu, ball, X.OVER, 7, a.size, b.size, offset=offset, orient=orient, max_words=want.size) == (0, want.size)
    assert_words(render.read_nodes(want.size), want, "the cap exactly reached")

    # without a node buffer, and with an adaptive state attached: both before n_words is looked at
    fresh = pkg.Gpu(0)
    try:
        assert raw_place(pkg, fresh, ball, 0, 7, 12, b.size)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
        ms = (C.c_float * 5)()
        assert pkg._lib.lib().svo_place_timing(fresh._h, ms) == ERR_STATE and "no tree placed" in last_error(pkg, fresh)
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
        assert raw_place(pkg, g, ball, 0, 7, 12, b.size)[0] == ERR_STATE and "adaptive" in last_error(pkg, g)
        assert np.array_equal(r.read_nodes(), held)
        del attached
    finally:
        g.close()


def test_the_canonical_form_is_a_build_of_the_moved_and_turned_cells(pkg, render, tensors):
    """replace into an empty scene, then simplify and compact: byte for byte the tree built from the cells, after the same two"""
    b, grid_b, _ = sources()["ball"]
    offset, orient = (3, -5, 64), pkg.orientation.from_matrix([[0, -1, 0], [0, 0, 1], [-1, 0, 0]])
    assert orient and pkg.orientation.is_rotation(orient)
    cells = P.apply_cells(np.zeros((128,) * 3, dtype=np.uint32), grid_b, "replace", offset, orient)
    want = P.place(EMPTY_ROOT, 8, b, "replace", 7, offset, orient)[0]
    check_place(render, EMPTY_ROOT, want, tensors["ball"], "replace", 7, "into an empty scene", offset, orient, runs=1)
    assert np.array_equal(sampled(render, 7), cells)
    render.simplify_nodes()
    placed_words = render.read_nodes(render.compact_nodes())
    at = np.argwhere(cells != 0)
    assert 100000 < len(at) < (grid_b != 0).sum()  # (clipped at z = 128)
    other = pkg.Gpu(0)
    try:
        built = pkg.Render.from_voxels(other, (64, 64), at, 7, cells[tuple(at.T)].astype(np.int64), capacity=CAPACITY)
        built.simplify_nodes()
        assert_words(placed_words, built.read_nodes(built.compact_nodes()), "placed, simplified and compacted against built")
    finally:
        other.close()


def test_quarter_turns_are_stamp_structures(pkg, render):
    """place_structures with rots = k against place_nodes of a tree of the unrotated structure with quarter_turns_y(k)"""
    offsets, _, colours = tree_structure()  # 187 voxels within x -4..5, y 0..13, z -4..4: a cube of 16 holds them
    offsets, colours = np.asarray(offsets, dtype=np.int64), np.asarray(colours, dtype=np.int64)
    assert (colours != 0).all() and (offsets.max(axis=0) - offsets.min(axis=0) < 16).all()
    structure = pkg.Structure(offsets, np.ones(len(offsets)), colours)
    model = B.build(offsets - offsets.min(axis=0), 4, colours)
    grid = S.sample_dense(model, model.size, (0, 0, 0), (16,) * 3, 4)
    tensor = on_device(render.gpu, model)
    origin = np.array([70, 40, 33])
    grids = []
    for k in range(4):
        set_base(render, EMPTY_ROOT, 8 * 4000)
        render.place_structures(structure, [origin], 7, [k])
        stamped = sampled(render, 7)
        # the offset: the turned structure's min corner in the scene less the oriented source's in its cube
        orient = pkg.orientation.quarter_turns_y(k)
        turn = np.linalg.matrix_power(np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]]), k)
        in_scene = (offsets @ turn.T + origin).min(axis=0)
        in_cube = np.argwhere(P.orient_grid(grid, orient) != 0).min(axis=0)
        set_base(render, EMPTY_ROOT, 8 * 4000)
        render.place_nodes(tensor, "over", 7, offset=tuple(int(v) for v in in_scene - in_cube), orient=orient, src_depth=4)
        assert np.array_equal(sampled(render, 7), stamped) and (stamped != 0).sum() == len(offsets), k
        grids.append(stamped.tobytes())
    assert len(set(grids)) == 4


def test_a_placed_tree_traces_like_the_oracle(pkg, O):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a = trees7()["base"][0]
    b = sources()["ball"][0]
    model = sources()["model5"][0]
    name, _, _, offset, orient = case_named("over", "ball", (3, -5, 64))
    pasted = placed(name)[0]
    carved = P.place(pasted, pasted.size, model, "carve", 7, (50, 60, 70), 13, 5)[0]
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    hits_base, hits_pasted, hits_carved = (O.trace_frame(t, u, threads=4) for t in (a, pasted, carved))
    assert (hits_pasted["value"] != hits_base["value"]).sum() > 50 and (hits_carved["value"] != hits_pasted["value"]).sum() > 0
    g1, g2 = pkg.Gpu(0), pkg.Gpu(0)
    try:
        r1 = pkg.Render(g1, (64, 64), a, capacity=CAPACITY)
        assert_hits_equal(frame(pkg, r1, u), hits_base, "the base")
        assert r1.place_nodes(on_device(g1, b), "over", 7, offset, orient) == pasted.size
        assert_words(r1.read_nodes(), pasted, "pasted")
        assert_hits_equal(frame(pkg, r1, u), hits_pasted, "the placed ball")
        # the next placement through a second context that shares the store; traced through the first
        r2 = pkg.Render.share_nodes(g2, r1)
        assert r2.place_nodes(on_device(g2, model), "carve", 7, (50, 60, 70), 13, 5) == carved.size
        g2.sync()
        r1.node_length = r2.node_length
        assert_words(r1.read_nodes(), carved, "carved through the sharing context")
        assert_hits_equal(frame(pkg, r1, u), hits_carved, "carved, on the context that did not place")
        assert_hits_equal(frame(pkg, r1, u), hits_carved, "carved, a second frame")
        assert_hits_equal(frame(pkg, r2, u), hits_carved, "carved, on the context that placed")
    finally:
        g2.close()
        g1.close()
