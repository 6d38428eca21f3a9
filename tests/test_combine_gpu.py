"""Two trees combined on the GPU (csrc/svo_combine.hip): word for word against the rule's restatement
(tests/combine_ref.py: combine) and cell for cell against the per-cell contract (apply_cells) on the depth-7 cases of the
host tests; nothing written behind the new length, on an error or by a second identical call; the same bytes on every run;
the edges of the arguments (depth 1, a path of 20 splits at depth 21, sources handed over as tensors and as a Render, a
source whose pointers share a group); every error in the header's order; compaction and simplification afterwards; frames
traced from a combined tree against the oracle, also when the combine came through a context that shares the buffer."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import combine_ref as X
import compact_ref as K
import sample_ref as S
import simplify_ref as M
from conftest import assert_hits_equal, load_vox_fixture
from pass_frame import assert_words, last_error, own_gpu  # noqa: F401
from test_combine_host import EMPTY_ROOT, SHOWS, cases7, leaf, small_source, trees7
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, ERR_ARG, ERR_CAP, ERR_STATE, PAD, ROOT, frame, poison, set_base

pytestmark = pytest.mark.gpu

TILE = 4096  # items of one scan tile (csrc/svo_scan.h)


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


def on_device(gpu, words):
    """the words as a device int32 tensor, there when this returns"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(gpu.torch_device)
    torch.cuda.current_stream(gpu.torch_device).synchronize()
    return t


@pytest.fixture(scope="module")
def sources(own_gpu):
    """the shared sources in device memory, uploaded once"""
    return {name: on_device(own_gpu, trees7()[name][0]) for name in ("ball", "words")}


def check_combine(render, scene, source, tensor, op, depth, what, at_level=0, at=(0, 0, 0), runs=2):
    """scene -> combine_nodes on the GPU == combine_ref.combine, the words behind the new length keep what they held, and a
    second run from the same scene gives the same bytes.  Returns (the words, the reference's tallies)"""
    want, tally = X.combine(scene, scene.size, source, op, depth, at_level, at)
    growth = want.size - scene.size
    assert growth == 8 * tally["splits"]
    for run in range(runs):
        set_base(render, scene, growth)
        n = render.combine_nodes(tensor, op, depth, at=at, at_level=at_level)
        assert n == want.size == render.node_length, f"{what}: length {n}, want {want.size}"
        got = render.read_nodes(n + PAD)
        assert_words(got[:n], want, f"{what}, run {run}")
        assert np.array_equal(got[n:], poison(growth + PAD)[growth:]), f"{what}: words behind the new length were written"
    return want, tally


def sampled(render, depth):
    side = 1 << depth
    return render.sample_dense((0, 0, 0), (side,) * 3, depth).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name,scene,source,op", cases7(), ids=[c[0] for c in cases7()])
def test_the_depth_7_cases(render, sources, name, scene, source, op):
    (a, grid_a), (b, grid_b) = trees7()[scene], trees7()[source]
    want, tally = check_combine(render, a, b, sources[source], op, 7, name)
    if scene == "base" and source == "ball":
        for key in SHOWS[op]:
            assert tally[key] > 0 or (op, key) == ("carve", "splits"), (name, key, tally)
    if name == "carve, pasted scene":
        assert tally["splits"] > TILE  # (what no carve of the base can show: a coarse voxel split by the source's surface)
    if name == "over, ball":
        # a level's frontier and its splits go beyond one scan tile, and its groups fill no whole wave
        assert max(s for _, s in tally["levels"]) > TILE and max(n for n, _ in tally["levels"]) > TILE, tally["levels"]
        assert any((n // 8) % 64 and n > TILE for n, _ in tally["levels"]), tally["levels"]
    assert np.array_equal(sampled(render, 7), X.apply_cells(grid_a, grid_b, op, (0, 0, 0), 7)), f"{name}: the cells"


def test_an_identical_second_call_writes_nothing(render, sources):
    a, b = trees7()["base"][0], trees7()["ball"][0]
    for op in ("over", "carve"):
        first, _ = check_combine(render, a, b, sources["ball"], op, 7, op, runs=1)
        whole = render.read_nodes(first.size + PAD)
        assert render.combine_nodes((sources["ball"], b.size), op, 7) == first.size
        assert np.array_equal(render.read_nodes(first.size + PAD), whole), op
    ms = render.gpu.combine_timing()
    assert len(ms) == 5 and all(t >= 0 for t in ms) and ms[0] > 0 and ms[4] > 0


def test_untouched_words_keep_their_counters(render, sources):
    a, b = trees7()["base"][0], trees7()["ball"][0]
    rng = np.random.default_rng(33)
    counted = a | rng.integers(1, 16, a.size).astype(np.uint32)
    want, tally = check_combine(render, counted, b, sources["ball"], "under", 7, "a scene with hit counters", runs=1)
    kept = want[: a.size] == counted
    assert kept.sum() > a.size // 2 and (~kept).sum() > 1000 and (want[: a.size][~kept] & 15 == 0).all()
    assert (want[a.size:] & 15 == 0).all()
    # the source's counters are ignored
    src = b | rng.integers(1, 16, b.size).astype(np.uint32)
    check_combine(render, a, src, on_device(render.gpu, src), "over", 7, "a source with hit counters", runs=1)
    assert_words(render.read_nodes(), X.combine(a, a.size, b, "over", 7)[0], "against the source without them")


def test_depth_1(render):
    scene = np.array([leaf(v) | c for v, c in zip([0, 0, 5, 5, 0x7FFFFFF, 9, 0, 3], range(8))], dtype=np.uint32)
    source = np.array([leaf(v) for v in [0, 7, 0, 7, 1, 0, 0, 0x7FFFFFF]], dtype=np.uint32)
    ga, gb = (S.sample_dense(w, 8, (0, 0, 0), (2,) * 3, 1) for w in (scene, source))
    tensor = on_device(render.gpu, source)
    for op in X.OPS:
        want, tally = check_combine(render, scene, source, tensor, op, 1, f"depth 1, {op}")
        assert want.size == 8 and np.array_equal(sampled(render, 1), X.apply_cells(ga, gb, op, (0, 0, 0), 1)), op
        assert tally["overwrites"] == (ga != X.apply_cells(ga, gb, op, (0, 0, 0), 1)).sum()


def test_a_path_of_20_splits_at_depth_21(render):
    source = np.array([leaf(v) for v in [0x010203, 0, 0, 0x0A0B0C, 0, 0, 0, 0xFFFFFF]], dtype=np.uint32)
    at = ((1 << 20) - 1, 5, 617283)
    want, tally = check_combine(render, EMPTY_ROOT, source, on_device(render.gpu, source), "over", 21, "depth 21", at_level=20, at=at)
    assert tally["splits"] == 20 and want.size == 168 and tally["overwrites"] == 3 and tally["levels"] == [(8, 1)] * 20 + [(8, 0)]
    corner = np.array(at) * 2
    cells = np.array([corner, corner + (0, 1, 1), corner + 1, corner + (1, 0, 0), corner - (0, 1, 0), [0, 0, 0]])
    assert render.sample_voxels(cells, 21).cpu().numpy().tolist() == [0x010203, 0x0A0B0C, 0xFFFFFF, 0, 0, 0]
    # the same placement again writes nothing; under a KEEP the path's seven siblings per level stay out of it
    assert render.combine_nodes(on_device(render.gpu, source), "over", 21, at=at, at_level=20) == 168
    assert_words(render.read_nodes(), want, "the second call")
    check_combine(render, want, EMPTY_ROOT, on_device(render.gpu, EMPTY_ROOT), "keep", 21, "depth 21, masked away", at_level=20, at=at, runs=1)
    assert render.sample_voxels(cells, 21).cpu().numpy().tolist() == [0] * 6


def test_a_source_placed_in_a_cell_of_level_3(render):
    src = small_source()
    tensor = on_device(render.gpu, src)
    gb = S.sample_dense(src, src.size, (0, 0, 0), (16,) * 3, 4)
    a, ga = trees7()["pasted"]
    for op in ("over", "carve", "under"):
        check_combine(render, a, src, tensor, op, 7, f"placed in a coarse voxel, {op}", at_level=3, at=(3, 3, 3), runs=1)
        assert np.array_equal(sampled(render, 7), X.apply_cells(ga, gb, op, (3, 3, 3), 4)), op
    a, ga = trees7()["base"]
    want, tally = check_combine(render, a, src, tensor, "replace", 7, "placed where the scene is interior", at_level=3, at=(3, 3, 3))
    assert [s for _, s in tally["levels"][:3]] == [0, 0, 0]
    assert np.array_equal(sampled(render, 7), X.apply_cells(ga, gb, "replace", (3, 3, 3), 4))


def test_sources_from_a_simplification_and_from_another_render(pkg, render):
    a, ga = trees7()["base"]
    b, gb = trees7()["ball"]
    want = X.combine(a, a.size, b, "over", 7)[0]
    other = pkg.Gpu(0)
    try:
        # the ball built and merged on a second context: its Render is the source, and so is its out-of-place simplification
        cells = X.ball_cells(7, (128, 128, 128), 100)
        model = pkg.Render.from_voxels(other, (64, 64), cells, 7, np.where(cells[:, 0] < 64, 0x40C0FF, 0xFF8020), capacity=1 << 20)
        pair = model.simplify_nodes(out_of_place=True)
        assert pair[1] == b.size
        set_base(render, a, want.size - a.size)
        assert render.combine_nodes(pair, "over", 7) == want.size
        assert_words(render.read_nodes(), want, "the pair of simplify_nodes(out_of_place=True)")
        assert model.simplify_nodes() == b.size
        assert_words(model.read_nodes(), b, "the merged ball")
        set_base(render, a, want.size - a.size)
        assert render.combine_nodes(model, "over", 7) == want.size
        assert_words(render.read_nodes(), want, "another Render")
        assert_words(model.read_nodes(), b, "the source, only read")
        with pytest.raises(ValueError):
            render.combine_nodes(model, "above", 7)
    finally:
        other.close()


def test_a_source_whose_pointers_share_a_group(render):
    b = trees7()["ball"][0]
    twice = b.copy()
    twice[:8] = twice[int(np.flatnonzero(b[:8] >> 4 < B.VOXEL_OFFSET)[0])]
    want, tally = check_combine(render, EMPTY_ROOT, twice, on_device(render.gpu, twice), "over", 7, "eight pointers to one group")
    got = sampled(render, 7)
    assert tally["splits"] > 8 and np.array_equal(got[:64, :64, :64], got[64:, 64:, 64:]) and (got != 0).any()


def raw_combine(pkg, gpu, src, op, depth, n_words, src_words, at_level=0, at=(0, 0, 0), max_words=0, params=True, out=True):
    """src: a device tensor, an address or None"""
    p = pkg._lib.CombineParams()
    p.op, p.depth, p.at_level, p.n_words, p.src_words, p.max_words = op, depth, at_level, n_words, src_words, max_words
    p.at[:] = list(at)
    n_out = C.c_uint64(12345)
    ptr = src.data_ptr() if hasattr(src, "data_ptr") else src
    rc = pkg._lib.lib().svo_nodes_combine(gpu._h, ptr, C.byref(p) if params else None, C.byref(n_out) if out else None)
    gpu.sync()
    return rc, n_out.value


def test_errors_write_nothing(pkg, render, own_gpu, sources):
    a, ga = trees7()["base"]
    b = trees7()["ball"][0]
    ball = sources["ball"]
    set_base(render, a)
    before = render.read_nodes(a.size + PAD)
    err = lambda: last_error(pkg, own_gpu)  # noqa: E731

    def refused(code, src=ball, op=0, depth=7, n_words=a.size, src_words=b.size, **kw):
        assert raw_combine(pkg, own_gpu, src, op, depth, n_words, src_words, **kw)[0] == code, (op, depth, kw, err())
        return err()

    # in the header's order; of two causes the earlier one is reported
    assert "null params" in refused(ERR_ARG, params=False)
    assert "n_words_out" in refused(ERR_ARG, out=False, op=9)
    assert "null source" in refused(ERR_ARG, src=None, op=9)
    assert "op must be 0..5 (got 6)" in refused(ERR_ARG, op=6, depth=0)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=0, at_level=3)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=22)
    assert "at_level must be below depth" in refused(ERR_ARG, at_level=7, at=(1 << 30, 0, 0))
    assert "axis 1: 4" in refused(ERR_ARG, at_level=2, at=(3, 4, 0), n_words=12)
    for n_words in (0, 12, CAPACITY + 8):
        assert "n_words must be a positive multiple of 8" in refused(ERR_ARG, n_words=n_words, src_words=12)
    for src_words in (0, 12, (1 << 27) + 8):
        assert "src_words must be a positive multiple of 8" in refused(ERR_ARG, src_words=src_words)
    ptr, room = C.c_void_p(), C.c_size_t()
    own_gpu.check(pkg._lib.lib().svo_nodes_device_ptr(own_gpu._h, C.byref(ptr), C.byref(room)))
    assert room.value == CAPACITY
    for address, src_words in ((ptr.value, 8), (ptr.value + 4 * (CAPACITY - 8), 16), (ptr.value - 4 * 8, 16)):
        assert "overlaps the node buffer" in refused(ERR_ARG, src=address, src_words=src_words)

    # the depth refusal names the cell and the tree; the restatement names the same
    for scene, src, source, op, finer, text in ((a, ball, b, "over", "both", "the scene and the source are interior nodes"),
                                                (a, on_device(own_gpu, np.full(8, leaf(7), dtype=np.uint32)), np.full(8, leaf(7), dtype=np.uint32),
                                                 "paint", "scene", "the scene is an interior node")):
        with pytest.raises(X.Refused) as e:
            X.combine(scene, scene.size, source, op, 5)
        assert e.value.finer == finer
        message = refused(ERR_STATE, src=src, op=X.OPS.index(op), depth=5, src_words=source.size)
        assert "%s meets cell (%d, %d, %d)" % ((op,) + e.value.cell) in message and text in message and "at depth 5" in message
    with pytest.raises(pkg.SvoError):
        render.combine_nodes(ball, "over", 5)
    assert render.node_length == a.size
    # the cap: one group short of the reference's length fails, exactly reached succeeds (below)
    want = X.combine(a, a.size, b, "over", 7)[0]
    assert want.size > a.size
    assert str(want.size) in refused(ERR_CAP, max_words=want.size - 8)
    with pytest.raises(pkg.SvoError):
        render.combine_nodes(ball, "over", 7, max_words=want.size - 8)
    assert render.node_length == a.size
    assert np.array_equal(render.read_nodes(a.size + PAD), before)

    # the source is finer where it is pasted into a coarse leaf
    set_base(render, EMPTY_ROOT)
    held = render.read_nodes(8 + PAD)
    with pytest.raises(X.Refused) as e:
        X.combine(EMPTY_ROOT, 8, b, "over", 5)
    message = refused(ERR_STATE, depth=5, n_words=8)
    assert "over meets cell (%d, %d, %d)" % e.value.cell in message and "the source is an interior node" in message
    # a malformed source: only the pointers that the call follows, and before the depth refusal
    bad = b.copy()
    first = int(np.flatnonzero(bad[:8] >> 4 < B.VOXEL_OFFSET)[0])
    bad[first] = (b.size + 8) << 4
    message = refused(ERR_STATE, src=on_device(own_gpu, bad), depth=5, n_words=8)
    assert "malformed source" in message and "leaves the first src_words" in message
    bad[first] = 12 << 4
    unaligned = on_device(own_gpu, bad)
    message = refused(ERR_STATE, src=unaligned, n_words=8)
    assert "malformed source" in message and "not a multiple of 8" in message
    assert np.array_equal(render.read_nodes(8 + PAD), held)
    solid = np.full(8, leaf(0x102030), dtype=np.uint32)
    set_base(render, solid)
    assert raw_combine(pkg, own_gpu, unaligned, X.UNDER, 7, 8, b.size) == (0, 8)  # (never looked at)
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
        message = refused(ERR_STATE, src=paint, op=X.PAINT, depth=5, n_words=words.size, src_words=8)
        assert "malformed tree" in message and part in message, (name, message)
        assert np.array_equal(render.read_nodes(words.size + PAD), held), name

    set_base(render, a, want.size - a.size)
    assert raw_combine(pkg, own_gpu, ball, X.OVER, 7, a.size, b.size, max_words=want.size) == (0, want.size)
    assert_words(render.read_nodes(want.size), want, "the cap exactly reached")

    # without a node buffer, and with an adaptive state attached: both before n_words is looked at
    fresh = pkg.Gpu(0)
    try:
        assert raw_combine(pkg, fresh, ball, 0, 7, 12, b.size)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
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
        assert raw_combine(pkg, g, ball, 0, 7, 12, b.size)[0] == ERR_STATE and "adaptive" in last_error(pkg, g)
        assert np.array_equal(r.read_nodes(), held)
        del attached
    finally:
        g.close()


@pytest.mark.parametrize("op", ["carve", "over"])
def test_compaction_and_simplification_afterwards(render, sources, op):
    (a, ga), (b, gb) = trees7()["base"], trees7()["ball"]
    combined, _ = check_combine(render, a, b, sources["ball"], op, 7, op, runs=1)
    cells = X.apply_cells(ga, gb, op, (0, 0, 0), 7)
    want = K.compact(combined, combined.size, True)[0]
    assert render.compact_nodes(prune=True) == want.size and (op != "carve" or want.size < combined.size)
    assert_words(render.read_nodes(), want, f"{op}, compacted")
    assert np.array_equal(sampled(render, 7), cells)
    merged = M.simplify(want, want.size)[0]
    assert render.simplify_nodes() == merged.size
    assert_words(render.read_nodes(), merged, f"{op}, simplified")
    assert np.array_equal(sampled(render, 7), cells)


def test_a_combined_tree_traces_like_the_oracle(pkg, O):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    (a, _), (b, _), (w, _) = trees7()["base"], trees7()["ball"], trees7()["words"]
    pasted = trees7()["pasted"][0]
    carved = X.combine(pasted, pasted.size, w, "carve", 7)[0]
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    hits_base, hits_pasted, hits_carved = (O.trace_frame(t, u, threads=4) for t in (a, pasted, carved))
    assert (hits_pasted["value"] != hits_base["value"]).sum() > 50 and (hits_carved["value"] != hits_pasted["value"]).sum() > 0
    g1, g2 = pkg.Gpu(0), pkg.Gpu(0)
    try:
        r1 = pkg.Render(g1, (64, 64), a, capacity=CAPACITY)
        assert_hits_equal(frame(pkg, r1, u), hits_base, "the base")
        assert r1.combine_nodes(on_device(g1, b), "over", 7) == pasted.size
        assert_words(r1.read_nodes(), pasted, "pasted")
        assert_hits_equal(frame(pkg, r1, u), hits_pasted, "the pasted ball")
        # the next combine through a second context that shares the store; traced through the first
        r2 = pkg.Render.share_nodes(g2, r1)
        assert r2.combine_nodes(on_device(g2, w), "carve", 7) == carved.size
        g2.sync()
        r1.node_length = r2.node_length
        assert_words(r1.read_nodes(), carved, "carved through the sharing context")
        assert_hits_equal(frame(pkg, r1, u), hits_carved, "carved, on the context that did not combine")
        assert_hits_equal(frame(pkg, r2, u), hits_carved, "carved, on the context that combined")
    finally:
        g2.close()
        g1.close()
