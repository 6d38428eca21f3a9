"""A tree placed under an affine map on the GPU (csrc/svo_transform.hip): word for word against the rule's
restatement (tests/transform_ref.py: transform, which walks the source from its root for every item and knows no hint) and cell
for cell against the per-cell contract (apply_cells) on the cases of the host tests; nothing written behind the new length, on
an error or by a second identical call; the same bytes on every run; a signed permutation against place_nodes; the edges of the
arguments (depth 1 at all 27 offsets, a turned source at the two ends of a depth-21 scene, entries of 2^20 and a translation near
2^40 at depth 21 where the box arithmetic stands at its bound, factors of 16 either way, sources
handed over as tensors, as a Render and as simplify_nodes' pair); every error in the header's order; the canonical form after
simplification and compaction against a build of the mapped cells; the shared frontier workspace between a shape edit, a
transform and a morphology step; frames traced from a transformed tree against the oracle, also when the call came through a
context that shares the buffer."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import combine_ref as X
import morph_ref as M
import place_ref as P
import region_ref as R
import sample_ref as S
import transform_ref as T
from conftest import assert_hits_equal
from pass_frame import assert_words, last_error, own_gpu  # noqa: F401
from test_combine_gpu import on_device, sampled
from test_combine_host import EMPTY_ROOT, leaf, trees7
from test_edit_gpu import CAPACITY, ERR_ARG, ERR_CAP, ERR_STATE, PAD, ROOT, frame, poison, set_base
from test_place_host import case_named, placed, sources
from test_region_gpu import to_shapes
from test_transform_host import CASES, IDS, MAPS, TILE, fixed, numbers, rot, transformed

pytestmark = pytest.mark.gpu

IDENTITY = (65536, 0, 0, 0, 65536, 0, 0, 0, 65536)


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def tensors(own_gpu):
    """the shared sources in device memory, uploaded once"""
    return {name: on_device(own_gpu, words) for name, (words, _, _) in sources().items()}


def check_transform(render, scene, want, tensor, op, depth, what, matrix, translate, src_depth=None, runs=2):
    """scene -> transform_nodes on the GPU == `want`, the restatement's words; the words behind the new length keep what they
    held, and a second run from the same scene gives the same bytes"""
    growth = want.size - scene.size
    for run in range(runs):
        set_base(render, scene, growth)
        n = render.transform_nodes(tensor, op, depth, matrix=matrix, translate=translate, src_depth=src_depth)
        assert n == want.size == render.node_length, f"{what}: length {n}, want {want.size}"
        got = render.read_nodes(n + PAD)
        assert_words(got[:n], want, f"{what}, run {run}")
        assert np.array_equal(got[n:], poison(growth + PAD)[growth:]), f"{what}: words behind the new length were written"
    return want


@pytest.mark.parametrize("name,source,op,which", CASES, ids=IDS)
def test_the_host_cases(render, tensors, name, source, op, which):
    a, grid_a = trees7()["base"]
    _, grid_b, src_depth = sources()[source]
    want, tally = transformed(name)
    matrix, translate = numbers(source, which)
    check_transform(render, a, want, tensors[source], op, 7, name, matrix, translate, src_depth)
    if name == "over, ball, turn y 30":
        # a level's frontier and its splits go beyond one scan tile, and its groups fill no whole wave
        assert any(n > TILE and s > TILE and (n // 8) % 64 for n, s in tally["levels"]), tally["levels"]
    assert np.array_equal(sampled(render, 7), T.apply_cells(grid_a, grid_b, op, matrix, translate)), f"{name}: the cells"


def test_a_signed_permutation_gives_the_bytes_of_place_nodes(pkg, render, tensors):
    a = trees7()["base"][0]
    for op, source, offset in (("over", "ball", (1, 1, 1)), ("keep", "ball", (3, -5, 64)), ("replace", "model5", (-9, 110, 3))):
        name, _, _, _, orient = case_named(op, source, offset)
        src_depth = sources()[source][2]
        room = placed(name)[0].size - a.size
        set_base(render, a, room)
        n = render.place_nodes(tensors[source], op, 7, offset=offset, orient=orient, src_depth=src_depth)
        want = render.read_nodes(n + PAD)
        assert n == placed(name)[0].size
        matrix, translate = pkg.transform.from_orientation(orient, offset, src_depth)
        assert (tuple(matrix), tuple(translate)) == T.permutation(orient, offset, src_depth)
        set_base(render, a, room)
        assert render.transform_nodes(tensors[source], op, 7, matrix=matrix, translate=translate, src_depth=src_depth) == n
        assert_words(render.read_nodes(n + PAD), want, name)


def test_an_identical_second_call_writes_nothing(render, tensors):
    a = trees7()["base"][0]
    for op in ("over", "carve", "replace"):
        name = f"{op}, ball, turn y 30"
        matrix, translate = numbers("ball", "turn y 30")
        first = check_transform(render, a, transformed(name)[0], tensors["ball"], op, 7, name, matrix, translate, runs=1)
        whole = render.read_nodes(first.size + PAD)
        assert render.transform_nodes((tensors["ball"], sources()["ball"][0].size), op, 7, matrix=matrix, translate=translate) == first.size
        assert np.array_equal(render.read_nodes(first.size + PAD), whole), op
    ms = render.gpu.transform_timing()
    assert len(ms) == 5 and all(t >= 0 for t in ms) and ms[0] > 0 and ms[4] > 0


def test_untouched_words_keep_their_counters(render, tensors):
    a, b = trees7()["base"][0], sources()["ball"][0]
    rng = np.random.default_rng(35)
    counted = a | rng.integers(1, 16, a.size).astype(np.uint32)
    matrix, translate = numbers("ball", "turn y 30")
    want = T.transform(counted, counted.size, b, "under", 7, matrix, translate)[0]
    check_transform(render, counted, want, tensors["ball"], "under", 7, "a scene with hit counters", matrix, translate, runs=1)
    kept = want[: a.size] == counted
    assert kept.sum() > a.size // 2 and (~kept).sum() > 1000 and (want[: a.size][~kept] & 15 == 0).all() and (want[a.size:] & 15 == 0).all()
    # the source's counters are ignored
    src = b | rng.integers(1, 16, b.size).astype(np.uint32)
    check_transform(render, a, transformed("over, ball, turn y 30")[0], on_device(render.gpu, src), "over", 7, "a source with hit counters", matrix,
                    translate, runs=1)


def test_depth_1_at_all_27_offsets(render):
    scene = np.array([leaf(v) | c for v, c in zip([0, 0, 5, 5, 0x7FFFFFF, 9, 0, 3], range(8))], dtype=np.uint32)
    source = np.array([leaf(v) for v in [0, 7, 0, 7, 1, 0, 0, 0x7FFFFFF]], dtype=np.uint32)
    ga, gb = (S.sample_dense(w, 8, (0, 0, 0), (2,) * 3, 1) for w in (scene, source))
    tensor = on_device(render.gpu, source)
    for i, offset in enumerate((x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)):
        for op in X.OPS:
            orient = (7 * i + X.OPS.index(op)) % 48
            matrix, translate = T.permutation(orient, offset, 1)
            want, tally = T.transform(scene, 8, source, op, 1, matrix, translate, 1)
            cells = T.apply_cells(ga, gb, op, matrix, translate)
            assert np.array_equal(cells, P.apply_cells(ga, gb, op, offset, orient))
            check_transform(render, scene, want, tensor, op, 1, f"depth 1, {op} at {offset}", matrix, translate, 1, runs=1)
            assert want.size == 8 and np.array_equal(sampled(render, 1), cells), (op, offset)
            assert tally["overwrites"] == (ga != cells).sum()


def test_the_ends_of_the_integer_range_at_depth_21(render):
    """a depth-1 source of eight voxels turned by 45 degrees about y into an empty depth-21 scene, its centre on the scene's
    middle and two cells from its far corner: the products of the box reach 2^38 and the translation 2^37"""
    colours = [0x010203, 0x0A0B0C, 0x111111, 0x222222, 0x333333, 0x444444, 0x555555, 0xFFFFFF]
    source = np.array([leaf(v) for v in colours], dtype=np.uint32)
    tensor = on_device(render.gpu, source)
    for centre in (1 << 20, (1 << 21) - 2):
        matrix, translate = fixed(rot("y", 45), (centre,) * 3, 1)
        want, tally = T.transform(EMPTY_ROOT, 8, source, "over", 21, matrix, translate, 1)
        assert len(tally["levels"]) == 21 and tally["splits"] >= 20 and tally["overwrites"] == 8, tally
        check_transform(render, EMPTY_ROOT, want, tensor, "over", 21, f"depth 21 about {centre}", matrix, translate, 1)
        near = np.array([[centre + x, centre + y, centre + z] for x in (-2, -1, 0, 1) for y in (-1, 0) for z in (-2, -1, 0, 1)])
        q = (((2 * near + 1) @ np.array(matrix, dtype=np.int64).reshape(3, 3).T + 2 * np.array(translate, dtype=np.int64)) >> 17)
        hit = ((q >= 0) & (q < 2)).all(axis=1)
        expect = np.where(hit, np.array(colours)[np.clip(q[:, 0], 0, 1) * 4 + np.clip(q[:, 1], 0, 1) * 2 + np.clip(q[:, 2], 0, 1)], 0)
        assert hit.sum() == 8 and render.sample_voxels(near, 21).cpu().numpy().tolist() == expect.tolist()


def test_the_overflow_bound_at_depth_21(render, tensors):
    """Entries of +-2^20 and a translation near 2^40 in an empty depth-21 scene: the depth-5 model, shrunk by 16 and sheared,
    sampled about the cell (300 000, 300 001, 299 999).  The words of the levels beside the path to it have boxes far from the
    source: the far corner's mid passes 2^43 and a level-1 word's rad is (2^20 - 1) * 3 * 2^20, the largest there is, so the
    sums stand where the header's bound of 2^45 is about.  Word for word against the restatement, which computes in int64 and
    is itself checked here against Python's integers."""
    model, grid, src_depth = sources()["model5"]
    E = 1 << 20
    matrix = (E, E, E, E, -E, E, -E, E, E)
    at = (300000, 300001, 299999)
    translate = tuple(16 * 65536 - sum(matrix[3 * i + j] * (2 * at[j] + 1) for j in range(3)) // 2 for i in range(3))  # `at` samples the cell (16, 16, 16)
    assert max(abs(t) for t in translate) > 0.8 * (1 << 40) and max(abs(t) for t in translate) <= 1 << 40
    far = (1 << 21) - 1
    mids = [sum(matrix[3 * i + j] * (2 * far + 1) for j in range(3)) + 2 * translate[i] for i in range(3)]  # (Python's integers: no width)
    assert max(abs(v) for v in mids) > 1 << 43
    cells = np.array([at, (at[0] + 1, at[1], at[2]), (0, 0, 0), (far,) * 3])
    q = ((2 * cells + 1) @ np.array(matrix, dtype=np.int64).reshape(3, 3).T + 2 * np.array(translate, dtype=np.int64)) >> 17
    assert q[0].tolist() == [16, 16, 16] and q[3].tolist() == [v >> 17 for v in mids] and grid[16, 16, 16] != 0
    for op in ("over", "replace"):
        want, tally = T.transform(EMPTY_ROOT, 8, model, op, 21, matrix, translate, src_depth)
        assert len(tally["levels"]) == 21 and tally["splits"] >= 20 and tally["overwrites"] >= 1, tally
        check_transform(render, EMPTY_ROOT, want, tensors["model5"], op, 21, f"entries of 2^20 at depth 21, {op}", matrix, translate, src_depth)
        assert render.sample_voxels(cells, 21).cpu().numpy().tolist() == [int(grid[16, 16, 16]), 0, 0, 0]


def test_factors_of_16_either_way(render, tensors):
    # magnified by 16 (entries of 2^12): a depth-3 source fills the depth-7 scene, every source cell a cube of 16 cells
    rng = np.random.default_rng(36)
    cells = rng.integers(0, 8, (60, 3))
    small = B.build(cells, 3, rng.integers(1, 1 << 24, 60))
    grid_small = S.sample_dense(small, small.size, (0, 0, 0), (8,) * 3, 3)
    a, grid_a = trees7()["base"]
    matrix, translate = fixed(16 * np.eye(3), (64, 64, 64), 3)
    assert matrix == (4096, 0, 0, 0, 4096, 0, 0, 0, 4096) and translate == (0, 0, 0)
    for op in ("under", "replace"):
        want, tally = T.transform(a, a.size, small, op, 7, matrix, translate, 3)
        check_transform(render, a, want, on_device(render.gpu, small), op, 7, f"magnified, {op}", matrix, translate, 3, runs=1)
        got = sampled(render, 7)
        assert np.array_equal(got, T.apply_cells(grid_a, grid_small, op, matrix, translate))
    assert np.array_equal(got, np.repeat(np.repeat(np.repeat(grid_small, 16, 0), 16, 1), 16, 2)) and tally["splits"] == 0
    # shrunk by 16 (entries of 2^20): the depth-7 ball on eight cells a side, every cell one sample of 16^3
    _, grid_b, _ = sources()["ball"]
    matrix, translate = fixed(np.eye(3) / 16, (40.5, 90, 77.25), 7)
    assert max(matrix) == 1 << 20
    for op in ("over", "replace"):
        want, tally = T.transform(a, a.size, sources()["ball"][0], op, 7, matrix, translate, 7)
        check_transform(render, a, want, tensors["ball"], op, 7, f"shrunk, {op}", matrix, translate, 7, runs=1)
        cells = T.apply_cells(grid_a, grid_b, op, matrix, translate)
        assert np.array_equal(sampled(render, 7), cells) and 0 < (cells != grid_a).sum() <= 8 ** 3, op


def test_sources_from_a_simplification_and_from_another_render(pkg, render):
    a = trees7()["base"][0]
    b = sources()["ball"][0]
    name = "over, ball, turn y 30"
    want = transformed(name)[0]
    kw = dict(zip(("matrix", "translate"), numbers("ball", "turn y 30")))
    other = pkg.Gpu(0)
    try:
        cells = X.ball_cells(7, (128, 128, 128), 100)
        model = pkg.Render.from_voxels(other, (64, 64), cells, 7, np.where(cells[:, 0] < 64, 0x40C0FF, 0xFF8020), capacity=1 << 20)
        pair = model.simplify_nodes(out_of_place=True)
        assert pair[1] == b.size
        set_base(render, a, want.size - a.size)
        assert render.transform_nodes(pair, "over", 7, **kw) == want.size
        assert_words(render.read_nodes(), want, "the pair of simplify_nodes(out_of_place=True)")
        assert model.simplify_nodes() == b.size
        set_base(render, a, want.size - a.size)
        assert render.transform_nodes(model, "over", 7, **kw) == want.size
        assert_words(render.read_nodes(), want, "another Render")
        assert_words(model.read_nodes(), b, "the source, only read")
        set_base(render, a, want.size - a.size)
        assert render.transform_nodes(on_device(render.gpu, b), "over", 7, src_depth=7, **kw) == want.size
        assert_words(render.read_nodes(), want, "a tensor")
        with pytest.raises(ValueError):
            render.transform_nodes(model, "above", 7, **kw)
        with pytest.raises(ValueError):
            render.transform_nodes(model, "over", 7, matrix=IDENTITY[:8])
        with pytest.raises(ValueError, match="whole numbers"):  # a forward map in floats where Q16 was meant
            render.transform_nodes(model, "over", 7, matrix=pkg.transform.rotation("y", 30))
        assert render.node_length == want.size  # (refused before the call)
    finally:
        other.close()


def raw_transform(pkg, gpu, src, op, depth, n_words, src_words, src_depth=None, matrix=IDENTITY, translate=(0, 0, 0), max_words=0, params=True, out=True):
    """src: a device tensor, an address or None"""
    p = pkg._lib.TransformParams()
    p.op, p.depth, p.src_depth, p.n_words, p.src_words, p.max_words = op, depth, depth if src_depth is None else src_depth, n_words, src_words, max_words
    p.matrix[:] = list(matrix)
    p.translate[:] = list(translate)
    n_out = C.c_uint64(12345)
    ptr = src.data_ptr() if hasattr(src, "data_ptr") else src
    rc = pkg._lib.lib().svo_nodes_transform(gpu._h, ptr, C.byref(p) if params else None, C.byref(n_out) if out else None)
    gpu.sync()
    return rc, n_out.value


def test_errors_write_nothing(pkg, render, own_gpu, tensors):
    a = trees7()["base"][0]
    b = sources()["ball"][0]
    ball = tensors["ball"]
    turn = dict(zip(("matrix", "translate"), numbers("ball", "turn y 30")))
    set_base(render, a)
    before = render.read_nodes(a.size + PAD)
    err = lambda: last_error(pkg, own_gpu)  # noqa: E731

    def refused(code, src=ball, op=0, depth=7, n_words=a.size, src_words=b.size, **kw):
        assert raw_transform(pkg, own_gpu, src, op, depth, n_words, src_words, **kw)[0] == code, (op, depth, kw, err())
        return err()

    # in the header's order; of two causes the earlier one is reported
    big, far = (1 << 20) + 1, (1 << 40) + 1
    assert "null params" in refused(ERR_ARG, params=False)
    assert "n_words_out" in refused(ERR_ARG, out=False, op=9)
    assert "null source" in refused(ERR_ARG, src=None, op=9)
    assert "op must be 0..5 (got 6)" in refused(ERR_ARG, op=6, depth=0)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=0, src_depth=0)
    assert "depth must be 1..21" in refused(ERR_ARG, depth=22)
    assert "src_depth must be 1..21 (got 0)" in refused(ERR_ARG, src_depth=0, matrix=(big,) * 9)
    assert "src_depth must be 1..21 (got 22)" in refused(ERR_ARG, src_depth=22, matrix=(big,) * 9)
    assert "entry 8: 1048577" in refused(ERR_ARG, matrix=(0,) * 8 + (big,), translate=(far, 0, 0))
    assert "entry 0: -1048577" in refused(ERR_ARG, matrix=(-big,) + IDENTITY[1:], translate=(far, 0, 0))
    assert "axis 1: 1099511627777" in refused(ERR_ARG, translate=(0, far, 0), n_words=12)
    assert "axis 2: -1099511627777" in refused(ERR_ARG, translate=(0, 0, -far), n_words=12)
    for n_words in (0, 12, CAPACITY + 8):
        assert "n_words must be a positive multiple of 8" in refused(ERR_ARG, n_words=n_words, src_words=12)
    for src_words in (0, 12, (1 << 27) + 8):
        assert "src_words must be a positive multiple of 8" in refused(ERR_ARG, src_words=src_words)
    ptr, room = C.c_void_p(), C.c_size_t()
    own_gpu.check(pkg._lib.lib().svo_nodes_device_ptr(own_gpu._h, C.byref(ptr), C.byref(room)))
    assert room.value == CAPACITY
    for address, src_words in ((ptr.value, 8), (ptr.value + 4 * (CAPACITY - 8), 16), (ptr.value - 4 * 8, 16)):
        assert "overlaps the node buffer" in refused(ERR_ARG, src=address, src_words=src_words)
    # the ends of the ranges are allowed: every cell samples outside the source, nothing written
    assert raw_transform(pkg, own_gpu, ball, 5, 7, a.size, b.size, translate=(1 << 40, 0, -(1 << 40))) == (0, a.size)
    assert raw_transform(pkg, own_gpu, ball, 5, 7, a.size, b.size, matrix=(1 << 20,) * 9, translate=(-(1 << 40),) * 3) == (0, a.size)

    # the depth refusal names the cell and the tree; the restatement names the same
    seven = np.full(8, leaf(7), dtype=np.uint32)
    quarter = tuple(v // 4 for v in IDENTITY)
    for src, source, op, src_depth, kw, text in (
            (ball, b, "over", 5, {"matrix": IDENTITY, "translate": (0, 0, 0)}, "the scene and the source are interior nodes"),
            (ball, b, "over", 5, {"matrix": turn["matrix"], "translate": tuple(v // 4 for v in turn["translate"])}, None),
            (on_device(own_gpu, seven), seven, "paint", 1, {"matrix": quarter, "translate": (0, 0, 0)}, "the scene is an interior node")):
        with pytest.raises(X.Refused) as e:
            T.transform(a, a.size, source, op, 5, kw["matrix"], kw["translate"], src_depth)
        text = text or {"both": "the scene and the source are", "scene": "the scene is", "source": "the source is"}[e.value.finer]
        message = refused(ERR_STATE, src=src, op=X.OPS.index(op), depth=5, src_depth=src_depth, src_words=source.size, **kw)
        assert "%s meets cell (%d, %d, %d)" % ((op,) + e.value.cell) in message and text in message and "at depth 5" in message
    with pytest.raises(pkg.SvoError):
        render.transform_nodes(ball, "over", 5, src_depth=5)
    assert render.node_length == a.size
    # the cap: one group short of the restatement's length fails, exactly reached succeeds (below)
    want = transformed("over, ball, turn y 30")[0]
    assert want.size > a.size
    assert str(want.size) in refused(ERR_CAP, max_words=want.size - 8, **turn)
    with pytest.raises(pkg.SvoError):
        render.transform_nodes(ball, "over", 7, max_words=want.size - 8, **turn)
    assert render.node_length == a.size
    assert np.array_equal(render.read_nodes(a.size + PAD), before)

    # the source is finer than src_depth where it is pasted into a coarse leaf
    set_base(render, EMPTY_ROOT)
    held = render.read_nodes(8 + PAD)
    coarse = {"matrix": turn["matrix"], "translate": tuple(v // 4 for v in turn["translate"])}
    with pytest.raises(X.Refused) as e:
        T.transform(EMPTY_ROOT, 8, b, "over", 7, coarse["matrix"], coarse["translate"], 5)
    message = refused(ERR_STATE, n_words=8, src_depth=5, **coarse)
    assert "over meets cell (%d, %d, %d)" % e.value.cell in message and "the source is an interior node" in message
    # a malformed source: every pointer that the call follows, in the root group and below it, and before the depth refusal
    first = int(np.flatnonzero(b[:8] >> 4 < B.VOXEL_OFFSET)[0])
    below = int(b[first] >> 4) + int(np.flatnonzero(b[b[first] >> 4:][:8] >> 4 < B.VOXEL_OFFSET)[0])
    unaligned = None
    for at in (first, below):
        bad = b.copy()
        bad[at] = (b.size + 8) << 4
        with pytest.raises(X.Malformed) as e:
            T.transform(EMPTY_ROOT, 8, bad, "over", 7, turn["matrix"], turn["translate"], 7)
        message = refused(ERR_STATE, src=on_device(own_gpu, bad), n_words=8, **turn)
        assert str(e.value) in message and "leaves the first src_words" in message, (at, message, str(e.value))
        message = refused(ERR_STATE, src=on_device(own_gpu, bad), depth=5, n_words=8, **coarse)
        assert "malformed source" in message and "leaves the first src_words" in message
        bad[at] = 12 << 4
        unaligned = on_device(own_gpu, bad)
        with pytest.raises(X.Malformed) as e:
            T.transform(EMPTY_ROOT, 8, bad, "over", 7, turn["matrix"], turn["translate"], 7)
        message = refused(ERR_STATE, src=unaligned, n_words=8, **turn)
        assert str(e.value) in message and "not a multiple of 8" in message, (at, message, str(e.value))
    assert np.array_equal(render.read_nodes(8 + PAD), held)
    solid = np.full(8, leaf(0x102030), dtype=np.uint32)
    set_base(render, solid)
    assert raw_transform(pkg, own_gpu, unaligned, X.UNDER, 7, 8, b.size, **turn) == (0, 8)  # (never looked at)
    assert np.array_equal(render.read_nodes(8), solid)

    # malformed scenes, with the compaction's wording; a paint by one voxel over the whole grid opens every interior word
    from test_compact_host import malformed_cases
    paint = on_device(own_gpu, solid)
    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice"}
    cases = malformed_cases()
    for name, part in causes.items():
        words = cases[name]
        set_base(render, words)
        held = render.read_nodes(words.size + PAD)
        message = refused(ERR_STATE, src=paint, op=X.PAINT, depth=5, src_depth=1, n_words=words.size, src_words=8, matrix=(0,) * 9, translate=(65536,) * 3)
        assert "malformed tree" in message and part in message, (name, message)
        assert np.array_equal(render.read_nodes(words.size + PAD), held), name

    set_base(render, a, want.size - a.size)
    assert raw_transform(pkg, own_gpu, ball, X.OVER, 7, a.size, b.size, max_words=want.size, **turn) == (0, want.size)
    assert_words(render.read_nodes(want.size), want, "the cap exactly reached")

    # without a node buffer: before n_words is looked at
    fresh = pkg.Gpu(0)
    try:
        assert raw_transform(pkg, fresh, ball, 0, 7, 12, b.size)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
        ms = (C.c_float * 5)()
        assert pkg._lib.lib().svo_transform_timing(fresh._h, ms) == ERR_STATE and "no tree transformed" in last_error(pkg, fresh)
    finally:
        fresh.close()


def test_the_canonical_form_is_a_build_of_the_mapped_cells(pkg, render, tensors):
    """replace into an empty scene, then simplify and compact: byte for byte the tree built from the cells, after the same two"""
    b, grid_b, _ = sources()["ball"]
    matrix, translate = numbers("ball", "turn y 30")
    cells = T.apply_cells(np.zeros((128,) * 3, dtype=np.uint32), grid_b, "replace", matrix, translate)
    want = T.transform(EMPTY_ROOT, 8, b, "replace", 7, matrix, translate)[0]
    check_transform(render, EMPTY_ROOT, want, tensors["ball"], "replace", 7, "into an empty scene", matrix, translate, runs=1)
    assert np.array_equal(sampled(render, 7), cells)
    render.simplify_nodes()
    turned = render.read_nodes(render.compact_nodes())
    at = np.argwhere(cells != 0)
    assert abs(len(at) - (grid_b != 0).sum()) < 0.01 * len(at) and not np.array_equal(cells, grid_b)
    other = pkg.Gpu(0)
    try:
        built = pkg.Render.from_voxels(other, (64, 64), at, 7, cells[tuple(at.T)].astype(np.int64), capacity=CAPACITY)
        built.simplify_nodes()
        assert_words(turned, built.read_nodes(built.compact_nodes()), "turned, simplified and compacted against built")
    finally:
        other.close()


def test_a_shape_edit_a_transform_and_a_morphology_step_share_the_workspace(pkg):
    """one call each on one context, the frontiers small, large and middling: every call's words are its restatement's"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a = trees7()["base"][0]
    model, _, src_depth = sources()["model5"]
    g = pkg.Gpu(0)
    try:
        r = pkg.Render(g, (64, 64), a, capacity=CAPACITY)
        shapes = [R.box((3, 3, 3), (9, 12, 7), 0x0A0B0C)]
        want = R.edit(a, a.size, R.shapes(shapes), 7)[0]
        assert r.edit_region(to_shapes(pkg, shapes), 7) == want.size
        assert_words(r.read_nodes(), want, "the shape edit")
        matrix, translate = numbers("model5", "scale 1.5 turn z 45")
        want, tally = T.transform(want, want.size, model, "over", 7, matrix, translate, src_depth)
        assert tally["splits"] > 0 and r.transform_nodes(on_device(g, model), "over", 7, matrix=matrix, translate=translate, src_depth=src_depth) == want.size
        assert_words(r.read_nodes(), want, "the transform behind the shape edit")
        want = M.morph(want, want.size, "grow", 6, 7, 0x30C8F0, False)[0]
        assert r.morph_nodes("grow", 1, 6, 0x30C8F0, 7) == want.size
        assert_words(r.read_nodes(), want, "the morphology step behind the transform")
        again, tally = T.transform(want, want.size, model, "carve", 7, matrix, translate, src_depth)
        assert r.transform_nodes(on_device(g, model), "carve", 7, matrix=matrix, translate=translate, src_depth=src_depth) == again.size
        assert_words(r.read_nodes(), again, "a second transform behind the morphology step")
        assert len(g.transform_timing()) == 5 and len(g.region_timing()) == 5 and len(g.morph_timing()) == 5
    finally:
        g.close()


def test_a_transformed_tree_traces_like_the_oracle(pkg, O):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a = trees7()["base"][0]
    b = sources()["ball"][0]
    model, _, src_depth = sources()["model5"]
    pasted = transformed("over, ball, turn y 30")[0]
    matrix, translate = numbers("model5", "shear")  # (beside the ball, where the camera sees it)
    sheared = T.transform(pasted, pasted.size, model, "over", 7, matrix, translate, src_depth)[0]
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    hits_base, hits_pasted, hits_sheared = (O.trace_frame(t, u, threads=4) for t in (a, pasted, sheared))
    assert (hits_pasted["value"] != hits_base["value"]).sum() > 50 and (hits_sheared["value"] != hits_pasted["value"]).sum() > 0
    g1, g2 = pkg.Gpu(0), pkg.Gpu(0)
    try:
        r1 = pkg.Render(g1, (64, 64), a, capacity=CAPACITY)
        assert_hits_equal(frame(pkg, r1, u), hits_base, "the base")
        turn = dict(zip(("matrix", "translate"), numbers("ball", "turn y 30")))
        assert r1.transform_nodes(on_device(g1, b), "over", 7, **turn) == pasted.size
        assert_words(r1.read_nodes(), pasted, "pasted")
        assert_hits_equal(frame(pkg, r1, u), hits_pasted, "the turned ball")
        # the next transform through a second context that shares the store; traced through the first
        r2 = pkg.Render.share_nodes(g2, r1)
        assert r2.transform_nodes(on_device(g2, model), "over", 7, matrix=matrix, translate=translate, src_depth=src_depth) == sheared.size
        g2.sync()
        r1.node_length = r2.node_length
        assert_words(r1.read_nodes(), sheared, "sheared through the sharing context")
        assert_hits_equal(frame(pkg, r1, u), hits_sheared, "sheared, on the context that did not transform")
        assert_hits_equal(frame(pkg, r1, u), hits_sheared, "sheared, a second frame")
        assert_hits_equal(frame(pkg, r1, u), hits_sheared, "sheared, a third frame")
        assert_hits_equal(frame(pkg, r2, u), hits_sheared, "sheared, on the context that transformed")
    finally:
        g2.close()
        g1.close()
