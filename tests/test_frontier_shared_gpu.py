"""The one frontier-walk workspace of a context (csrc/svo_frontier.h), which the shape edit, the combine, the
placement, the morphology and the height-map edit take turns in: the five passes interleaved on one Render in two orders,
every pass once with a frontier larger than the call before it and once with a smaller one, so that the shared arrays grow and
hold stale tails; a refused call of one pass followed by a call of another; and every pass's times, which stay its own.  After
every call the words equal the pass's restatement (region_ref, combine_ref, place_ref, morph_ref, heightmap_ref) and what the
same call writes on a context that no other pass has used.  The trees are 32^3 grids: a merged ball, a height field, one voxel."""
import functools

import numpy as np
import pytest

import build_ref as B
import combine_ref as X
import heightmap_ref as H
import morph_ref as M
import place_ref as P
import region_ref as R
import simplify_ref
from pass_frame import assert_words, own_gpu  # noqa: F401
from test_combine_gpu import on_device
from test_compact_host import malformed_cases
from test_edit_gpu import PAD, ROOT, poison, set_base
from test_heightmap_gpu import edit_on_gpu
from test_region_gpu import to_shapes
from test_simplify_host import ball_voxels, field_voxels

pytestmark = pytest.mark.gpu

DEPTH = 5
CAPACITY = 1 << 17
PASSES = ("region", "combine", "place", "morph", "heightmap")


@functools.lru_cache(maxsize=None)
def trees():
    """name -> words.  Computed once; nobody writes to the arrays."""
    ball = B.build(*ball_voxels(DEPTH)[:1], DEPTH, ball_voxels(DEPTH)[1])
    field = B.build(field_voxels(DEPTH, False)[0], DEPTH, field_voxels(DEPTH, False)[1])
    return {"ball": simplify_ref.simplify(ball, ball.size)[0], "field": field, "dot": B.build(np.array([[9, 20, 14]]), DEPTH, np.array([0xC08040])),
            "dot2": B.build(np.array([[9, 21, 14], [30, 1, 2]]), DEPTH, np.array([0x4080C0, 0x102030])),
            "corner": B.build(np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1]]), 1, np.array([0x111111, 0x222222, 0x333333])),
            "unaligned": malformed_cases()["an unaligned pointer"]}


def terrain(sx, sz):
    x, z = np.meshgrid(np.arange(sx), np.arange(sz), indexing="ij")
    return (6 + (x * 5 + z * 3) % 17).astype(np.int64)


# name -> (pass, the scene, what the call takes); per pass a call with a small frontier and one with a large one
CALLS = {
    "region small": ("region", "dot", [R.box((3, 3, 3), (5, 6, 4), 0x0A0B0C)]),
    "region big": ("region", "field", [R.ball((30, 36, 33), 27, 0x808000), R.box((0, 0, 0), (32, 32, 32), 0x00A0A0, R.MODE_VOXELS)]),
    "combine small": ("combine", "dot", ("dot2", "over")),
    "combine big": ("combine", "field", ("ball", "over")),
    "place small": ("place", "dot", ("corner", "over", (7, 9, 11), 5, 1)),
    "place big": ("place", "field", ("ball", "under", (-3, 4, 2), 13, DEPTH)),
    "morph small": ("morph", "dot", ("grow", 6, 0, False)),
    "morph big": ("morph", "ball", ("grow", 26, 0x30C8F0, False)),
    "heightmap small": ("heightmap", "dot", (terrain(2, 2), (10, 12), H.params(((0, 0x3A9D23),)))),
    "heightmap big": ("heightmap", "field", (terrain(32, 32), (0, 0), H.params(H.TERRAIN, above="set"))),
}
# every pass follows a call with a smaller frontier once and one with a larger frontier once, in either order
ORDERS = {
    "region first": ("region small", "combine big", "place small", "morph big", "heightmap small",
                     "region big", "combine small", "place big", "morph small", "heightmap big", "region small"),
    "heightmap first": ("heightmap small", "morph big", "place small", "combine big", "region small",
                        "heightmap big", "morph small", "place big", "combine small", "region big", "heightmap small"),
}


def restated(kind, scene, args, depth=DEPTH):
    """the pass's restatement on the scene's words -> (words, tallies); raises what the restatement raises"""
    if kind == "region":
        return R.edit(scene, scene.size, R.shapes(args), depth)
    if kind == "combine":
        return X.combine(scene, scene.size, trees()[args[0]], args[1], depth)
    if kind == "place":
        source, op, offset, orient, src_depth = args
        return P.place(scene, scene.size, trees()[source], op, depth, offset, orient, src_depth)
    if kind == "morph":
        op, conn, colour, open_b = args
        return M.morph(scene, scene.size, op, conn, depth, colour, open_b)
    heights, origin, p = args
    return H.edit(scene, scene.size, heights, origin, depth, p)


@functools.lru_cache(maxsize=None)
def wanted(name):
    kind, scene, args = CALLS[name]
    return restated(kind, trees()[scene], args)


def frontier_words(tally):
    return 8 * (1 + tally["opened"] + tally["splits"])


def run(pkg, render, kind, args, depth=DEPTH, **kw):
    """the call on the GPU -> the new length"""
    if kind == "region":
        return render.edit_region(to_shapes(pkg, args), depth, **kw)
    if kind == "combine":
        return render.combine_nodes(on_device(render.gpu, trees()[args[0]]), args[1], depth, **kw)
    if kind == "place":
        source, op, offset, orient, src_depth = args
        return render.place_nodes(on_device(render.gpu, trees()[source]), op, depth, offset=offset, orient=orient, src_depth=src_depth, **kw)
    if kind == "morph":
        op, conn, colour, open_b = args
        return render.morph_nodes(op, 1, conn, colour or None, depth, open_b, **kw)
    heights, origin, p = args
    return edit_on_gpu(render, heights, origin, depth, p, **kw)


def check_call(pkg, render, name, what):
    """the scene -> the call on `render` == the restatement, with the words behind the new length as they were"""
    kind, scene, args = CALLS[name]
    base, (want, _) = trees()[scene], wanted(name)
    growth = want.size - base.size
    set_base(render, base, growth)
    n = run(pkg, render, kind, args)
    assert n == want.size == render.node_length, f"{what}: length {n}, want {want.size}"
    got = render.read_nodes(n + PAD)
    assert_words(got[:n], want, what)
    assert np.array_equal(got[n:], poison(growth + PAD)[growth:]), f"{what}: words behind the new length were written"


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture
def fresh(pkg, own_gpu):
    """a context that no pass has used, with a Render of its own (after own_gpu: the module has a device)"""
    g = pkg.Gpu(0)
    yield pkg.Render(g, (64, 64), ROOT, capacity=CAPACITY)
    g.close()


def test_the_orders_are_what_they_claim():
    """by the restatements' tallies: in both orders every pass has a frontier larger than the call before it in one of its two
    calls and a smaller one in the other; the large ones go beyond a scan tile's 4 096 words (csrc/svo_scan.h) and so beyond one
    workgroup, the small ones fill no workgroup's 256 lanes"""
    for order, names in ORDERS.items():
        sizes = [frontier_words(wanted(name)[1]) for name in names]
        larger = {p: [] for p in PASSES}
        for k in range(1, len(names)):
            larger[CALLS[names[k]][0]].append(sizes[k] > sizes[k - 1])
        for p in PASSES:
            assert sorted(larger[p]) == [False, True], (order, p, sizes)
    for name in CALLS:
        words = frontier_words(wanted(name)[1])
        assert words > 4096 if name.endswith("big") else words < 256, (name, words)


@pytest.mark.parametrize("order", list(ORDERS))
def test_interleaved_passes_equal_their_restatements(pkg, order):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg.Gpu(0)  # a context of the order's own: its workspace starts empty and only grows
    try:
        render = pkg.Render(g, (64, 64), ROOT, capacity=CAPACITY)
        for k, name in enumerate(ORDERS[order]):
            check_call(pkg, render, name, f"{order}, call {k}: {name}")
    finally:
        g.close()


@pytest.mark.parametrize("name", list(CALLS))
def test_a_fresh_context_gives_the_same_words(pkg, fresh, name):
    check_call(pkg, fresh, name, f"{name} on a context of its own")


def refusals():
    """name -> (the refused call: pass, scene words, args, depth, keywords, part of its message; the call behind it)"""
    bad = malformed_cases()
    cap = {name: wanted(name)[0].size - 8 for name in ("combine big", "heightmap big")}
    return {
        "region, finer than depth": (("region", trees()["field"], [R.box((0, 0, 0), (16, 16, 16), 7, R.MODE_VOXELS)], 4, {}, "which is an interior node at depth 4"),
                                     "morph big"),
        "morph, finer than depth": (("morph", trees()["ball"], CALLS["morph big"][2], 4, {}, "where the tree is finer than depth 4"), "heightmap big"),
        "combine, max_words": (("combine", trees()["field"], CALLS["combine big"][2], DEPTH, {"max_words": cap["combine big"]},
                                f"the combined tree needs {cap['combine big'] + 8} words, over the limit of {cap['combine big']}"), "heightmap small"),
        "heightmap, max_words": (("heightmap", trees()["field"], CALLS["heightmap big"][2], DEPTH, {"max_words": cap["heightmap big"]},
                                  f"the edited tree needs {cap['heightmap big'] + 8} words, over the limit of {cap['heightmap big']}"), "place big"),
        "morph, a group reached twice": (("morph", bad["two parents sharing one group"], ("grow", 6, 0, False), DEPTH, {},
                                          "malformed tree: a group is reached twice"), "place small"),
        "heightmap, an unaligned pointer": (("heightmap", bad["an unaligned pointer"], (terrain(16, 16), (0, 0), H.params(H.TERRAIN, "voxels", "voxels", 0x010101)), 4, {},
                                             "is not a multiple of 8"), "combine big"),
        "region, a pointer out of range": (("region", bad["a pointer with pointer + 8 > n_words"], [R.box((0, 0, 0), (32, 32, 32), 7, R.MODE_VOXELS)], DEPTH,
                                            {}, "leaves the first n_words"), "morph small"),
        "place, a malformed source": (("place", trees()["field"], ("unaligned", "over", (0, 0, 0), 0, 4), DEPTH, {}, "malformed source: an interior pointer at level"),
                                      "region big"),
    }


@pytest.mark.parametrize("name", list(refusals()))
def test_a_refused_call_then_another_pass(pkg, render, name):
    (kind, scene, args, depth, kw, part), then = refusals()[name]
    if "finer" in name:  # the restatement refuses it too, and names the cell
        with pytest.raises((R.Refused, M.Refused)) as r:
            restated(kind, scene, args, depth)
        part = "meets cell (%d, %d, %d), " % r.value.cell + part
    set_base(render, scene)
    before = render.read_nodes(scene.size + PAD)
    with pytest.raises(pkg.SvoError) as e:
        run(pkg, render, kind, args, depth, **kw)
    assert part in str(e.value), f"{name}: the refusal says {e.value}"
    assert render.node_length == scene.size and np.array_equal(render.read_nodes(scene.size + PAD), before), f"{name}: a refused call wrote"
    check_call(pkg, render, then, f"{then} behind {name}")


TIMINGS = {"region": ("region_timing", 5, "no tree edited by shapes"), "combine": ("combine_timing", 5, "no trees combined"),
           "place": ("place_timing", 5, "no tree placed"), "morph": ("morph_timing", 5, "no morphology step"),
           "heightmap": ("heightmap_timing", 6, "no tree edited by a height map")}


@pytest.mark.parametrize("first", PASSES)
def test_a_passes_times_are_its_own(pkg, fresh, first):
    """on a context where only `first` has run, the other passes' timing calls refuse with their own words; then every other
    pass runs, and `first`'s times are read again: the same floats"""
    check_call(pkg, fresh, first + " big", first)
    call, count, _ = TIMINGS[first]
    ms = getattr(fresh.gpu, call)()
    assert len(ms) == count and all(t >= 0 for t in ms) and ms[0] > 0 and ms[-1] > 0
    for other in PASSES:
        if other != first:
            with pytest.raises(pkg.SvoError) as e:
                getattr(fresh.gpu, TIMINGS[other][0])()
            assert TIMINGS[other][2] in str(e.value), (first, other, str(e.value))
    for other in PASSES:
        if other != first:
            check_call(pkg, fresh, other + " small", f"{other} behind {first}")
            assert getattr(fresh.gpu, call)() == ms, (first, other)
