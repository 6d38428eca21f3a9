"""Two trees combined (csrc/svo_combine.hip), CPU side: the rule's restatement (tests/combine_ref.py: combine)
makes trees that sample (tests/sample_ref.py) to the per-cell contract (apply_cells), for every op on the depth-7 base of the
pass tests against a merged ball and against a tree in edit order, on a depth-4 case whose words are written out here, with
the source placed in a cell of level 3, with the source equal to the scene and empty, and at the depth limit; a second
application changes nothing; the parameter record has the header's layout and the entry points are exported."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import build_ref as B
import combine_ref as X
import sample_ref as S
from conftest import ROOT as REPO
from pass_frame import tree7_base

NEW = ("svo_nodes_combine", "svo_combine_timing")
WHOLE7 = ((0, 0, 0), (128, 128, 128))
EMPTY_ROOT = np.full(8, B.EMPTY, dtype=np.uint32)
# the tallies that an op's cases are there to show: each non-zero in the restatement, so the cases prove that it happened
SHOWS = {"over": ("splits", "collapses"), "under": ("carried", "overwrites"), "paint": ("carried",), "carve": ("collapses", "splits"),
         "keep": ("collapses",), "replace": ("collapses", "splits")}


def leaf(v):
    return (B.VOXEL_OFFSET + v) << 4


def grid7(words):
    return S.sample_dense(words, words.size, *WHOLE7, 7)


@functools.lru_cache(maxsize=None)
def trees7():
    """the depth-7 scene and sources with their whole grids, computed once per session; nobody writes to the arrays.
    "base": the scene of every case; "ball": the merged two-coloured ball (coarse leaves); "words": the base edited in put
    order, a layout that no compaction made; "pasted": the base with the ball pasted over it, the scene with coarse VOXELS
    that a carve needs before it can split one -- every voxel of the base is a cell of the deepest level"""
    t = tree7_base()
    out = {"base": t["base"], "ball": X.ball_source(), "words": t["words"]}
    assert out["base"].size == 182304
    out["pasted"] = X.combine(out["base"], out["base"].size, out["ball"], "over", 7)[0]
    return {name: (w, grid7(w)) for name, w in out.items()}


def cases7():
    """(name, scene, source, op): every op on the base against both sources, and the carve of the pasted scene"""
    return [(f"{op}, {src}", "base", src, op) for op in X.OPS for src in ("ball", "words")] + [("carve, pasted scene", "pasted", "words", "carve")]


@pytest.mark.parametrize("name,scene,source,op", cases7(), ids=[c[0] for c in cases7()])
def test_the_rule_samples_to_the_per_cell_contract(name, scene, source, op):
    (a, grid_a), (b, grid_b) = trees7()[scene], trees7()[source]
    counted = a.copy()
    counted[:8] |= np.arange(1, 9, dtype=np.uint32)  # hit counters in the root group
    words, tally = X.combine(counted, counted.size, b, op, 7)
    assert words.dtype == np.uint32 and words.size == a.size + 8 * tally["splits"]
    kept = words[:8] >> 4 == counted[:8] >> 4
    assert np.array_equal((words[:8] & 15)[kept], (counted[:8] & 15)[kept]) and (words[:8][~kept] & 15 == 0).all() and kept.any()
    assert np.array_equal(grid7(words), X.apply_cells(grid_a, grid_b, op, (0, 0, 0), 7)), name
    # idempotence: the same source on the result writes nothing and appends nothing
    again, tally2 = X.combine(words, words.size, b, op, 7)
    assert np.array_equal(again, words) and tally2["splits"] == tally2["collapses"] == tally2["overwrites"] == 0


@pytest.mark.parametrize("op", X.OPS)
def test_an_ops_cases_show_its_tallies(op):
    """Over an op's cases every tally it is there to show is non-zero.  The base's voxels all lie on the deepest level, where
    nothing is split, so no source makes a carve of the base split anything: that is the pasted scene's case."""
    total = dict.fromkeys(X.TALLIES, 0)
    for name, scene, source, case_op in cases7():
        if case_op == op:
            a, b = trees7()[scene][0], trees7()[source][0]
            tally = X.combine(a, a.size, b, op, 7)[1]
            for key in X.TALLIES:
                total[key] += tally[key]
            if scene == "base" and source == "ball":  # the case that alone has to show all of them, the carve's splits apart
                for key in SHOWS[op]:
                    assert tally[key] > 0 or (op, key) == ("carve", "splits"), (name, key, tally)
    for key in SHOWS[op]:
        assert total[key] > 0, (op, key, total)


def test_a_depth_4_case_by_hand():
    """The scene: one level-1 voxel A over the cells [0, 8)^3, with a hit counter, and a level-2 voxel D over [12, 16)^3 under the
    root's child 7.  The source: its child 0 is a group whose child 7, the cells [4, 8)^3, is the voxel P; its child 7 is the
    voxel Q over [8, 16)^3."""
    A, D, P, Q, E = 0xA1B2C3, 0x0D0D0D, 0x00BEEF, 0x123456, B.EMPTY
    scene = np.array([leaf(A) | 5, E, E, E, E, E, E, 8 << 4] + [E] * 7 + [leaf(D)], dtype=np.uint32)
    source = np.array([8 << 4 | 3, E, E, E, E, E, E, leaf(Q) | 9] + [E] * 7 + [leaf(P)], dtype=np.uint32)
    ga, gb = (S.sample_dense(w, 16, (0, 0, 0), (16,) * 3, 4) for w in (scene, source))
    want = {
        # A is split (its colour carried down, counter 0) and P pasted into the new group; Q collapses the group under child 7
        "over": [16 << 4, E, E, E, E, E, E, leaf(Q)] + [E] * 7 + [leaf(D)] + [leaf(A)] * 7 + [leaf(P)],
        # A stays whatever the source holds (counter kept); Q is carried into the group under child 7 and fills its empty words
        "under": [leaf(A) | 5, E, E, E, E, E, E, 8 << 4] + [leaf(Q)] * 7 + [leaf(D)],
        # A is split for P's cube; D takes Q's colour, the empty words beside it stay empty
        "paint": [16 << 4, E, E, E, E, E, E, 8 << 4] + [E] * 7 + [leaf(Q)] + [leaf(A)] * 7 + [leaf(P)],
        "carve": [16 << 4, E, E, E, E, E, E, E] + [E] * 7 + [leaf(D)] + [leaf(A)] * 7 + [E],
        # Q covers the group under child 7: untouched with its subtree
        "keep": [16 << 4, E, E, E, E, E, E, 8 << 4] + [E] * 7 + [leaf(D)] + [E] * 7 + [leaf(A)],
        "replace": [16 << 4, E, E, E, E, E, E, leaf(Q)] + [E] * 7 + [leaf(D)] + [E] * 7 + [leaf(P)],
    }
    tallies = {"over": (1, 1, 1, 0, 0), "under": (0, 0, 7, 1, 8), "paint": (1, 0, 2, 1, 8), "carve": (1, 1, 1, 0, 0), "keep": (1, 0, 7, 0, 0),
               "replace": (1, 1, 8, 0, 0)}
    for op in X.OPS:
        words, tally = X.combine(scene, 16, source, op, 4)
        assert np.array_equal(words, np.array(want[op], dtype=np.uint32)), (op, words, want[op])
        assert tuple(tally[k] for k in X.TALLIES) == tallies[op], (op, tally)
        assert np.array_equal(S.sample_dense(words, words.size, (0, 0, 0), (16,) * 3, 4), X.apply_cells(ga, gb, op, (0, 0, 0), 4)), op


def small_source():
    """a depth-4 model: 300 random voxels in two colours and a solid 8^3 corner, which builds into one coarse leaf once merged"""
    import simplify_ref as M
    rng = np.random.default_rng(27)
    cells = np.concatenate([rng.integers(0, 16, (300, 3)), S.box_cells((8, 8, 8), (8, 8, 8))])
    built = B.build(cells, 4, np.where(np.arange(len(cells)) < 300, 0x00FF40, 0x7F00FF))
    return M.simplify(built, built.size)[0]


def test_a_source_placed_in_a_cell_of_level_3():
    src = small_source()
    gb = S.sample_dense(src, src.size, (0, 0, 0), (16,) * 3, 4)
    assert (gb == 0x7F00FF).sum() >= 512 and (gb == 0).sum() > 1000
    at = (3, 3, 3)  # the cells [48, 64)^3: inside the ball
    # the pasted scene holds one coarse voxel there: the path ends in a scene leaf, which is split and keeps its colour
    a, ga = trees7()["pasted"]
    assert len(set(ga[48:64, 48:64, 48:64].ravel().tolist())) == 1 and ga[48, 48, 48] != 0
    words, tally = X.combine(a, a.size, src, "under", 7, 3, at)
    assert np.array_equal(words, a) and tally["opened"] == 2 and tally["levels"] == [(8, 0)] * 3  # (a voxel stays whatever is put under it)
    for op in ("over", "carve", "replace"):
        words, tally = X.combine(a, a.size, src, op, 7, 3, at)
        assert tally["splits"] > 0 and words.size == a.size + 8 * tally["splits"]
        carried = (words[a.size:] == leaf(int(ga[48, 48, 48]))).sum()  # in the new groups: the colour carried down (a replace writes over all of it)
        assert carried == 0 if op == "replace" else carried > 100
        want = X.apply_cells(ga, gb, op, at, 4)
        assert np.array_equal(grid7(words), want), op
        outside = np.ones(ga.shape, dtype=bool)
        outside[48:64, 48:64, 48:64] = False
        assert np.array_equal(want[outside], ga[outside]) and not np.array_equal(want, ga)
    # a path that is split above at_level: the masked scene is one empty leaf of level 2 over [0, 32)^3
    masked = X.combine(trees7()["base"][0], 182304, trees7()["ball"][0], "keep", 7)[0]
    gm = grid7(masked)
    assert masked[masked[0] >> 4] == B.EMPTY  # the root's child 0 is interior, its child 0 an empty leaf
    words, tally = X.combine(masked, masked.size, src, "over", 7, 3, (1, 0, 1))
    assert tally["levels"][1][1] == 1 and tally["levels"][2][1] == 1 and np.array_equal(grid7(words), X.apply_cells(gm, gb, "over", (1, 0, 1), 4))
    # the base is interior along the whole path: nothing is split above the source's root
    a, ga = trees7()["base"]
    words, tally = X.combine(a, a.size, src, "over", 7, 3, at)
    assert [s for _, s in tally["levels"][:3]] == [0, 0, 0] and [n for n, _ in tally["levels"][:4]] == [8, 8, 8, 8] and tally["splits"] > 0
    assert np.array_equal(grid7(words), X.apply_cells(ga, gb, "over", at, 4))


def test_a_source_equal_to_the_scene():
    a, ga = trees7()["words"]
    for op in ("over", "under", "paint", "replace"):
        words, tally = X.combine(a, a.size, a.copy(), op, 7)
        assert np.array_equal(words, a) and tally["splits"] == tally["collapses"] == tally["overwrites"] == 0, op
    words, tally = X.combine(a, a.size, a.copy(), "carve", 7)
    assert tally["overwrites"] == (ga != 0).sum() > 0 and (grid7(words) == 0).all()
    words, tally = X.combine(a, a.size, a.copy(), "keep", 7)
    assert np.array_equal(words, a)


def test_an_empty_source():
    a, ga = trees7()["base"]
    assert (a[:8] >> 4 < B.VOXEL_OFFSET).all()
    words, tally = X.combine(a, a.size, EMPTY_ROOT, "keep", 7)
    assert tally["collapses"] == 8 and (words[:8] == B.EMPTY).all() and np.array_equal(words[8:], a[8:])
    for op in ("over", "under", "paint", "carve"):
        words, tally = X.combine(a, a.size, EMPTY_ROOT, op, 7)
        assert np.array_equal(words, a) and not any(tally[k] for k in X.TALLIES), op
    words, tally = X.combine(a, a.size, EMPTY_ROOT, "replace", 7)
    assert tally["collapses"] == 8 and (words[:8] == B.EMPTY).all()


def test_what_the_rule_refuses():
    a, ga = trees7()["base"]
    ball = trees7()["ball"][0]
    # the scene is finer than depth 5 where the ball's surface makes a paste open it; the source where it is pasted into a coarse leaf
    with pytest.raises(X.Refused) as e:
        X.combine(a, a.size, ball, "over", 5)
    assert e.value.finer == "both" and all(0 <= v < 32 for v in e.value.cell)
    with pytest.raises(X.Refused) as e:
        X.combine(EMPTY_ROOT, 8, ball, "over", 5)
    assert e.value.finer == "source"
    with pytest.raises(X.Refused) as e:
        X.combine(a, a.size, np.full(8, leaf(7), dtype=np.uint32), "paint", 5)
    assert e.value.finer == "scene" and e.value.cell == tuple(int(v) for v in np.argwhere(S.sample_dense(a, a.size, (0, 0, 0), (32,) * 3, 5) == S.FINER)[0])
    # not refused: where the op leaves the scene word untouched, a source deeper than `depth` under it is never looked at
    solid = np.full(8, leaf(0x102030), dtype=np.uint32)
    for op, scene in (("under", solid), ("paint", EMPTY_ROOT), ("carve", EMPTY_ROOT), ("keep", EMPTY_ROOT)):
        words, tally = X.combine(scene, 8, ball, op, 1)
        assert np.array_equal(words, scene) and not any(tally[k] for k in X.TALLIES), op
    # ... and a scene deeper than `depth` under a source word that decides it as a whole
    words, tally = X.combine(a, a.size, solid, "carve", 1)
    assert tally["collapses"] == 8 and (words[:8] == B.EMPTY).all()
    assert np.array_equal(X.combine(a, a.size, EMPTY_ROOT, "over", 1)[0], a)
    # malformed trees: only the pointers that the call follows
    bad = ball.copy()
    first = int(np.flatnonzero(bad[:8] >> 4 < B.VOXEL_OFFSET)[0])
    bad[first] = (ball.size + 8) << 4
    with pytest.raises(X.Malformed) as e:
        X.combine(EMPTY_ROOT, 8, bad, "over", 7)
    assert e.value.which == "source" and "leaves the first src_words" in str(e.value)
    bad[first] = 12 << 4
    with pytest.raises(X.Malformed) as e:
        X.combine(EMPTY_ROOT, 8, bad, "over", 7)
    assert e.value.which == "source" and "not a multiple of 8" in str(e.value)
    assert np.array_equal(X.combine(solid, 8, bad, "under", 7)[0], solid)  # (never looked at)
    twice = ball.copy()
    twice[:8] = twice[first]  # a source group reached through eight pointers is allowed: the result holds copies
    words, tally = X.combine(EMPTY_ROOT, 8, twice, "over", 7)
    gw = S.sample_dense(words, words.size, *WHOLE7, 7)
    assert tally["splits"] > 8 and np.array_equal(gw[:64, :64, :64], gw[64:, 64:, 64:])
    for kw in ({"op": 6}, {"depth": 0}, {"depth": 22}, {"at_level": 7}, {"at_level": 2, "at": (4, 0, 0)}):
        args = {"op": 0, "depth": 7, "at_level": 0, "at": (0, 0, 0), **kw}
        with pytest.raises(ValueError):
            X.combine(a, a.size, ball, **args)
    with pytest.raises(ValueError):
        X.combine(a, a.size, ball[:12], 0, 7)
    with pytest.raises(ValueError):
        X.combine(a, 12, ball, 0, 7)


def test_the_parameter_record_has_the_headers_layout(pkg):
    P = pkg._lib.CombineParams
    assert C.sizeof(P) == 48
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("op", 0, 4), ("depth", 4, 4), ("at_level", 8, 4), ("at", 12, 12), ("n_words", 24, 8), ("src_words", 32, 8), ("max_words", 40, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_combine_params \{(.*?)\} svo_combine_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+)(?:\[3\])?;", body) == [("uint32_t", "op"), ("uint32_t", "depth"), ("uint32_t", "at_level"),
                                                                        ("uint32_t", "at"), ("uint64_t", "n_words"), ("uint64_t", "src_words"),
                                                                        ("uint64_t", "max_words")]
    for value, name in enumerate(X.OPS):
        assert re.search(rf"#define SVO_COMBINE_{name.upper()}\s+{value}u", header) and pkg.render.COMBINE_OPS[value] == name
    assert re.search(r"#define SVO_COMBINE_TIMES 5\b[^\n]*\nint svo_combine_timing\(svo_ctx \*ctx, float ms_out\[SVO_COMBINE_TIMES\]\);", header)


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_combine.argtypes) == 4 and len(lib.svo_combine_timing.argtypes) == 2
    assert callable(pkg.Render.combine_nodes) and callable(pkg.Gpu.combine_timing)


def test_the_entry_points_appear_in_the_integration_guide():
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW + ("SvoCombineParams",):
        assert name in text, name
