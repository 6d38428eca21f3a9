"""A tree placed at any cell offset and orientation (csrc/svo_place.hip), CPU side: the rule's restatement
(tests/place_ref.py: place) makes trees that sample (tests/sample_ref.py) to the per-cell contract (apply_cells: numpy's
transpose, flip and slice) for every op on the depth-7 base of the combine's tests against the merged ball and a depth-5 model,
at offsets that align on some levels, on none, hang over the edge and lie outside; all 48 orientations of a source without a
symmetry differ and equal numpy's; an aligned placement gives the combine's words byte for byte; a second application changes
nothing; a depth-3 case whose words are written out here; what is refused; the parameter record has the header's layout, the
entry points are exported, and the orientation module numbers the symmetries as the header does."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import build_ref as B
import combine_ref as X
import place_ref as P
import sample_ref as S
from conftest import ROOT as REPO
from test_combine_host import EMPTY_ROOT, cases7, grid7, leaf, small_source, trees7

NEW = ("svo_nodes_place", "svo_place_timing")
TILE = 4096  # items of one scan tile (csrc/svo_scan.h)
# aligned on no level; on some axes at some levels; (4, 0, -8) on the levels of cells up to 4, all and 8; over the scene's
# edge on three sides (the depth-5 model lies wholly outside at x = -40); wholly outside; over the edge for both sources
OFFSETS = ((1, 1, 1), (3, -5, 64), (4, 0, -8), (-40, 17, 100), (200, 0, 0), (-9, 110, 3))


@functools.lru_cache(maxsize=None)
def sources():
    """name -> (words, their whole grid, src_depth): the combine's merged ball, and a depth-5 model, a two-coloured ball of
    radius 13 cells with 150 single voxels around it, merged.  Computed once per session; nobody writes to the arrays."""
    import simplify_ref as M
    rng = np.random.default_rng(30)
    cells = np.concatenate([X.ball_cells(5, (33, 31, 32), 26), rng.integers(0, 32, (150, 3))])
    built = B.build(cells, 5, np.where(cells[:, 1] < 14, 0x20E0A0, 0xD03060))
    model = M.simplify(built, built.size)[0]
    ball, ball_grid = trees7()["ball"]
    return {"ball": (ball, ball_grid, 7), "model5": (model, S.sample_dense(model, model.size, (0, 0, 0), (32,) * 3, 5), 5)}


def cases():
    """(name, source, op, offset, orient): every op against both sources at every offset, the orientations taken in turn"""
    out = []
    for source in ("ball", "model5"):
        for offset in OFFSETS:
            for op in X.OPS:
                orient = (11 * len(out) + 21) % 48
                out.append((f"{op}, {source} at {offset}, orient {orient}", source, op, offset, orient))
    return out


CASES = cases()
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def placed(name):
    """the restatement's (words, tallies) of a case on the base, computed once and shared with the GPU tests"""
    _, source, op, offset, orient = CASES[IDS.index(name)]
    a = trees7()["base"][0]
    b, _, src_depth = sources()[source]
    return P.place(a, a.size, b, op, 7, offset, orient, src_depth)


def case_named(op, source, offset):
    return next(c for c in CASES if c[1:4] == (source, op, offset))


@pytest.mark.parametrize("name,source,op,offset,orient", CASES, ids=IDS)
def test_the_rule_samples_to_the_per_cell_contract(name, source, op, offset, orient):
    a, grid_a = trees7()["base"]
    b, grid_b, src_depth = sources()[source]
    words, tally = placed(name)
    assert words.dtype == np.uint32 and words.size == a.size + 8 * tally["splits"] and np.array_equal(words[:8] >> 4, a[:8] >> 4)
    want = P.apply_cells(grid_a, grid_b, op, offset, orient)
    assert np.array_equal(grid7(words), want), name
    if any(o >= 128 or o + (1 << src_depth) <= 0 for o in offset):  # wholly outside: (200, 0, 0), and the model at x = -40
        assert np.array_equal(words, a) and tally["levels"] == [(8, 0)] and not any(tally[k] for k in X.TALLIES) and np.array_equal(want, grid_a)
    else:
        assert not np.array_equal(want, grid_a), name


def test_hit_counters_of_untouched_words_stay():
    a = trees7()["base"][0]
    b = sources()["ball"][0]
    rng = np.random.default_rng(31)
    counted = a | rng.integers(1, 16, a.size).astype(np.uint32)
    words, _ = P.place(counted, counted.size, b | np.uint32(5), "under", 7, (1, 1, 1), 9)
    plain = placed(case_named("under", "ball", (1, 1, 1))[0])
    again = P.place(a, a.size, b, "under", 7, (1, 1, 1), 9)[0]
    assert plain[0].size > a.size and again.size == words.size
    kept = words[: a.size] == counted
    assert kept.sum() > a.size // 2 and (~kept).sum() > 1000 and (words[: a.size][~kept] & 15 == 0).all() and (words[a.size:] & 15 == 0).all()
    assert np.array_equal(words >> 4, again >> 4)


def asymmetric_source():
    """the combine tests' depth-4 model: random voxels in two colours and a solid corner, which no symmetry maps to itself"""
    src = small_source()
    return src, S.sample_dense(src, src.size, (0, 0, 0), (16,) * 3, 4)


def test_all_48_orientations():
    src, gb = asymmetric_source()
    rng = np.random.default_rng(48)
    cells = rng.integers(0, 32, (400, 3))
    scene = B.build(cells, 5, rng.integers(1, 1 << 24, 400))
    ga = S.sample_dense(scene, scene.size, (0, 0, 0), (32,) * 3, 5)
    seen = set()
    for orient in range(48):
        words, tally = P.place(scene, scene.size, src, "replace", 5, (7, 9, 19), orient, 4)
        got = S.sample_dense(words, words.size, (0, 0, 0), (32,) * 3, 5)
        assert np.array_equal(got, P.apply_cells(ga, gb, "replace", (7, 9, 19), orient)), orient
        assert np.array_equal(got[7:23, 9:25, 19:32], P.orient_grid(gb, orient)[:, :, :13])
        seen.add(got.tobytes())
        # the oriented child index against the grid: the child of the oriented root that holds r holds q in the source
        perm, flips = P.unpack(orient)
        for r in ((0, 0, 0), (15, 0, 0), (0, 15, 0), (3, 9, 12)):
            q = [0, 0, 0]
            for i in range(3):
                q[perm[i]] = 15 - r[i] if flips[i] else r[i]
            assert P.orient_grid(gb, orient)[r] == gb[tuple(q)]
            assert P.child_map(orient)[S.child(*r, 3)] == S.child(*q, 3)
    assert len(seen) == 48
    assert np.array_equal(P.orient_grid(gb, 0), gb) and sorted(P.child_map(0).tolist()) == list(range(8))


@pytest.mark.parametrize("name,scene,source,op", cases7(), ids=[c[0] for c in cases7()])
def test_an_aligned_placement_gives_the_combines_words(name, scene, source, op):
    a, b = trees7()[scene][0], trees7()[source][0]
    want, tally = X.combine(a, a.size, b, op, 7)
    words, tally2 = P.place(a, a.size, b, op, 7)
    assert np.array_equal(words, want) and tally2 == tally, name


def test_a_source_placed_in_a_cell_of_level_3_gives_the_combines_words():
    src = small_source()
    masked = X.combine(trees7()["base"][0], 182304, trees7()["ball"][0], "keep", 7)[0]
    for scene, at, ops in ((trees7()["pasted"][0], (3, 3, 3), ("under", "over", "carve", "replace")), (masked, (1, 0, 1), ("over", "keep")),
                           (trees7()["base"][0], (3, 3, 3), ("over", "paint")), (EMPTY_ROOT, (5, 2, 7), X.OPS)):
        for op in ops:
            want, tally = X.combine(scene, scene.size, src, op, 7, 3, at)
            words, tally2 = P.place(scene, scene.size, src, op, 7, tuple(v << 4 for v in at), 0, 4)
            assert np.array_equal(words, want) and tally2 == tally, (at, op, tally, tally2)


@pytest.mark.parametrize("op", X.OPS)
def test_a_second_run_changes_nothing(op):
    for source in ("ball", "model5"):
        name, _, _, offset, orient = case_named(op, source, (1, 1, 1))
        b, _, src_depth = sources()[source]
        words = placed(name)[0]
        again, tally = P.place(words, words.size, b, op, 7, offset, orient, src_depth)
        assert np.array_equal(again, words) and tally["splits"] == tally["collapses"] == tally["overwrites"] == 0, name


def test_a_depth_3_case_by_hand():
    """The scene: one level-1 voxel A over the cells [0, 4)^3, with a hit counter.  The source: depth 1, the voxel Q in its cell
    (0, 0, 0) and P in (1, 1, 1), at offset (1, 1, 1): Q lands on the scene's cell (1, 1, 1), P on (2, 2, 2), and on no level
    but the last does a scene word face one source cell.  A faces the cell above the root and is split; its eight children, the
    cells [0, 2) and [2, 4) per axis, all straddle the source's cube and are split in turn, A carried down; the last level
    decides cell by cell.  The seven empty words of the root group lie beside the source's cube and are not looked into."""
    A, P_, Q, E = 0xA1B2C3, 0x00BEEF, 0x123456, B.EMPTY
    scene = np.array([leaf(A) | 5, E, E, E, E, E, E, E], dtype=np.uint32)
    source = np.array([leaf(Q) | 3, E, E, E, E, E, E, leaf(P_)], dtype=np.uint32)
    ga, gb = S.sample_dense(scene, 8, (0, 0, 0), (8,) * 3, 3), S.sample_dense(source, 8, (0, 0, 0), (2,) * 3, 1)

    def tree(at_q, at_p, inside, outside):
        """the root, A's group of eight pointers, and their groups: the scene cell (1,1,1) is child 7 of the first, (2,2,2)
        child 0 of the last; `inside`: the six other cells of the source's cube, `outside`: the cells around it"""
        words = [8 << 4, E, E, E, E, E, E, E] + [(16 + 8 * c) << 4 for c in range(8)]
        for c in range(8):
            for k in range(8):
                cell = tuple(2 * ((c >> s) & 1) + ((k >> s) & 1) for s in (2, 1, 0))
                words.append(at_q if cell == (1, 1, 1) else at_p if cell == (2, 2, 2) else inside if all(1 <= v <= 2 for v in cell) else outside)
        return np.array(words, dtype=np.uint32)

    want = {"over": tree(leaf(Q), leaf(P_), leaf(A), leaf(A)), "under": scene, "paint": tree(leaf(Q), leaf(P_), leaf(A), leaf(A)),
            "carve": tree(E, E, leaf(A), leaf(A)), "keep": tree(leaf(A), leaf(A), E, leaf(A)), "replace": tree(leaf(Q), leaf(P_), E, leaf(A))}
    # splits, collapses, overwrites, opened, carried
    tallies = {"over": (9, 0, 2, 0, 0), "under": (0, 0, 0, 0, 0), "paint": (9, 0, 2, 0, 0), "carve": (9, 0, 2, 0, 0), "keep": (9, 0, 6, 0, 0),
               "replace": (9, 0, 8, 0, 0)}
    for op in X.OPS:
        words, tally = P.place(scene, 8, source, op, 3, (1, 1, 1), 0, 1)
        assert np.array_equal(words, want[op]), (op, words.tolist(), want[op].tolist())
        assert tuple(tally[k] for k in X.TALLIES) == tallies[op], (op, tally)
        assert tally["levels"] == ([(8, 0)] if op == "under" else [(8, 1), (8, 8), (64, 0)]), (op, tally["levels"])
        assert np.array_equal(S.sample_dense(words, words.size, (0, 0, 0), (8,) * 3, 3), P.apply_cells(ga, gb, op, (1, 1, 1), 0)), op
    # a constant carried down: under an interior word, the source's one leaf over [0, 4)^3 is opened into and fills the empties
    scene = np.array([8 << 4, E, E, E, E, E, E, E] + [leaf(A), E, E, 16 << 4, E, E, E, E] + [E] * 7 + [leaf(A)], dtype=np.uint32)
    source = np.array([leaf(Q)] + [E] * 7, dtype=np.uint32)
    words, tally = P.place(scene, 24, source, "under", 3, (0, 0, 0), 0, 3)
    assert words.tolist() == [8 << 4, E, E, E, E, E, E, E] + [leaf(A), leaf(Q), leaf(Q), 16 << 4] + [leaf(Q)] * 4 + [leaf(Q)] * 7 + [leaf(A)]
    assert tuple(tally[k] for k in X.TALLIES) == (0, 0, 13, 2, 16)
    # ... and moved by two cells, the empty root word over x in [4, 8) faces two leaves of the source, Q and empty space: one split
    words, tally = P.place(scene, 24, source, "under", 3, (2, 0, 0), 0, 3)
    assert S.sample_dense(words, words.size, (0, 0, 0), (8,) * 3, 3)[:, 0, 0].tolist() == [A, A, Q, Q, Q, Q, 0, 0] and tally["splits"] == 1


def test_what_the_rule_refuses():
    a = trees7()["base"][0]
    ball = trees7()["ball"][0]
    # the scene and the source are finer than depth 5 where the ball's surface crosses the base
    with pytest.raises(X.Refused) as e:
        P.place(a, a.size, ball, "over", 5)
    with pytest.raises(X.Refused) as same:
        X.combine(a, a.size, ball, "over", 5)
    assert e.value.finer == "both" and e.value.cell == same.value.cell
    with pytest.raises(X.Refused) as e:
        P.place(a, a.size, ball, "over", 5, (1, 1, 1), 3)
    assert all(0 <= v < 32 for v in e.value.cell)
    # the source is finer than src_depth: its level-5 words are the cells of a depth-7 scene, and some are interior
    with pytest.raises(X.Refused) as e:
        P.place(EMPTY_ROOT, 8, ball, "over", 7, (1, 1, 1), 3, 5)
    assert e.value.finer == "source" and all(1 <= v < 33 for v in e.value.cell)
    with pytest.raises(X.Refused) as e:
        P.place(a, a.size, np.full(8, leaf(7), dtype=np.uint32), "paint", 5, (-3, 0, 2), 0, 5)
    assert e.value.finer == "scene"
    # not refused: where the op leaves the scene word untouched, or the source decides it as a whole, nothing below is looked at
    solid = np.full(8, leaf(0x102030), dtype=np.uint32)
    for op, scene in (("under", solid), ("paint", EMPTY_ROOT), ("carve", EMPTY_ROOT), ("keep", EMPTY_ROOT)):
        words, tally = P.place(scene, 8, ball, op, 1, (1, 0, -1), 7, 1)
        assert np.array_equal(words, scene) and not any(tally[k] for k in X.TALLIES), op
    words, tally = P.place(a, a.size, solid, "carve", 1, (0, 0, 0), 5, 1)
    assert tally["collapses"] == 8 and (words[:8] == B.EMPTY).all()
    # malformed sources: only the pointers that the call follows
    bad = ball.copy()
    first = int(np.flatnonzero(bad[:8] >> 4 < B.VOXEL_OFFSET)[0])
    bad[first] = (ball.size + 8) << 4
    with pytest.raises(X.Malformed) as e:
        P.place(EMPTY_ROOT, 8, bad, "over", 7, (1, 1, 1))
    assert e.value.which == "source" and "leaves the first src_words" in str(e.value)
    bad[first] = 12 << 4
    with pytest.raises(X.Malformed) as e:
        P.place(EMPTY_ROOT, 8, bad, "over", 7, (1, 1, 1))
    assert e.value.which == "source" and "not a multiple of 8" in str(e.value)
    assert np.array_equal(P.place(solid, 8, bad, "under", 7, (1, 1, 1))[0], solid)  # (never looked at)
    # the arguments, in the header's order: of two causes the earlier one is named
    for kw, text in (({"op": 6, "depth": 0}, "op must"), ({"depth": 0, "src_depth": 0}, "depth must be 1..21"), ({"depth": 22}, "depth must be 1..21"),
                     ({"src_depth": 0, "orient": 48}, "src_depth must"), ({"src_depth": 8, "orient": 48}, "src_depth must"),
                     ({"orient": 48, "offset": (1 << 22, 0, 0)}, "orient must"), ({"offset": (0, (1 << 21) + 1, 0)}, "offset must"),
                     ({"offset": (0, 0, -(1 << 21) - 1)}, "offset must")):
        args = {"op": 0, "depth": 7, "offset": (0, 0, 0), "orient": 0, "src_depth": 7, **kw}
        with pytest.raises(ValueError, match=text):
            P.place(a, a.size, ball, **args)
    for offset in ((1 << 21, 0, 0), (0, -(1 << 21), 5)):  # the ends of the range: wholly outside
        assert np.array_equal(P.place(a, a.size, ball, "replace", 7, offset)[0], a)
    with pytest.raises(ValueError):
        P.place(a, a.size, ball[:12], 0, 7)
    with pytest.raises(ValueError):
        P.place(a, 12, ball, 0, 7)


def test_the_tallies_show_what_the_combines_cases_cannot():
    """An unaligned paste splits the scene's coarse empty leaves along every leaf boundary of the source: a level whose frontier
    and whose splits both go beyond one scan tile, with a group count that fills no whole wave; every tally is shown."""
    tally = placed(case_named("over", "ball", (1, 1, 1))[0])[1]
    assert any(n > TILE and s > TILE and (n // 8) % 64 for n, s in tally["levels"]), tally["levels"]
    assert all(tally[k] > 0 for k in X.TALLIES), tally
    # more than one item per word on every level but the last: the frontier is wider than the aligned paste's
    aligned = X.combine(trees7()["base"][0], 182304, trees7()["ball"][0], "over", 7)[1]
    assert tally["splits"] > aligned["splits"] and len(tally["levels"]) == 7
    for op in X.OPS:
        total = dict.fromkeys(X.TALLIES, 0)
        for name, _, case_op, _, _ in CASES:
            if case_op == op:
                for key in X.TALLIES:
                    total[key] += placed(name)[1][key]
        for key in {"over": X.TALLIES, "under": ("splits", "overwrites", "opened", "carried"), "paint": ("overwrites", "opened", "carried"),
                    "carve": ("collapses", "overwrites", "opened"), "keep": ("collapses", "overwrites", "opened"), "replace": X.TALLIES}[op]:
            assert total[key] > 0, (op, key, total)


def test_the_parameter_record_has_the_headers_layout(pkg):
    R = pkg._lib.PlaceParams
    assert C.sizeof(R) == 56
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == [
        ("op", 0, 4), ("depth", 4, 4), ("src_depth", 8, 4), ("orient", 12, 4), ("offset", 16, 12), ("reserved", 28, 4), ("n_words", 32, 8),
        ("src_words", 40, 8), ("max_words", 48, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_place_params \{(.*?)\} svo_place_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|int32_t|uint64_t) (\w+)(?:\[3\])?;", body) == [
        ("uint32_t", "op"), ("uint32_t", "depth"), ("uint32_t", "src_depth"), ("uint32_t", "orient"), ("int32_t", "offset"), ("uint32_t", "reserved"),
        ("uint64_t", "n_words"), ("uint64_t", "src_words"), ("uint64_t", "max_words")]
    assert re.search(r"#define SVO_PLACE_ORIENTS 48u", header)
    assert re.search(r"#define SVO_PLACE_TIMES 5\b[^\n]*\nint svo_place_timing\(svo_ctx \*ctx, float ms_out\[SVO_PLACE_TIMES\]\);", header)
    assert "int svo_nodes_place(svo_ctx *ctx, const uint32_t *src_dev, const svo_place_params *p, uint64_t *n_words_out);" in header


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_place.argtypes) == 4 and len(lib.svo_place_timing.argtypes) == 2
    assert callable(pkg.Render.place_nodes) and callable(pkg.Gpu.place_timing)


def test_the_entry_points_appear_in_the_integration_guide():
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW + ("SvoPlaceParams",):
        assert name in text, name


def test_the_orientation_module_numbers_the_symmetries_as_the_header_does(pkg):
    T = pkg.orientation
    assert T.PERMS == P.PERMS and T.orientation() == 0
    _, gb = asymmetric_source()
    for orient in range(48):
        perm, flips = P.unpack(orient)
        assert T.orientation(perm, flips) == orient
        m = np.zeros((3, 3), dtype=np.int64)
        for i in range(3):
            m[i, perm[i]] = -1 if flips[i] else 1
        assert T.from_matrix(m) == orient and T.from_matrix(m.tolist()) == orient and round(np.linalg.det(m)) == (1 if T.is_rotation(orient) else -1)
        # about the cube's centre r - c = m (q - c), c = 7.5: the oriented grid holds at r what the source holds at q
        for q in ((0, 0, 0), (15, 3, 8), (4, 11, 2)):
            r = tuple(int(v) for v in np.rint(m @ (np.array(q) - 7.5) + 7.5))
            assert P.orient_grid(gb, orient)[r] == gb[q], (orient, q, r)
    assert sum(T.is_rotation(o) for o in range(48)) == 24
    # quarter turns about +y as stamp_structures counts them: (dx, dy, dz) -> (dz, dy, -dx)
    turn = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    assert T.quarter_turns_y(0) == T.quarter_turns_y(4) == 0 and T.quarter_turns_y(1) == T.orientation((2, 1, 0), (0, 0, 1)) == T.quarter_turns_y(-3)
    for k in range(4):
        assert T.quarter_turns_y(k) == T.from_matrix(np.linalg.matrix_power(turn, k)) and T.is_rotation(T.quarter_turns_y(k))
    assert len({T.quarter_turns_y(k) for k in range(4)}) == 4
    for bad in ([[1, 0, 0], [1, 0, 0], [0, 0, 1]], [[2, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 1, 0], [0, 1, 0], [0, 0, 1]], [[1, 0], [0, 1]]):
        with pytest.raises(ValueError):
            T.from_matrix(bad)
    with pytest.raises(ValueError):
        T.orientation((0, 0, 1))
    with pytest.raises(ValueError):
        T.is_rotation(48)
