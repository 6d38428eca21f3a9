"""A step of morphology on a tree (csrc/svo_morph.hip), CPU side: the rule's restatement (tests/morph_ref.py:
morph) makes trees that sample (tests/sample_ref.py) to the per-cell contract (cells: shifted copies of the grid) on all 256
depth-1 trees under every op, conn, boundary and colour rule, on the depth-7 base of the pass tests, on the merged ball with its
coarse leaves and on a seeded depth-5 tree of mixed levels; occupancy agrees with scipy's dilation, erosion, closing and opening;
a depth-3 case whose words are written out here; a single voxel in the middle of a depth-21 grid and one in a corner; repeated
steps; what is refused, in the header's order; the parameter record has the header's layout and the entry points are exported."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import build_ref as B
import morph_ref as R
import sample_ref as S
from combine_ref import Malformed
from conftest import ROOT as REPO
from test_combine_host import EMPTY_ROOT, leaf, trees7

NEW = ("svo_nodes_morph", "svo_morph_timing")
TILE = 4096  # items of one scan tile (csrc/svo_scan.h)
COLOUR = 0x30C8F0
# (op, conn, colour, open_boundary) of the big trees' cases: every op with every conn, both colour rules, both boundaries
VARIANTS = (("grow", 6, 0, False), ("grow", 18, COLOUR, False), ("grow", 26, 0, False), ("shrink", 6, 0, True), ("shrink", 18, 0, False),
            ("shrink", 26, 0, True))


def grid_of(words, depth):
    return S.sample_dense(words, words.size, (0, 0, 0), (1 << depth,) * 3, depth)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (words, their whole grid, depth).  "base": the depth-7 scene of the pass tests, every voxel a cell of the deepest
    level; "ball": the combine's merged two-coloured ball, coarse leaves of both colours and of empty space; "mixed5": a seeded
    depth-5 tree, a two-coloured solid box (coarse leaves once merged) that touches the wall x = 0, with 300 voxels of random
    colours around and inside it.  Computed once per session; nobody writes to the arrays."""
    import simplify_ref as M
    rng = np.random.default_rng(31)
    box = S.box_cells((0, 6, 9), (12, 16, 14))
    loose = rng.integers(0, 32, (300, 3))
    cells = np.concatenate([box, loose])
    built = B.build(cells, 5, np.concatenate([np.where(box[:, 2] < 16, 0x8040C0, 0x40C080), rng.integers(1, 1 << 24, 300)]))
    mixed = M.simplify(built, built.size)[0]
    t = trees7()
    return {"base": (t["base"][0], t["base"][1], 7), "ball": (t["ball"][0], t["ball"][1], 7), "mixed5": (mixed, grid_of(mixed, 5), 5)}


CASES = [(f"{scene}: {op} {conn}{', coloured' if colour else ''}{', open' if open_b else ''}", scene, op, conn, colour, open_b)
         for scene in ("base", "ball", "mixed5") for op, conn, colour, open_b in VARIANTS if scene != "base" or (op, conn) in (("grow", 6), ("shrink", 6))]
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def morphed(name):
    """the restatement's (words, tallies) of a case, computed once and shared with the GPU tests"""
    _, scene, op, conn, colour, open_b = CASES[IDS.index(name)]
    words, _, depth = scenes()[scene]
    return R.morph(words, words.size, op, conn, depth, colour, open_b)


@pytest.mark.parametrize("name,scene,op,conn,colour,open_b", CASES, ids=IDS)
def test_the_rule_samples_to_the_per_cell_contract(name, scene, op, conn, colour, open_b):
    a, grid, depth = scenes()[scene]
    words, tally = morphed(name)
    assert words.dtype == np.uint32 and words.size == a.size + 8 * tally["splits"] and tally["refusals"] == 0
    want = R.cells(grid, op, conn, colour, open_b)
    assert np.array_equal(grid_of(words, depth), want), name
    assert not np.array_equal(want, grid) and tally["overwrites"] > 0 and tally["opened"] == int((a >> 4 < B.VOXEL_OFFSET).sum()), (name, tally)
    # what the op cannot change keeps all 32 bits; a grow adds, a shrink removes, and nothing else changes
    if op == "grow":
        assert np.array_equal(want[grid != 0], grid[grid != 0]) and (want != 0).sum() > (grid != 0).sum()
        assert colour == 0 or set(np.unique(want[grid == 0]).tolist()) == {0, colour}
    else:
        assert np.array_equal(want[want != 0], grid[want != 0]) and (want != 0).sum() < (grid != 0).sum()


@pytest.mark.parametrize("op", R.OPS)
def test_all_256_trees_of_depth_1(op):
    """every occupancy of a root group, each child a colour of its own, so that an inherited colour names its neighbour"""
    for pattern in range(256):
        words = np.array([leaf(0x101010 * (c + 1)) if pattern >> c & 1 else B.EMPTY for c in range(8)], dtype=np.uint32)
        grid = grid_of(words, 1)
        for conn in (6, 18, 26):
            for open_b in (False, True):
                for colour in ((0, COLOUR) if op == "grow" else (0,)):
                    got, tally = R.morph(words, 8, op, conn, 1, colour, open_b)
                    want = R.cells(grid, op, conn, colour, open_b)
                    assert got.size == 8 and np.array_equal(grid_of(got, 1), want), (pattern, conn, open_b, colour)
                    assert tally["overwrites"] == int((want != grid).sum()) and tally["splits"] == tally["opened"] == 0
    full = np.array([leaf(c + 1) for c in range(8)], dtype=np.uint32)
    assert np.array_equal(R.morph(full, 8, op, 26, 1)[0], full)
    assert np.array_equal(R.morph(EMPTY_ROOT, 8, op, 26, 1, 0, True)[0], EMPTY_ROOT)
    if op == "shrink":
        assert np.array_equal(R.morph(full, 8, op, 6, 1, 0, True)[0], EMPTY_ROOT)
    else:  # the first neighbour by priority: of cell (0, 0, 0) with everything else set, the face neighbour -x < +x ... (0, 0, 1) before (0, 1, 0)
        one_hole = full.copy()
        one_hole[0] = B.EMPTY
        assert R.morph(one_hole, 8, op, 26, 1)[0][0] == leaf(2) and R.cells(grid_of(one_hole, 1), op, 26)[0, 0, 0] == 2


@pytest.mark.parametrize("scene", ("ball", "mixed5"))
def test_occupancy_agrees_with_scipy(scene):
    _, grid, _ = scenes()[scene]
    occ = grid != 0
    for k, conn in ((1, 6), (2, 18), (3, 26)):
        shape = ndimage.generate_binary_structure(3, k)
        assert shape.sum() == conn + 1
        assert np.array_equal(R.cells(grid, "grow", conn) != 0, ndimage.binary_dilation(occ, shape, border_value=0))
        assert np.array_equal(R.cells(grid, "grow", conn, COLOUR, True) != 0, ndimage.binary_dilation(occ, shape, border_value=0))
        assert np.array_equal(R.cells(grid, "shrink", conn) != 0, ndimage.binary_erosion(occ, shape, border_value=1))
        assert np.array_equal(R.cells(grid, "shrink", conn, 0, True) != 0, ndimage.binary_erosion(occ, shape, border_value=0))
    for name, _, op, conn, _, open_b in (c for c in CASES if c[1] == scene):
        shape = ndimage.generate_binary_structure(3, R.REACH[conn])
        want = ndimage.binary_dilation(occ, shape) if op == "grow" else ndimage.binary_erosion(occ, shape, border_value=0 if open_b else 1)
        assert np.array_equal(grid_of(morphed(name)[0], scenes()[scene][2]) != 0, want), name


def test_a_depth_3_case_by_hand():
    """Shrink, conn 6, closed boundary.  The scene: the level-1 voxel A over the cells [0, 4)^3, with a hit counter, beside the
    interior word of the octant x in [4, 8), y, z in [0, 4), whose group at 8 holds the level-2 voxel Q over x in [4, 6), y, z in [0, 2)
    and seven empty words.  A faces the interior word at +x (and empty leaves at +y, +z) and is split into the group 16, A
    carried down; the interior word is opened.  Of A's eight children (0, 0, 0) sees only A, the wall and, a level-2 cell, nothing
    else; (1, 0, 0) sees Q at +x, the constant of a leaf of its own level: both stay whole.  The other six see an empty word of
    level 1 carried down, or an empty word of the group at 8, and are split in child order into the groups 24 .. 64; Q has the
    empty word (3, 0, 0) of its own group at +x and is split into 72.  The last level decides cell by cell: of A, a cell stays
    when y <= 2, z <= 2 and x <= 2, or x == 3 with Q behind it (y, z < 2); of Q only (4, 0, 0) stays."""
    A, Q, E = 0xA1B2C3, 0x123456, B.EMPTY
    scene = np.array([leaf(A) | 5, E, E, E, (8 << 4) | 3, E, E, E] + [leaf(Q) | 9, E, E, E, E, E, E, E], dtype=np.uint32)

    def cell_word(x, y, z):
        if x < 4:
            return leaf(A) if y <= 2 and z <= 2 and (x <= 2 or (y < 2 and z < 2)) else E
        return leaf(Q) if (x, y, z) == (4, 0, 0) else E

    def group(x2, y2, z2):
        """the eight level-3 words of the level-2 cell (x2, y2, z2)"""
        return [cell_word(2 * x2 + (k >> 2), 2 * y2 + (k >> 1 & 1), 2 * z2 + (k & 1)) for k in range(8)]

    want = [16 << 4, E, E, E, (8 << 4) | 3, E, E, E] + [72 << 4, E, E, E, E, E, E, E]
    want += [leaf(A), 24 << 4, 32 << 4, 40 << 4, leaf(A), 48 << 4, 56 << 4, 64 << 4]
    for c in (1, 2, 3, 5, 6, 7):
        want += group(c >> 2, c >> 1 & 1, c & 1)
    want += group(2, 0, 0)
    words, tally = R.morph(scene, 16, "shrink", 6, 3)
    assert words.tolist() == want, (words.tolist(), want)
    assert {k: tally[k] for k in R.TALLIES} == {"splits": 8, "overwrites": 40, "opened": 1, "refusals": 0}
    assert tally["levels"] == [(8, 1), (16, 7), (56, 0)]
    assert np.array_equal(grid_of(words, 3), R.cells(grid_of(scene, 3), "shrink", 6))
    # under an open boundary the two children that stayed whole face the wall and are split too
    words, tally = R.morph(scene, 16, "shrink", 6, 3, 0, True)
    assert tally["levels"] == [(8, 1), (16, 9), (72, 0)] and np.array_equal(grid_of(words, 3), R.cells(grid_of(scene, 3), "shrink", 6, 0, True))
    # at depth 1 the same call is refused: the word A, a leaf at the last level then, would be changed by an interior neighbour
    with pytest.raises(R.Refused) as e:
        R.morph(scene[:16], 16, "shrink", 6, 1)
    assert e.value.cell == (0, 0, 0) and e.value.count == 2  # (A, and the interior word itself)


def test_a_single_voxel_in_the_middle_of_a_depth_21_grid():
    """(2^20, 2^20, 2^20) is the first cell of the last octant: its 26 neighbours lie in all eight.  At level 1 the seven empty
    octants face the interior one and are split.  At every level l in 2 .. 20 the path's cell (2^(l-1),)*3 is child 0 of its group: its
    26 neighbours of that level, the 7 real empty siblings and 19 virtual children of the level above's splits, are empty leaves
    that face an interior word and are split, and nothing else is: 7 + 19 * 26 = 501 splits.  The frontier is the 8 root words,
    then the 8 groups of level 1's words, then the path's group and the 26 splits' at every level.  The last level writes the 26 cells."""
    mid = 1 << 20
    V = 0x00C0FFEE
    scene = B.build(np.array([[mid, mid, mid]]), 21, np.array([V]))
    assert scene.size == 8 * 21
    words, tally = R.morph(scene, scene.size, "grow", 26, 21)
    assert {k: tally[k] for k in R.TALLIES} == {"splits": 501, "overwrites": 26, "opened": 20, "refusals": 0}
    assert tally["levels"] == [(8, 7), (64, 26)] + [(216, 26)] * 18 + [(216, 0)] and words.size == 168 + 8 * 501 == 4176
    around = S.box_cells((mid - 2,) * 3, (5, 5, 5))
    got = S.sample(words, words.size, around, 21)[0].reshape(5, 5, 5)
    want = np.zeros((5, 5, 5), dtype=np.uint32)
    want[1:4, 1:4, 1:4] = V
    assert np.array_equal(got, want)
    octants = {tuple((around[i] >> 20).tolist()) for i in np.flatnonzero(got.reshape(-1))}
    assert len(octants) == 8
    # conn 6: the six face neighbours, in four octants; only the faces' chains are split: 3 at level 1, then 6 per level
    words, tally = R.morph(scene, scene.size, "grow", 6, 21, COLOUR)
    got = S.sample(words, words.size, around, 21)[0].reshape(5, 5, 5)
    assert (got != 0).sum() == 7 and got[2, 2, 2] == V and got[1, 2, 2] == got[3, 2, 2] == got[2, 2, 1] == COLOUR
    assert tally["splits"] == 3 + 6 * 19 and tally["overwrites"] == 6
    # a shrink removes the voxel and splits nothing: it is a cell of the last level
    words, tally = R.morph(scene, scene.size, "shrink", 26, 21)
    assert words.size == scene.size and tally["overwrites"] == 1 and (words != scene).sum() == 1


def test_a_voxel_in_the_corner_and_a_full_grid():
    corner = B.build(np.array([[0, 0, 0]]), 3, np.array([7]))
    words, tally = R.morph(corner, corner.size, "grow", 26, 3)
    grid = grid_of(words, 3)
    assert (grid != 0).sum() == 8 and (grid[:2, :2, :2] == 7).all() and tally["overwrites"] == 7
    assert tally["levels"] == [(8, 7), (64, 7), (64, 0)]  # (the empty leaves beside the voxel's path, split level by level)
    far = B.build(np.array([[7, 7, 7]]), 3, np.array([9]))
    assert (grid_of(R.morph(far, far.size, "grow", 18, 3)[0], 3) != 0).sum() == 7  # (the corner cell (6, 6, 6) is no neighbour under 18)
    # the outside is neutral: a full grid stays one group of eight leaves under a closed boundary, whatever the depth
    full = np.full(8, leaf(0x445566), dtype=np.uint32) | np.arange(8, dtype=np.uint32)
    for conn in (6, 18, 26):
        words, tally = R.morph(full, 8, "shrink", conn, 4)
        assert np.array_equal(words, full) and not any(tally[k] for k in R.TALLIES) and tally["levels"] == [(8, 0)]
        words, tally = R.morph(full, 8, "grow", conn, 4, COLOUR, True)
        assert np.array_equal(words, full) and tally["levels"] == [(8, 0)]
    # ... and an open one peels one layer of cells off it
    words, tally = R.morph(full, 8, "shrink", 6, 4, 0, True)
    grid = grid_of(words, 4)
    assert (grid[1:15, 1:15, 1:15] == 0x445566).all() and (grid != 0).sum() == 14 ** 3
    assert tally["levels"] == [(8, 8), (64, 56), (448, 8 ** 3 - 6 ** 3), (8 * 296, 0)]  # (the cells on the wall, level by level)


def test_repeated_steps():
    words, grid, depth = scenes()["mixed5"]
    for op, conn, colour, open_b in (("grow", 18, 0, False), ("shrink", 6, 0, True)):
        w, g = words, grid
        for _ in range(3):
            w = R.morph(w, w.size, op, conn, depth, colour, open_b)[0]
            g = R.cells(g, op, conn, colour, open_b)
        assert np.array_equal(grid_of(w, depth), g) and np.array_equal(g, R.steps(grid, op, 3, conn, colour, open_b))
    # three grows under 6, 18 and 26 are the octahedron, the 18-cell shape's third power and the cube of radius 3
    one = B.build(np.array([[8, 7, 9]]), 4, np.array([5]))
    d = np.abs(S.box_cells((0, 0, 0), (16, 16, 16)) - (8, 7, 9)).reshape(16, 16, 16, 3)
    w = one
    for _ in range(3):
        w = R.morph(w, w.size, "grow", 6, 4)[0]
    assert np.array_equal(grid_of(w, 4) != 0, d.sum(axis=-1) <= 3) and (grid_of(w, 4) != 0).sum() == 63
    assert np.array_equal(R.steps(grid_of(one, 4), "grow", 3, 26) != 0, d.max(axis=-1) <= 3)
    ball18 = ndimage.binary_dilation(grid_of(one, 4) != 0, ndimage.generate_binary_structure(3, 2), iterations=3)
    assert np.array_equal(R.steps(grid_of(one, 4), "grow", 3, 18) != 0, ball18)


def test_close_and_open_against_scipy():
    """a tree whose voxels stay three cells off the walls, so that two grows never reach the wall and scipy's border value
    (one for both halves of a closing) never shows"""
    rng = np.random.default_rng(8)
    cells = np.concatenate([3 + rng.integers(0, 26, (900, 3)), S.box_cells((8, 9, 10), (9, 7, 8))])
    tree = B.build(cells, 5, rng.integers(1, 1 << 24, len(cells)))
    grid = grid_of(tree, 5)
    occ = grid != 0
    for k, conn in ((1, 6), (2, 18), (3, 26)):
        shape = ndimage.generate_binary_structure(3, k)
        for n in (1, 2):
            closed = R.steps(grid, "close", n, conn)
            opened = R.steps(grid, "open", n, conn)
            assert np.array_equal(closed != 0, ndimage.binary_closing(occ, shape, iterations=n)), (conn, n)
            assert np.array_equal(opened != 0, ndimage.binary_opening(occ, shape, iterations=n)), (conn, n)
            assert (closed != 0).sum() > occ.sum() > (opened != 0).sum()
    # the words' route: two grows and two shrinks of the tree
    w = tree
    for op in ("grow", "grow", "shrink", "shrink"):
        w = R.morph(w, w.size, op, 18, 5)[0]
    assert np.array_equal(grid_of(w, 5), R.steps(grid, "close", 2, 18))


def test_what_the_rule_refuses():
    a = scenes()["base"][0]
    # the arguments, in the header's order: of two causes the earlier one is named
    for kw, text in (({"op": 2, "conn": 7}, "op must"), ({"conn": 7, "depth": 0}, "conn must"), ({"conn": 0}, "conn must"), ({"depth": 0, "flags": 2}, "depth must"),
                     ({"depth": 22}, "depth must"), ({"flags": 2, "op": 1, "colour": 5}, "unknown flag"), ({"op": 1, "colour": 5}, "colour must be 0")):
        args = {"op": 0, "conn": 26, "depth": 7, "colour": 0, "flags": 0, **kw}
        with pytest.raises(ValueError, match=text):
            R.check_params(**args)
    with pytest.raises(ValueError, match="colour must be 0"):
        R.morph(a, a.size, "shrink", 6, 7, 5)
    with pytest.raises(ValueError):
        R.morph(a, 12, "grow", 6, 7)
    with pytest.raises(ValueError):
        R.morph(a, a.size + 8, "grow", 6, 7)
    # a tree finer than depth: the first interior word of level 5, whatever the op, and nothing is written
    for op in R.OPS:
        with pytest.raises(R.Refused) as e:
            R.morph(a, a.size, op, 26, 5)
        assert all(0 <= v < 32 for v in e.value.cell) and e.value.count > 1000
    # malformed trees: every pointer, also one that no changed cell is near
    bad = a.copy()
    first = int(np.flatnonzero(bad[:8] >> 4 < B.VOXEL_OFFSET)[0])
    bad[first] = (a.size + 8) << 4
    with pytest.raises(Malformed, match="leaves the first n_words"):
        R.morph(bad, bad.size, "grow", 6, 7)
    bad[first] = 12 << 4
    with pytest.raises(Malformed, match="level 1 is not a multiple of 8"):
        R.morph(bad, bad.size, "shrink", 6, 7)
    bad[first] = a[(first + 1) % 8] if a[(first + 1) % 8] >> 4 < B.VOXEL_OFFSET else 0
    with pytest.raises(Malformed, match="reached twice"):
        R.morph(bad, bad.size, "grow", 26, 7)


def test_the_tallies_show_a_level_beyond_one_scan_tile():
    """the ball at depth 7, grown under 26: level 6 has 46 400 frontier words of which 12 608 are split -- both beyond one scan
    tile of 4 096 --, in 5 800 groups, which fill no whole wave; the last level's frontier holds 147 776 words.  Every case pins
    its tallies."""
    tally = morphed("ball: grow 26")[1]
    assert tally["levels"] == [(8, 0), (64, 8), (512, 272), (3584, 1064), (13952, 3512), (46400, 12608), (147776, 0)], tally["levels"]
    assert any(n > TILE and s > TILE and (n // 8) % 64 for n, s in tally["levels"])
    # splits, overwrites, opened
    want = {"base: grow 6": (71427, 58406, 22787), "base: shrink 6, open": (0, 9974, 22787),
            "ball: grow 6": (9544, 26472, 9072), "ball: grow 18, coloured": (15168, 41528, 9072), "ball: grow 26": (17464, 48368, 9072),
            "ball: shrink 6, open": (7832, 25776, 9072), "ball: shrink 18": (11896, 39632, 9072), "ball: shrink 26, open": (13808, 45968, 9072),
            "mixed5: grow 6": (1545, 2411, 703), "mixed5: grow 18, coloured": (2706, 5142, 703), "mixed5: grow 26": (3049, 6692, 703),
            "mixed5: shrink 6, open": (237, 1273, 703), "mixed5: shrink 18": (256, 1110, 703), "mixed5: shrink 26, open": (269, 1278, 703)}
    assert sorted(want) == sorted(IDS)
    for name in IDS:
        t = morphed(name)[1]
        assert (t["splits"], t["overwrites"], t["opened"], t["refusals"]) == want[name] + (0,), (name, t)


def test_the_parameter_record_has_the_headers_layout(pkg):
    P = pkg._lib.MorphParams
    assert C.sizeof(P) == 40
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("op", 0, 4), ("conn", 4, 4), ("depth", 8, 4), ("flags", 12, 4), ("colour", 16, 4), ("reserved", 20, 4), ("n_words", 24, 8), ("max_words", 32, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_morph_params \{(.*?)\} svo_morph_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [
        ("uint32_t", "op"), ("uint32_t", "conn"), ("uint32_t", "depth"), ("uint32_t", "flags"), ("uint32_t", "colour"), ("uint32_t", "reserved"),
        ("uint64_t", "n_words"), ("uint64_t", "max_words")]
    for line in ("#define SVO_MORPH_GROW   0u", "#define SVO_MORPH_SHRINK 1u", "#define SVO_MORPH_OPEN_BOUNDARY 1u"):
        assert line in header
    assert re.search(r"#define SVO_MORPH_TIMES 5\b[^\n]*\nint svo_morph_timing\(svo_ctx \*ctx, float ms_out\[SVO_MORPH_TIMES\]\);", header)
    assert "int svo_nodes_morph(svo_ctx *ctx, const svo_morph_params *p, uint64_t *n_words_out);" in header


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_morph.argtypes) == 3 and len(lib.svo_morph_timing.argtypes) == 2
    assert callable(pkg.Render.morph_nodes) and callable(pkg.Render.shell_nodes) and callable(pkg.Gpu.morph_timing)
    assert pkg.render.MORPH_OPS == ("grow", "shrink", "close", "open") and pkg.MORPH_OPS is pkg.render.MORPH_OPS


def test_the_entry_points_appear_in_the_integration_guide():
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW + ("SvoMorphParams",):
        assert name in text, name
