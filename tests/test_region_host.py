"""A tree edited by shapes (csrc/svo_region.hip), CPU side: the rule's restatement (tests/region_ref.py: edit)
makes trees that sample (tests/sample_ref.py) to the per-cell contract (apply_cells), on the six depth-7 edits that the GPU
tests share and on a depth-4 case whose words are written out here; the integer classification of a ball against a cube
equals the enumeration of cell centres; a second application changes nothing; the shape record has the header's layout and
the entry points are exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import build_ref as B
import region_ref as R
import sample_ref as S
from conftest import ROOT as REPO
from pass_frame import tree7_base

NEW = ("svo_nodes_edit_region", "svo_region_timing")
# the tallies that a second, independent restatement of the rule counted when the pass was specified (and the new lengths)
TABLE = {
    "carve ball": {"collapses": 97, "splits": 0, "words": 182304},
    "fill ball": {"splits": 1215, "collapses": 97, "overwrites": 4849, "words": 192024},
    "paint box": {"splits": 0, "collapses": 0, "overwrites": 925, "opened": 2370},
    "flood box": {"splits": 4700, "overwrites": 57731, "words": 219904},
    "stroke": {},
    "whole grid": {"collapses": 8, "words": 182304},
}


def leaf(v):
    return (B.VOXEL_OFFSET + v) << 4


@pytest.fixture(scope="module")
def base7():
    base = tree7_base()["base"]
    assert base.size == 182304
    return base, S.sample_dense(base, base.size, (0, 0, 0), (128,) * 3, 7)


@pytest.mark.parametrize("name", list(TABLE))
def test_the_rule_samples_to_the_per_cell_contract(base7, name):
    base, grid = base7
    sh = R.shapes(R.table_cases()[name])
    words, tally = R.edit(base, base.size, sh, 7)
    assert words.dtype == np.uint32 and np.array_equal(words[:8] & 15, base[:8] & 15)
    assert words.size == base.size + 8 * tally["splits"]
    for key, want in TABLE[name].items():
        assert (words.size if key == "words" else tally[key]) == want, (name, key, tally)
    assert np.array_equal(S.sample_dense(words, words.size, (0, 0, 0), (128,) * 3, 7), R.apply_cells(grid, 7, sh)), name
    # idempotence: the same shapes on the result write nothing and append nothing
    again, tally2 = R.edit(words, words.size, sh, 7)
    assert np.array_equal(again, words) and tally2["splits"] == tally2["collapses"] == tally2["overwrites"] == 0


def test_the_order_of_the_shapes_matters(base7):
    base, grid = base7
    recs = R.table_cases()["stroke"]
    fwd, tally = R.edit(base, base.size, R.shapes(recs), 7)
    assert tally["splits"] > 0 and tally["collapses"] > 0
    back, _ = R.edit(base, base.size, R.shapes(recs[::-1]), 7)
    assert not np.array_equal(R.apply_cells(grid, 7, R.shapes(recs)), R.apply_cells(grid, 7, R.shapes(recs[::-1])))
    assert fwd.size != back.size or not np.array_equal(fwd, back)


def test_a_depth_4_case_by_hand():
    """One level-1 voxel A over the cells [0, 8)^3.  A carving box over [0, 4)^3 splits it and empties child 0 of the new
    group; a ball of EMPTY mode around the cell corner (13, 13, 13), radius 1 cell, is the level-3 cube [12, 14)^3: two
    splits on the way down the empty corner, then one leaf."""
    A, Bc, E = 0xA1B2C3, 0x00BEEF, B.EMPTY
    base = np.array([leaf(A) | 5] + [E] * 7, dtype=np.uint32)  # (the voxel carries a hit counter)
    sh = R.shapes([R.box((0, 0, 0), (4, 4, 4), 0), R.ball((26, 26, 26), 2, Bc, R.MODE_EMPTY)])
    want = np.array([8 << 4, E, E, E, E, E, E, 16 << 4,          # the root: both ends split, frontier order 0 then 7
                     E] + [leaf(A)] * 7 +                        # group 8: A carried down, counter 0; child 0 carved
                    [E] * 7 + [24 << 4] +                        # group 16: the empty corner's children; child 7 split
                    [leaf(Bc)] + [E] * 7, dtype=np.uint32)       # group 24: the ball is its child 0
    words, tally = R.edit(base, 8, sh, 4)
    assert np.array_equal(words, want), (words, want)
    assert (tally["splits"], tally["overwrites"], tally["collapses"], tally["opened"]) == (3, 2, 0, 0)
    grid = S.sample_dense(base, 8, (0, 0, 0), (16,) * 3, 4)
    cells = R.apply_cells(grid, 4, sh)
    assert np.array_equal(S.sample_dense(words, words.size, (0, 0, 0), (16,) * 3, 4), cells)
    assert (cells == Bc).sum() == 8 and (cells == A).sum() == 512 - 64 and (cells[12:14, 12:14, 12:14] == Bc).all()
    # a carving box over the whole of the split voxel collapses the interior word it became
    whole, t = R.edit(words, words.size, R.shapes([R.box((0, 0, 0), (8, 8, 8), 0)]), 4)
    assert t["collapses"] == 1 and whole[0] == E and whole.size == words.size
    # a painting box meets the interior word at depth 1: refused, naming the shape and the cell
    with pytest.raises(R.Refused) as e:
        R.edit(words, words.size, R.shapes([R.box((1, 1, 1), (2, 2, 2), 7, R.MODE_EMPTY), R.box((0, 0, 0), (1, 1, 1), 7, R.MODE_VOXELS)]), 1)
    assert (e.value.shape, e.value.cell) == (1, (0, 0, 0))


def test_ball_classes_equal_the_enumeration_of_cell_centres():
    rng = np.random.default_rng(25)
    seen = np.zeros(3, dtype=np.int64)
    for n in range(200):
        centre2 = rng.integers(0, 65, 3) if n % 4 else rng.integers(0, 33, 3) * 2  # odd and even; a quarter all even
        rec = R.ball(centre2.tolist(), int(rng.integers(0, 71)), 1)
        for level in range(1, 6):
            side = np.arange(1 << level)
            q = np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3)
            got = R.classify(rec, q, 5 - level)
            want = R.brute_class(rec, 5, level).reshape(-1)
            assert np.array_equal(got, want), (rec, level, int((got != want).sum()))
            if level == 5:
                assert (got != R.PART).all()
            seen += np.bincount(got, minlength=3)
    assert (seen >= 100).all(), seen
    # radius 0: an odd centre is exactly one cell, an even one none
    side = np.arange(32)
    q = np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3)
    one = R.classify(R.ball((7, 9, 63), 0, 1), q, 0)
    assert (one == R.FULL).sum() == 1 and q[one == R.FULL].tolist() == [[3, 4, 31]]
    assert (R.classify(R.ball((8, 9, 63), 0, 1), q, 0) == R.OUT).all()


def test_what_the_reference_refuses():
    root = np.full(8, B.EMPTY, dtype=np.uint32)
    ok = R.box((0, 0, 0), (1, 1, 1), 1)
    for depth in (0, 22):
        with pytest.raises(ValueError):
            R.edit(root, 8, R.shapes([ok]), depth)
    for bad in (R.box((1, 0, 0), (1, 1, 1), 1), R.box((0, 0, 0), (1, 17, 1), 1), R.ball((33, 0, 0), 1, 1), R.ball((0, 0, 0), (1 << 23) + 1, 1),
                [2 | 3 << 16, 0, 0, 0, 0, 1, 1, 1], [0 | 4 << 16, 0, 0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 0, 1, 1, 1]):
        with pytest.raises(ValueError):
            R.edit(root, 8, R.shapes([bad]), 4)
    with pytest.raises(ValueError):
        R.edit(root, 8, R.shapes([ok] * 1025), 4)
    with pytest.raises(ValueError):
        R.edit(root, 12, R.shapes([ok]), 4)
    words, tally = R.edit(root, 8, R.shapes([]), 4)
    assert np.array_equal(words, root) and not any(tally.values())


def test_the_shape_record_has_the_headers_layout(pkg):
    P = pkg._lib.RegionShape
    assert C.sizeof(P) == 32
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("kind", 0, 2), ("mode", 2, 2), ("colour", 4, 4), ("a", 8, 12), ("b", 20, 12)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_region_shape \{(.*?)\} svo_region_shape;", header, re.S).group(1)
    assert re.findall(r"(uint16_t|uint32_t) (\w+)(?:\[3\])?;", body) == [("uint16_t", "kind"), ("uint16_t", "mode"), ("uint32_t", "colour"),
                                                                        ("uint32_t", "a"), ("uint32_t", "b")]
    Q = pkg._lib.RegionParams
    assert C.sizeof(Q) == 24 and [(n, getattr(Q, n).offset) for n, _ in Q._fields_] == [("depth", 0), ("reserved", 4), ("n_words", 8), ("max_words", 16)]
    for name, value in (("BOX", 0), ("BALL", 1), ("EMPTY", 1), ("VOXELS", 2), ("SET", 3), ("MAX_SHAPES", 1024)):
        assert re.search(rf"#define SVO_REGION_{name}\s+{value}u", header) and getattr(pkg.region, name) == value
    assert re.search(r"#define SVO_REGION_TIMES 5\b[^\n]*\nint svo_region_timing\(svo_ctx \*ctx, float ms_out\[SVO_REGION_TIMES\]\);", header)


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_edit_region.argtypes) == 5 and len(lib.svo_region_timing.argtypes) == 2
    assert callable(pkg.Render.edit_region) and callable(pkg.Gpu.region_timing)
    assert "svo_nodes_edit_region" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_python_shapes_pack_to_the_record(pkg):
    G = pkg.region
    arr, n = G.pack([G.box((-3, 2, 5), (9, 40, 7), 0x1FFFFFF, G.VOXELS), G.box((40, 0, 0), (50, 1, 1), 1),
                     G.ball((3.5, 4, 0), 2.5, 9, G.EMPTY)], 5)
    assert n == 2  # (the second box lies outside the depth-5 grid: dropped)
    assert (arr[0].kind, arr[0].mode, arr[0].colour, list(arr[0].a), list(arr[0].b)) == (0, 2, 0xFFFFFF, [0, 2, 5], [9, 32, 7])
    assert (arr[1].kind, arr[1].mode, arr[1].colour, list(arr[1].a), list(arr[1].b)) == (1, 1, 9, [7, 8, 0], [5, 0, 0])
    for bad in (lambda: G.ball((0.25, 0, 0), 1, 1), lambda: G.ball((0, 0, 0), 1.3, 1), lambda: G.ball((0, 0, 0), -1, 1),
                lambda: G.box((0, 0, 0), (1.5, 1, 1), 1), lambda: G.box((0, 0), (1, 1, 1), 1), lambda: G.box((0, 0, 0), (1, 1, 1), 1, mode=0),
                lambda: G.ball((0, 0, 0), 1, 1, mode=4)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        G.pack([(0, 3, 1, (0, 0, 0), (1, 1, 1))], 5)
