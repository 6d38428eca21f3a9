"""A tree shaped by a height map (csrc/svo_heightmap.hip), CPU side: the rule's restatement
(tests/heightmap_ref.py: edit) makes trees that sample (tests/sample_ref.py) to the per-cell contract (apply_cells) on the
depth-7 cases that the GPU tests share and on a depth-3 case whose words are written out here; a second application changes
nothing; the pyramid equals a brute force over the tiles' columns; the records have the header's layout and the entry points
are exported.  The library's argument checks need a context, which needs a device: they are in test_heightmap_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import build_ref as B
import heightmap_ref as H
import sample_ref as S
from conftest import ROOT as REPO
from pass_frame import tree7_base

NEW = ("svo_nodes_edit_heightmap", "svo_heightmap_minmax", "svo_heightmap_timing")
ROOT = np.full(8, B.EMPTY, dtype=np.uint32)
# the tallies that a case is listed for: each must be non-zero, so the case proves that it happened
SHOWS = {"terraform": ("splits", "collapses", "overwrites", "opened"), "raise only": ("splits", "overwrites"), "lower only": ("collapses",),
         "repaint": ("overwrites", "opened"), "rectangle": ("splits", "collapses", "overwrites", "untouched"), "one column": ("splits", "overwrites"),
         "row": ("splits", "overwrites"), "empty root": ("splits", "overwrites"), "flat": ("overwrites",), "eight layers": ("splits", "collapses")}


def leaf(v):
    return (B.VOXEL_OFFSET + v) << 4


@pytest.fixture(scope="module")
def bases():
    base = tree7_base()["base"]
    return {"base7": (base, S.sample_dense(base, base.size, (0, 0, 0), (128,) * 3, 7)), "root": (ROOT, np.zeros((128,) * 3, dtype=np.uint32))}


@pytest.mark.parametrize("name", list(SHOWS))
def test_the_rule_samples_to_the_per_cell_contract(bases, name):
    which, heights, origin, p = H.table_cases()[name]
    base, grid = bases[which]
    words, tally = H.edit(base, base.size, heights, origin, 7, p)
    assert words.dtype == np.uint32 and words.size == base.size + 8 * tally["splits"]
    for key in SHOWS[name]:
        assert tally[key] > 0, (name, key, tally)
    assert np.array_equal(S.sample_dense(words, words.size, (0, 0, 0), (128,) * 3, 7), H.apply_cells(grid, 7, heights, origin, p)), name
    # idempotence: the same map on the result writes nothing and appends nothing
    again, tally2 = H.edit(words, words.size, heights, origin, 7, p)
    assert np.array_equal(again, words) and tally2["splits"] == tally2["collapses"] == tally2["overwrites"] == 0
    if name == "terraform":
        assert max(tally["level_splits"]) > 4096  # (a level's frontier and its splits go beyond one scan tile)
    if name in ("lower only", "repaint"):
        assert tally["splits"] == 0 and words.size == base.size
    if name == "flat":  # four leaf words of level 1, nothing appended
        assert words.size == 8 and tally["overwrites"] == 4 and tally["splits"] == 0
        assert words.tolist() == [leaf(0xFFFFFF) if not c & 2 else B.EMPTY for c in range(8)]


def test_a_depth_3_case_by_hand():
    """One level-1 voxel A over the cells [0, 4)^3 of an 8^3 grid, and a map over the columns x in [0, 4), z in [0, 2): height
    2 everywhere but 3 in the column (1, 1); one layer of colour G, below SET, above SET carving.  The voxel's footprint
    leaves the map, so it is split; of its children, the four with z in [2, 4) are outside the map and stay A; the children
    (0, 0, 0) and (1, 0, 0), y in [0, 2), lie wholly below the lowest ground and become G; of the children y in [2, 4) over
    the map, (0, 1, 0) has height 3 in one column: split, its cell (1, 2, 1) becomes G and its other cells are carved;
    (1, 1, 0) lies wholly above and is carved."""
    A, G, E = 0xA1B2C3, 0x00BEEF, B.EMPTY
    base = np.array([leaf(A) | 5] + [E] * 7, dtype=np.uint32)  # (the voxel carries a hit counter)
    heights = np.array([[2, 2], [2, 3], [2, 2], [2, 2]])
    p = H.params([(0, G)], "set", "set", 0)
    words, tally = H.edit(base, 8, heights, (0, 0), 3, p)
    assert words[0] == 8 << 4 and (words[1:8] == E).all()
    # group 8, the voxel's children by index x << 2 | y << 1 | z: z = 1 untouched, (0,0,0) and (1,0,0) G, (0,1,0) split, (1,1,0) empty
    assert words[8:16].tolist() == [leaf(G), leaf(A), 16 << 4, leaf(A), leaf(G), leaf(A), E, leaf(A)]
    assert words[16:24].tolist() == [E, E, E, E, E, leaf(G), E, E]  # x, z in [0, 2), y in [2, 4): the cell (1, 2, 1) alone
    assert words.size == 24 and (tally["splits"], tally["overwrites"], tally["collapses"], tally["opened"]) == (2, 11, 0, 0)
    grid = S.sample_dense(base, 8, (0, 0, 0), (8,) * 3, 3)
    cells = H.apply_cells(grid, 3, heights, (0, 0), p)
    assert np.array_equal(S.sample_dense(words, words.size, (0, 0, 0), (8,) * 3, 3), cells)
    assert (cells == G).sum() == 17 and (cells == A).sum() == 64 - 32
    # the same map one level up meets the interior word under "empty": refused, naming the cell; "set" collapses it
    with pytest.raises(H.Refused) as e:
        H.edit(words, words.size, np.array([[1]]), (0, 0), 1, H.params([(0, G)], "empty", None))
    assert e.value.cell == (0, 0, 0)
    whole, t = H.edit(words, words.size, np.array([[1]]), (0, 0), 1, H.params([(0, G)], "set", "set", 0))
    assert t["collapses"] == 1 and whole[0] == leaf(G) and whole.size == words.size


def test_layers_and_their_64_bit_sums():
    grid = np.zeros((16,) * 3, dtype=np.uint32)
    heights = np.full((16, 16), 12)
    layers = [(2, 1), (0, 2), (3, 0), (0xFFFFFFFF, 4), (0xFFFFFFFF, 5), (1, 6)]
    cells = H.apply_cells(grid, 4, heights, (0, 0), H.params(layers))
    column = cells[3, :, 5].tolist()
    assert column == [4] * 7 + [0] * 3 + [1] * 2 + [0] * 4  # the band of thickness 0 holds no cell; nothing reaches the layers 5 and 6
    words, tally = H.edit(np.full(8, B.EMPTY, dtype=np.uint32), 8, heights, (0, 0), 4, H.params(layers))
    assert np.array_equal(S.sample_dense(words, words.size, (0, 0, 0), (16,) * 3, 4), cells)
    # heights above the grid, 0xFFFFFFFF included, are clamped
    tall = H.apply_cells(grid, 4, np.array([[0xFFFFFFFF, 17], [16, 0]], dtype=np.uint64), (2, 2), H.params([(0, 9)]))
    assert (tall[2, :, 2] == 9).all() and (tall[2, :, 3] == 9).all() and (tall[3, :, 2] == 9).all() and (tall[3, :, 3] == 0).all()
    assert (tall != 0).sum() == 48


def brute_pyramid(heights, origin, depth, s):
    h = np.minimum(np.asarray(heights).astype(np.uint64), 1 << depth)
    (ox, oz), (sx, sz) = origin, h.shape
    t0 = [ox >> s, oz >> s]
    n = [((ox + sx - 1) >> s) - t0[0] + 1, ((oz + sz - 1) >> s) - t0[1] + 1]
    out = np.zeros(n + [2], dtype=np.uint32)
    for i in range(n[0]):
        for k in range(n[1]):
            xs = [x for x in range(max((t0[0] + i) << s, ox), min((t0[0] + i + 1) << s, ox + sx))]
            zs = [z for z in range(max((t0[1] + k) << s, oz), min((t0[1] + k + 1) << s, oz + sz))]
            tile = h[np.array(xs)[:, None] - ox, np.array(zs)[None, :] - oz]
            out[i, k] = tile.min(), tile.max()
    return out


def test_the_pyramid_equals_a_brute_force():
    rng = np.random.default_rng(32)
    for (sx, sz), origin, depth in (((67, 50), (5, 9), 7), ((1, 33), (127, 40), 7), ((40, 1), (3, 0), 6), ((1, 1), (63, 63), 6), ((3, 5), (2**21 - 3, 2**21 - 5), 21)):
        heights = rng.integers(0, (1 << min(depth, 8)) + 13, (sx, sz))
        for s in range(0, depth + 1):
            got = H.pyramid(heights, origin, depth, s)
            assert np.array_equal(got, brute_pyramid(heights, origin, depth, s)), ((sx, sz), origin, s)
        assert H.pyramid(heights, origin, depth, depth).shape == (1, 1, 2)
        assert got[0, 0].tolist() == [min(heights.min(), 1 << depth), min(heights.max(), 1 << depth)]


def test_what_the_reference_refuses():
    ok = np.ones((2, 2), dtype=np.int64)
    for depth in (0, 22):
        with pytest.raises(ValueError):
            H.edit(ROOT, 8, ok, (0, 0), depth, H.params())
    for origin in ((15, 0), (0, 15), (-1, 0)):
        with pytest.raises(ValueError):
            H.edit(ROOT, 8, ok, origin, 4, H.params())
    with pytest.raises(ValueError):
        H.edit(ROOT, 8, ok, (0, 0), 4, H.params([(1, 1)] * 9))
    with pytest.raises(ValueError):
        H.edit(ROOT, 8, ok, (0, 0), 4, H.params([]))
    with pytest.raises(ValueError):
        H.edit(ROOT, 12, ok, (0, 0), 4, H.params())
    for heights, p in ((np.zeros((0, 4), dtype=np.int64), H.params()), (ok, H.params([], None, None))):
        words, tally = H.edit(ROOT, 8, heights, (0, 0), 4, p)
        assert np.array_equal(words, ROOT) and not any(tally[k] for k in H.TALLIES)


def test_the_records_have_the_headers_layout(pkg):
    L, P = pkg._lib.HeightmapLayer, pkg._lib.HeightmapParams
    assert C.sizeof(L) == 8 and [(n, getattr(L, n).offset) for n, _ in L._fields_] == [("thickness", 0), ("colour", 4)]
    assert C.sizeof(P) == 120 and [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("depth", 0), ("n_layers", 4), ("n_words", 8), ("max_words", 16), ("origin_xz", 24), ("size_xz", 32), ("mode_below", 40), ("mode_above", 44),
        ("colour_above", 48), ("reserved", 52), ("layers", 56)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_heightmap_params \{(.*?)\} svo_heightmap_params;", header, re.S).group(1)
    assert re.findall(r"(?:uint32_t|uint64_t|svo_heightmap_layer) (\w+)", body) == [n for n, _ in P._fields_]
    assert re.search(r"#define SVO_HEIGHTMAP_MAX_LAYERS 8u", header) and len(P().layers) == H.MAX_LAYERS == 8
    assert re.search(r"#define SVO_HEIGHTMAP_TIMES 6\b[^\n]*\nint svo_heightmap_timing\(svo_ctx \*ctx, float ms_out\[SVO_HEIGHTMAP_TIMES\]\);", header)
    assert pkg.HEIGHTMAP_MODES == (None, "empty", "voxels", "set") and [H.MODES[m] for m in pkg.HEIGHTMAP_MODES] == [0, 1, 2, 3]


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_edit_heightmap.argtypes) == 4 and len(lib.svo_heightmap_minmax.argtypes) == 5 and len(lib.svo_heightmap_timing.argtypes) == 2
    assert callable(pkg.Render.edit_heightmap) and callable(pkg.Render.height_minmax) and callable(pkg.Render.from_heightmap)
    assert callable(pkg.Gpu.heightmap_timing)
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert all(name in text for name in NEW)


def test_python_refuses_what_it_can_see(pkg):
    with pytest.raises(ValueError):
        pkg.render._heightmap_mode("fill", "below")
    assert [pkg.render._heightmap_mode(m, "below") for m in pkg.HEIGHTMAP_MODES] == [0, 1, 2, 3]
