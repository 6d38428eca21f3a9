"""Simplification of a tree in the node buffer (csrc/svo_simplify.hip), CPU side: the entry points are
exported with signatures; the sequential restatement (tests/simplify_ref.py: simplify), the kernels' formulation
(simplify_parallel) and the per-cell statement on a dense grid agree on solid, filled, sparse and edited trees; a depth-3
case written out by hand; the tallies that tell the mechanisms apart; the properties of MERGE, min_level and CUT; and
oracle frames of a merged against an unmerged solid ball."""
import ctypes as C
import functools

import numpy as np
import pytest

import build_ref as B
import compact_ref as K
import edit_ref as E
import list_ref as L
import region_ref as G
import simplify_ref as R
import world_build_ref as W

NEW = ("svo_nodes_simplify", "svo_simplify_timing")
VO = B.VOXEL_OFFSET
# every way to call it: (merge, cut_level, min_level)
MODES = ((True, None, 0), (True, None, 3), (False, 3, 0), (True, 3, 0), (True, 4, 3), (False, 5, 0), (True, 2, 0), (False, 1, 0))


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_simplify.argtypes) == 5 and len(lib.svo_simplify_timing.argtypes) == 2
    assert C.sizeof(pkg._lib.SimplifyParams) == 32
    assert callable(pkg.Render.simplify_nodes) and callable(pkg.Gpu.simplify_timing)


def grid_cells(depth):
    ax = np.arange(1 << depth)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1)


def ball_voxels(depth, radius=0.4, colour=0x80C0FF):
    """a solid ball about the grid's centre, in one colour"""
    c = grid_cells(depth)
    side = 1 << depth
    coords = c[((c - (side / 2 - 0.5)) ** 2).sum(-1) <= (side * radius) ** 2]
    return coords, np.full(len(coords), colour, dtype=np.int64)


def box_voxels(depth):
    """a solid box aligned to level 2, and 40 stray voxels of other colours"""
    q = 1 << (depth - 2)
    c = grid_cells(depth)
    inside = (c[..., 0] >= q) & (c[..., 0] < 3 * q) & (c[..., 1] < 2 * q) & (c[..., 2] >= 2 * q)
    coords = c[inside]
    rng = np.random.default_rng(depth)
    stray = rng.integers(0, 1 << depth, (40, 3))
    stray = stray[~inside[tuple(stray.T)]]
    return np.concatenate([coords, stray]), np.concatenate([np.full(len(coords), 0xA05020), rng.integers(1, 1 << 24, len(stray))])


def field_voxels(depth, per_column):
    """a height field with its columns filled below the surface: stone under two layers of grass, or one colour of its
    own per column (then no group holds eight equal words)"""
    side = 1 << depth
    x, z = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    h = (side * (0.45 + 0.2 * np.sin(x / side * 5.0) * np.cos(z / side * 4.0) + 0.1 * np.sin((x + 2 * z) / side * 9.0))).astype(np.int64)
    c = grid_cells(depth)
    filled = c[..., 1] < h[:, None, :]
    coords = c[filled]
    if per_column:
        colours = 1 + coords[:, 0] * side + coords[:, 2]
    else:
        colours = np.where(coords[:, 1] >= h[coords[:, 0], coords[:, 2]] - 2, 0x30A040, 0x808080)
    return coords, colours.astype(np.int64)


def sparse_voxels(depth, n=500):
    rng = np.random.default_rng(11)
    return rng.integers(0, 1 << depth, (n, 3)), rng.choice([0xFF0000, 0x00FF00, 0x0000FF], n)


@functools.lru_cache(maxsize=None)
def scenes():
    """{name: (words, depth)}: computed once, shared with the GPU tests; nobody writes to the arrays"""
    out = {}
    for name, depth, (coords, colours) in (("ball6", 6, ball_voxels(6)), ("box6", 6, box_voxels(6)), ("field6", 6, field_voxels(6, False)),
                                           ("columns5", 5, field_voxels(5, True)), ("sparse5", 5, sparse_voxels(5)),
                                           ("ball7", 7, ball_voxels(7, 0.3))):
        out[name] = (B.build(coords, depth, colours), depth)
    # the ball carved, filled and painted by shapes: coarse leaves, cut-off subtrees and appended groups
    ball, _ = out["ball6"]
    sh = G.shapes([G.box((8, 8, 8), (40, 24, 56), 0), G.ball((90, 90, 64), 30, 0x123456), G.box((0, 32, 0), (64, 40, 64), 0xFFEE00, G.MODE_VOXELS)])
    out["ball6_shapes"] = (G.edit(ball, ball.size, sh, 6)[0], 6)
    # the box with voxels removed (groups left all empty), a stray put into the solid, in put order
    box, _ = out["box6"]
    rng = np.random.default_rng(5)
    gone = np.concatenate([grid_cells(6)[16:24, 0:8, 32:40].reshape(-1, 3), rng.integers(0, 64, (300, 3))])
    colours = np.concatenate([np.zeros(len(gone) - 100, dtype=np.int64), rng.integers(1, 1 << 24, 100)])
    out["box6_edited"] = (E.edit(box, box.size, gone, 6, colours), 6)
    # the merged ball edited by cell list: the coarse leaf is split into empty children
    merged = R.simplify(ball, ball.size)[0]
    out["ball6_merged_edited"] = (E.edit(merged, merged.size, [[32, 32, 32], [10, 50, 20]], 6, [0xFF00FF, 0x00FFFF]), 6)
    # counters on every word, and a group of eight equal values above 24 bits
    counted = out["field6"][0] | np.random.default_rng(8).integers(0, 16, out["field6"][0].size).astype(np.uint32)
    out["field6_counters"] = (counted, 6)
    high = ball.copy()
    last = high.size - 8  # the last group of the deepest level: eight leaves
    assert (high[last:] >> 4 >= VO).all()
    high[last:] = (VO + 0x5000007) << 4
    high[last - 8:last] = np.where(high[last - 8:last] >> 4 > VO, (VO + 0x5000007) << 4 | 3, high[last - 8:last])
    out["ball6_high"] = (high, 6)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """(out, perm) of simplify() for a scene and one of MODES, computed once"""
    words, _ = scenes()[name]
    merge, cut_level, min_level = mode
    return R.simplify(words, words.size, merge, cut_level, min_level)


def check_cells(words, depth, out, cut_level):
    """the per-cell statement: a lossless call leaves every cell; a cut gives every cell S of its cube"""
    want = R.cells(words, words.size, depth) if cut_level is None else R.cut_cells(words, words.size, depth, cut_level)
    assert np.array_equal(R.cells(out, out.size, depth), want)


@pytest.mark.parametrize("name", ["ball6", "box6", "field6", "columns5", "sparse5", "ball6_shapes", "box6_edited", "ball6_merged_edited",
                                  "field6_counters", "ball6_high"])
def test_both_restatements_and_the_cells_agree(name):
    words, depth = scenes()[name]
    for mode in MODES:
        merge, cut_level, min_level = mode
        out, perm = reference(name, mode)
        got, got_perm = R.simplify_parallel(words, words.size, merge, cut_level, min_level)
        assert np.array_equal(out, got) and np.array_equal(perm, got_perm), (name, mode)
        assert out.size <= words.size and out.size % 8 == 0
        check_cells(words, depth, out, cut_level)
        # counters: a kept word keeps its 4 bits, a rewritten word has 0
        rewritten = (words[perm] >> 4 < VO) & (out >> 4 >= VO)
        assert np.array_equal((out & 15)[~rewritten], (words[perm] & 15)[~rewritten]) and not (out & 15)[rewritten].any()


def test_depth_3_by_hand():
    a, b, c, red = VO + 0x2040AA, VO + 0x102030, VO + 0x506070, VO + 0xFF0000
    e = B.EMPTY
    words = np.array([
        8 << 4 | 1, red << 4 | 2, 24 << 4 | 3, 40 << 4 | 4, e, e, e, e | 5,                      # the root group
        16 << 4 | 6, a << 4, a << 4 | 7, a << 4, a << 4, a << 4, a << 4, a << 4,                 # 8: A once its first word is
        a << 4, a << 4 | 1, a << 4 | 2, a << 4 | 3, a << 4, a << 4, a << 4, a << 4 | 9,          # 16: eight A, counters differ
        b << 4, b << 4, b << 4, 32 << 4 | 8, b << 4, b << 4, b << 4, b << 4 | 1,                 # 24: seven B and an interior word
        b << 4, b << 4, b << 4, b << 4, b << 4 | 2, c << 4, b << 4, b << 4,                      # 32: seven B and one C
        e, e | 1, e, e, e, e, e, e,                                                              # 40: nothing
    ], dtype=np.uint32)
    merged = np.array([
        a << 4, red << 4 | 2, 8 << 4 | 3, e, e, e, e, e | 5,
        b << 4, b << 4, b << 4, 16 << 4 | 8, b << 4, b << 4, b << 4, b << 4 | 1,
        b << 4, b << 4, b << 4, b << 4, b << 4 | 2, c << 4, b << 4, b << 4,
    ], dtype=np.uint32)
    merged_perm = np.concatenate([np.arange(8), np.arange(24, 40)])
    # at level 2 the interior words are 8 + 0 (all A) and 24 + 3 (seven B and a C: (7 * 0x30 + 0x70) // 8 = 0x38, ...)
    mixed = VO + 0x182838
    cut2 = np.array([
        8 << 4 | 1, red << 4 | 2, 16 << 4 | 3, 24 << 4 | 4, e, e, e, e | 5,
        a << 4, a << 4, a << 4 | 7, a << 4, a << 4, a << 4, a << 4, a << 4,
        b << 4, b << 4, b << 4, mixed << 4, b << 4, b << 4, b << 4, b << 4 | 1,
        e, e | 1, e, e, e, e, e, e,
    ], dtype=np.uint32)
    cut2_perm = np.concatenate([np.arange(16), np.arange(24, 32), np.arange(40, 48)])
    both = np.array([
        a << 4, red << 4 | 2, 8 << 4 | 3, e, e, e, e, e | 5,
        b << 4, b << 4, b << 4, mixed << 4, b << 4, b << 4, b << 4, b << 4 | 1,
    ], dtype=np.uint32)
    both_perm = np.concatenate([np.arange(8), np.arange(24, 32)])
    # S of the root's words: A; red; the mean of seven B and `mixed`; nothing
    s2 = VO + (((7 * 0x30 + 0x38) // 8) | ((7 * 0x20 + 0x28) // 8) << 8 | ((7 * 0x10 + 0x18) // 8) << 16)
    cut1 = np.array([a << 4, red << 4 | 2, s2 << 4, e, e, e, e, e | 5], dtype=np.uint32)
    # min_level 2: the root's words stay interior although groups 8 and 40 are uniform; 8 + 0 still becomes A
    min2 = np.array([
        8 << 4 | 1, red << 4 | 2, 16 << 4 | 3, 24 << 4 | 4, e, e, e, e | 5,
        a << 4, a << 4, a << 4 | 7, a << 4, a << 4, a << 4, a << 4, a << 4,
        b << 4, b << 4, b << 4, 32 << 4 | 8, b << 4, b << 4, b << 4, b << 4 | 1,
        e, e | 1, e, e, e, e, e, e,
        b << 4, b << 4, b << 4, b << 4, b << 4 | 2, c << 4, b << 4, b << 4,
    ], dtype=np.uint32)
    min2_perm = np.concatenate([np.arange(16), np.arange(24, 32), np.arange(40, 48), np.arange(32, 40)])
    for kw, want, want_perm in ((dict(), merged, merged_perm), (dict(merge=False, cut_level=2), cut2, cut2_perm),
                                (dict(cut_level=2), both, both_perm), (dict(merge=False, cut_level=1), cut1, np.arange(8)),
                                (dict(min_level=2), min2, min2_perm)):
        for f in (R.simplify, R.simplify_parallel):
            out, perm = f(words, words.size, **kw)
            assert np.array_equal(out, want), (kw, f.__name__, out, want)
            assert np.array_equal(perm, want_perm), (kw, f.__name__)


def test_tallies_tell_the_mechanisms_apart():
    s = scenes()
    t = {name: R.tally(w, w.size) for name, (w, _) in s.items() if name != "ball7"}
    # merges that cascade over at least 3 levels; the box aligned to level 2 merges up to level 2
    assert t["ball6"]["cascade"] >= 3 and t["box6"]["cascade"] == 4 and t["box6"]["coarsest"] == 2
    # seven equal leaves and a non-uniform interior word: no merge there
    assert t["ball6"]["seven_of_eight"] > 100 and t["field6"]["seven_of_eight"] > 10
    # equal values with different counters merge; a value above 24 bits merges with itself only
    assert t["field6_counters"]["merged_counters"] > 50 and t["field6_counters"]["merged"] == t["field6"]["merged"] > 100
    assert t["ball6_high"]["merged_high"] == 1 and t["ball6_high"]["merged"] > t["ball6"]["merged"]
    # groups that hold nothing merge into the empty word
    assert t["box6_edited"]["merged_empty"] >= 1 and t["ball6_merged_edited"]["merged"] == 0
    # nothing to merge: distinct colours per column, a sparse list
    assert t["columns5"]["merged"] == 0 and t["sparse5"]["merged"] == 0
    assert t["ball6_shapes"]["merged"] > 100
    cut = R.tally(s["ball6"][0], s["ball6"][0].size, False, 3)
    assert cut["cut"] > 100 and cut["merged"] == 0


def test_merge_properties():
    s = scenes()
    for name in ("ball6", "box6_edited", "ball6_shapes", "field6_counters"):
        words, depth = s[name]
        out, _ = reference(name, MODES[0])
        assert out.size < K.compact(words, words.size, True)[0].size, name
        # idempotent: a merged tree is canonical and merges no further
        again, perm = R.simplify(out, out.size)
        assert np.array_equal(again, out) and np.array_equal(perm, np.arange(out.size)), name
        # the expanded list is the list before
        for a, b in zip(L.list_voxels(words, words.size, depth, expand=True), L.list_voxels(out, out.size, depth, expand=True)):
            assert np.array_equal(a, b), name
    # no eight equal siblings: the merge is the pruning compaction, bit for bit
    for name in ("columns5", "sparse5"):
        words, _ = s[name]
        for a, b in zip(reference(name, MODES[0]), K.compact(words, words.size, True)):
            assert np.array_equal(a, b), name
    words, _ = s["box6_edited"]
    empties = np.where(words >> 4 >= VO, B.EMPTY, words).astype(np.uint32)  # every leaf emptied: only the rule for empty is left
    assert np.array_equal(R.simplify(empties, empties.size)[0], K.compact(empties, empties.size, True)[0])
    assert R.simplify(empties, empties.size)[0].size == 8


def levels_of(words):
    """the level of every word of a canonical tree"""
    level = np.zeros(words.size, dtype=np.int64)
    lo, hi, l = 0, 1, 1
    while hi > lo:
        level[8 * lo:8 * hi] = l
        n = int((words[8 * lo:8 * hi] >> 4 < VO).sum())
        lo, hi, l = hi, hi + n, l + 1
    return level


def test_min_level_bounds_the_merge():
    for name in ("ball6", "box6"):
        words, _ = scenes()[name]
        free, perm_free = R.simplify_parallel(words, words.size)
        for m in (0, 1):
            assert np.array_equal(R.simplify_parallel(words, words.size, min_level=m)[0], free)
        sizes = [free.size]
        for m in (2, 3, 4, 5, 6, 7):
            out, perm = R.simplify_parallel(words, words.size, min_level=m)
            made = (words[perm] >> 4 < VO) & (out >> 4 >= VO)  # leaves that the merge made
            assert made.any() == (m <= 5) and (levels_of(out)[made] >= m).all(), (name, m)
            sizes.append(out.size)
        assert sizes == sorted(sizes) and sizes[0] < sizes[3] < sizes[-1] == words.size
        assert np.array_equal(R.simplify_parallel(words, words.size, min_level=7)[0], K.compact(words, words.size, False)[0])


def test_cut_properties():
    for name in ("ball6", "field6", "ball6_shapes"):
        words, depth = scenes()[name]
        plain = K.compact(words, words.size, False)
        for level in (depth, depth + 1, 31):  # at or below the tree's depth: the identity up to layout
            for a, b in zip(R.simplify_parallel(words, words.size, False, level), plain):
                assert np.array_equal(a, b)
        out, perm = R.simplify_parallel(words, words.size, False, 1)
        assert out.size == 8 and (out >> 4 >= VO).all() and np.array_equal(perm, np.arange(8))
        sizes = [R.simplify_parallel(words, words.size, False, level)[0].size for level in range(1, depth + 1)]
        assert sizes == sorted(sizes) and len(set(sizes)) == depth
    # unit leaves only: S is the mip pyramid of the dense grid, and a cut at L shows it
    for name in ("ball6", "field6", "sparse5"):
        words, depth = scenes()[name]
        pyramid = R.mip_pyramid(R.cells(words, words.size, depth))
        for level in (2, 4):
            side = 1 << (depth - level)
            want = np.repeat(np.repeat(np.repeat(pyramid[level], side, 0), side, 1), side, 2)
            assert np.array_equal(R.cut_cells(words, words.size, depth, level), want), (name, level)


def test_s_is_the_worlds_mip_colour():
    rng = np.random.default_rng(24)
    rgb = rng.integers(0, 256, (500, 8, 3))
    rgb[rng.random((500, 8)) < 0.4] = 0
    rgb[:5] = 0      # no voxel: S = 0 where mip gives (1, 1, 1)
    rgb[5:10, :, 1] = 0  # a channel that averages to 0 becomes 1
    values = rgb[..., 0] | rgb[..., 1] << 8 | rgb[..., 2] << 16
    got = np.array([R.mip_value(v) for v in values])
    want = W.mip(rgb)
    some = rgb.any(axis=2).any(axis=1)
    assert np.array_equal(got[some], (want[:, 0] | want[:, 1] << 8 | want[:, 2] << 16)[some])
    assert not got[~some].any() and (want[~some] == 1).all() and (~some).sum() >= 5


def test_merged_and_unmerged_balls_trace_alike(O):
    """a ray reaches a solid only through the empty leaf in front of it: the frames differ in voxel index and depth only"""
    words, _ = scenes()["ball7"]
    merged = R.simplify_parallel(words, words.size)[0]
    assert merged.size < words.size // 4
    for pos, look in (((0.1, 0.2, -1.5), (0.0, 0.0, 1.5)), ((1.4, 1.2, 1.3), (-1.0, -0.8, -1.0)), ((0.9, 0.85, -0.9), (-1.0, -1.0, 1.0))):
        u = O.make_uniforms(pos=pos, look=look, width=64, height=64)
        assert_frames_alike(O, O.trace_frame(words, u, threads=4), words, O.trace_frame(merged, u, threads=4), merged, str(pos))


def assert_frames_alike(O, a, words_a, b, words_b, what):
    a, b = a.reshape(-1), b.reshape(-1)
    ia, ib = O.unpack_info(a["info"]), O.unpack_info(b["info"])
    for f in ("hit", "steps", "normal"):
        assert np.array_equal(ia[f], ib[f]), f"{what}: {f}"
    assert np.array_equal(a["normal_bits"], b["normal_bits"]) and np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32)), what
    on_a, on_b = a["value"] < words_a.size, b["value"] < words_b.size  # (the rest are the sentinels of a miss)
    assert np.array_equal(on_a, on_b) and np.array_equal(a["value"][~on_a], b["value"][~on_a]), what
    hit = on_a & (ia["hit"] == 1)
    assert hit.sum() > 200 and np.array_equal(words_a[a["value"][hit]] >> 4, words_b[b["value"][hit]] >> 4), what
    assert (ia["depth"] != ib["depth"]).any() and (ia["depth"] >= ib["depth"]).all(), what
