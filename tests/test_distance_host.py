"""Distance fields of a device tree (csrc/svo_distance.hip), CPU side: the two restatements of the rule
(tests/distance_ref.py: brute, the rule read literally, and separable, three window passes) agree on d2 and on every site,
and scipy's Euclidean transform on d2, in the three modes, on cases that hold ties, sites outside the box and outside the
grid, and cells at and just beyond the radius; the entry points are exported with signatures and declared in the header,
DistanceParams has the header's layout, the documents name the calls, and distance.py's helpers take the outputs apart."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import build_ref as B
import distance_ref as D
import sample_ref as S
from conftest import ROOT as REPO
from pass_frame import tree7_base

NEW = ("svo_nodes_distance", "svo_distance_timing")
MODES = (D.TO_VOXELS, D.TO_EMPTY, D.SIGNED)
# the boxes of the depth-7 tree: one cell, a row longer than a word of the bit rows, a slab; at the origin, in the middle
# and flush with the far corner
BOXES7 = {f"{'x'.join(map(str, size))}, {where}": (origin(size), size)
          for size in ((1, 1, 1), (5, 3, 67), (33, 40, 7))
          for where, origin in (("origin", lambda s: (0, 0, 0)), ("middle", lambda s: (60, 50, 30)),
                                ("far corner", lambda s: tuple(128 - v for v in s)))}
# R = 127 on a depth-9 grid: the issue's box, and one whose y pass takes more than one slab
R127_BOXES = (((200, 210, 100), (8, 8, 300)), ((200, 200, 100), (8, 30, 300)))


def r127_voxels():
    """22 voxels of a depth-9 grid: 8 near the low end of the R = 127 boxes, 14 about a hundred cells off their side, so that
    cells of the boxes reach a voxel only at more than 100 cells and others reach none"""
    rng = np.random.default_rng(127)
    return np.unique(np.concatenate([rng.integers((90, 100, 0), (130, 330, 512), (14, 3)), rng.integers((190, 190, 90), (220, 250, 160), (8, 3))]), axis=0)


@functools.lru_cache(maxsize=None)
def grid7():
    words = tree7_base()["words"]
    return S.sample_dense(words, words.size, (0, 0, 0), (128,) * 3, 7)


def n_nearest(site, size, R, d2):
    """per cell of the box, how many sites lie at its distance d2 (0 where it is FAR)"""
    count = np.zeros(tuple(size), dtype=np.int64)
    for o, d in zip(*D.ball(R)):
        count += (d2 == d) & site[tuple(slice(R + int(v), R + int(v) + n) for v, n in zip(o, size))]
    return count


def test_the_restatements_agree_and_the_cases_hold_what_they_should():
    grid = grid7()
    ties = outside_box = 0
    for name, (origin, size) in BOXES7.items():
        for R in (1, 6):
            occ = D.grown(grid, origin, size, R)
            for mode in MODES:
                what = f"{name}, R {R}, mode {mode}"
                a, b = D.by_mode(occ, size, R, mode, D.brute_sites), D.by_mode(occ, size, R, mode, D.separable_sites)
                assert a[0].dtype == np.int32 and a[1].dtype == np.uint32 and a[0].shape == tuple(size) == a[1].shape, what
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
                assert np.array_equal((a[0] == D.FAR) | (a[0] == -D.FAR), a[1] == D.NO_SITE), what
                if mode == D.SIGNED:
                    assert (a[0] != 0).all() and np.array_equal(a[0] < 0, occ[R:R + size[0], R:R + size[1], R:R + size[2]]), what
            d2, packed = D.by_mode(occ, size, R, D.TO_VOXELS, D.brute_sites)
            ties += int((n_nearest(occ, size, R, d2) >= 2).sum())
            p = packed[d2 != D.FAR].astype(np.int64)
            site = S.box_cells(origin, size)[(d2 != D.FAR).reshape(-1)] + np.stack([p >> 16 & 0xFF, p >> 8 & 0xFF, p & 0xFF], axis=1) - 128
            outside_box += int(((site < np.array(origin)) | (site >= np.array(origin) + size)).any(axis=1).sum())
            assert (grid[site[:, 0], site[:, 1], site[:, 2]] != 0).all()
    assert ties >= 100 and outside_box >= 1, (ties, outside_box)
    # to-empty mode at the far corner: the nearest empty cell of some voxel lies outside the grid
    origin, size = BOXES7["33x40x7, far corner"]
    d2, packed = D.brute_grid(grid, origin, size, 6, D.TO_EMPTY)
    p = packed[d2 != D.FAR].astype(np.int64)
    site = S.box_cells(origin, size)[(d2 != D.FAR).reshape(-1)] + np.stack([p >> 16 & 0xFF, p >> 8 & 0xFF, p & 0xFF], axis=1) - 128
    assert (site >= 128).any()
    # cells exactly at the radius, and cells whose nearest site is the smallest squared distance above it: 37 = 36 + 1
    origin, size = BOXES7["33x40x7, middle"]
    at, beyond = D.brute_grid(grid, origin, size, 6, D.TO_VOXELS)[0], D.brute_grid(grid, origin, size, 7, D.TO_VOXELS)[0]
    assert (at == 36).any() and ((beyond == 37) & (at == D.FAR)).any() and np.array_equal(at[at != D.FAR], beyond[at != D.FAR])


def test_scipy_agrees_on_d2():
    pytest.importorskip("scipy.ndimage")
    words = tree7_base()["words"]
    for name in ("5x3x67, origin", "33x40x7, middle", "33x40x7, far corner"):
        origin, size = BOXES7[name]
        for mode in MODES:
            assert np.array_equal(D.edt_d2(words, words.size, 7, origin, size, 6, mode), D.brute_grid(grid7(), origin, size, 6, mode)[0]), (name, mode)
    # brute() itself, from the words, is brute_grid() of their grid
    got, want = D.brute(words, words.size, 7, origin, size, 6, D.SIGNED), D.brute_grid(grid7(), origin, size, 6, D.SIGNED)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_random_box_and_the_site_list():
    rng = np.random.default_rng(24)
    cells = np.unique(rng.integers(0, 36, (187, 3)), axis=0) + 14  # the grown 24^3 box of a depth-6 grid, filled to 0.4 %
    words = B.build(cells, 6, rng.integers(1, 1 << 24, len(cells)))
    origin, size = (20, 20, 20), (24, 24, 24)
    for mode in MODES:
        a, b = D.brute(words, words.size, 6, origin, size, 6, mode), D.separable(words, words.size, 6, origin, size, 6, mode)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), mode
    got, want = D.from_sites(cells, origin, size, 6), D.brute(words, words.size, 6, origin, size, 6, D.TO_VOXELS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # R = 127's cases: within the grid, few voxels, FAR cells among them
    cells = r127_voxels()
    assert len(cells) <= 64 and (cells >= 0).all() and (cells < 512).all()
    for origin, size in R127_BOXES:
        assert all(o + s <= 512 for o, s in zip(origin, size))
    with pytest.raises(ValueError):
        D.brute(words, words.size, 6, origin, size, 128, 0)
    with pytest.raises(ValueError):
        D.brute(words, words.size, 6, (0, 0, 0), (4, 4, 4), 3, 3)


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_distance.argtypes) == 6 and len(lib.svo_distance_timing.argtypes) == 2
    assert callable(pkg.Render.distance_dense) and callable(pkg.Render.morph_ball) and callable(pkg.Gpu.distance_timing)
    assert (pkg.distance.FAR, pkg.distance.NO_SITE, pkg.distance.MAX_RADIUS) == (D.FAR, D.NO_SITE, D.MAX_RADIUS) == (0x7FFFFFFF, 0xFFFFFFFF, 127)
    assert pkg.distance.MODES == ("voxels", "empty", "signed") and "distance" in pkg.__all__
    # a call without a context answers SVO_ERR_ARG and touches nothing
    p = pkg._lib.DistanceParams()
    assert lib.svo_nodes_distance(None, C.byref(p), (C.c_uint32 * 3)(), (C.c_uint32 * 3)(), None, None) == -1
    assert lib.svo_distance_timing(None, (C.c_float * 5)()) == -1


def test_distance_params_have_the_headers_layout(pkg):
    P = pkg._lib.DistanceParams
    assert C.sizeof(P) == 24
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("flags", 0, 4), ("mode", 4, 4), ("depth", 8, 4), ("max_distance", 12, 4), ("n_words", 16, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_distance_params \{(.*?)\} svo_distance_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [("uint32_t", "flags"), ("uint32_t", "mode"), ("uint32_t", "depth"),
                                                                ("uint32_t", "max_distance"), ("uint64_t", "n_words")]


def test_the_header_and_the_documents_name_the_calls():
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    assert "exact distance fields of the tree in the node buffer (DESIGN.md 35)" in header
    assert header.index("int svo_sample_timing(") < header.index("svo_distance_params") < header.index("triangle meshes voxelised on the GPU")
    assert re.search(r"int svo_nodes_distance\(svo_ctx \*ctx, const svo_distance_params \*p, const uint32_t origin\[3\], "
                     r"const uint32_t size\[3\],\s*int32_t \*d2_out_dev, uint32_t \*site_out_dev[^,)]*\);", header)
    assert re.search(r"#define SVO_DISTANCE_TIMES 5\b[^\n]*\nint svo_distance_timing\(svo_ctx \*ctx, float ms_out\[SVO_DISTANCE_TIMES\]\);", header)
    for name, value in (("TO_VOXELS", "0u"), ("TO_EMPTY", "1u"), ("SIGNED", "2u"), ("MAX_RADIUS", "127u"), ("FAR", "0x7FFFFFFF"),
                        ("NO_SITE", "0xFFFFFFFFu"), ("SLAB_CELLS", r"\(1u << 21\)"), ("MAX_WORKSPACE", r"\(1ull << 30\)")):
        assert re.search(rf"#define SVO_DISTANCE_{name}\s+{value}", header), name
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("svo_nodes_distance", "svo_distance_timing", "svo_distance_params", "Render::distance_dense"):
        assert name in integration, name
    assert "distance_dense" in open(os.path.join(REPO, "include", "svo_render.hpp")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert re.search(r"^## 35\.", design, re.M) and "svo_nodes_distance" in design


def test_the_workspace_formula_of_the_wrapper_is_the_headers(pkg):
    W = pkg.Render._distance_workspace
    assert W((0, 0, 0), (0, 5, 5), 4, False) == 0
    # one word per row when the grown row fits an aligned run of 64; two when it straddles one
    assert W((0, 0, 70), (1, 1, 10), 3, False) == 7 * 7 * 1 * 8 + 7 * 1 * 10 * 4
    assert W((0, 0, 60), (1, 1, 10), 3, True) == 7 * 7 * 2 * 8 + 2 * 7 * 1 * 10 * 4
    assert W((0, 0, 0), (1, 1, 10), 3, False) == 7 * 7 * 2 * 8 + 7 * 1 * 10 * 4  # (the halo below z = 0 is a word of its own)
    # the whole depth-7 grid with R = 3: words from z = -64 to 128, slabs of 122 rows
    assert W((0, 0, 0), (128, 128, 128), 3, False) == 134 * 134 * 4 * 8 + 134 * 122 * 128 * 4
    assert W((0, 0, 0), (128, 128, 128), 3, True) == 134 * 134 * 4 * 8 + 2 * 134 * 122 * 128 * 4
    assert W((0, 0, 0), (1, 1, 1 << 21), 127, False) > 1 << 30


def test_the_helpers_of_distance_py(pkg):
    import torch
    dist = pkg.distance
    rng = np.random.default_rng(5)
    offsets = rng.integers(-127, 128, (4, 5, 6, 3))
    packed = dist.pack_sites(offsets)
    assert packed.shape == (4, 5, 6) and packed[0, 0, 0] == D.pack(offsets[0, 0, 0])
    packed = packed.astype(np.uint32)
    packed[1, 2, 3] = D.NO_SITE
    for given in (packed, torch.as_tensor(packed.view(np.int32))):  # (a device tensor holds the u32 as int32)
        got, valid = dist.unpack_sites(given)
        got, valid = np.asarray(got), np.asarray(valid)
        assert got.dtype == np.int32 and got.shape == (4, 5, 6, 3) and valid.sum() == 119 and not valid[1, 2, 3]
        assert np.array_equal(got[valid], offsets[valid]) and (got[1, 2, 3] == 0).all()
        cells, valid2 = dist.site_cells(given, (100, 200, 300))
        cells = np.asarray(cells)
        assert np.array_equal(np.asarray(valid2), valid) and cells.shape == (4, 5, 6, 3)
        assert np.array_equal(cells[valid], (S.box_cells((100, 200, 300), (4, 5, 6)).reshape(4, 5, 6, 3) + offsets)[valid])
    assert np.array_equal(np.asarray(dist.pack_sites(torch.as_tensor(offsets))), dist.pack_sites(offsets))
    d2 = np.array([0, 1, 9, 10, -9, -10, D.FAR, -D.FAR], dtype=np.int32)
    for given in (d2, torch.as_tensor(d2)):
        assert np.asarray(dist.within(given, 3)).tolist() == [True, True, True, False, True, False, False, False]
        assert np.asarray(dist.within(given, 0)).tolist() == [True] + [False] * 7
    with pytest.raises(ValueError):
        dist.within(d2, -1)
    with pytest.raises(ValueError):
        dist.site_cells(packed.reshape(-1), (0, 0, 0))
