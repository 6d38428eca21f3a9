"""The visible surface merged into rectangles (csrc/svo_surface_merge.hip), CPU side: the contract's numpy
restatement (tests/surface_merge_ref.py: merge_rects) against the independent dense greedy mesher on uniform trees; on
every case the rectangles painted back cover the exposed faces' cells exactly once, with their values, and nothing is left
to join; the smallest trees, a depth-21 root, mixed levels over the rounds, a second round that joins what the first could
not, any_value; mesh.rects_to_mesh on CPU tensors (equal to quads_to_mesh on squares, area, signed volume, the .obj round
trip); the entry points are exported and SurfaceMergeParams has the header's layout."""
import ctypes as C
import functools
import os
import re

import numpy as np
import torch

import build_ref as B
import surface_merge_ref as M
import surface_ref as S
from conftest import ROOT as REPO
from test_list_host import EMPTY_ROOT, leaf_words, mixed_levels, one_leaf_root
from test_surface_host import ball

NEW = ("svo_nodes_merge_surface", "svo_surface_merge_timing")


def block_grid():
    """a solid 4 x 4 x 4 block of one colour, off the centre of the depth-3 grid"""
    grid = np.zeros((8, 8, 8), dtype=np.int64)
    grid[1:5, 3:7, 2:6] = 0x336699
    return grid


def two_colour_grid():
    """the same block, its upper half in a second colour"""
    grid = block_grid()
    grid[1:5, 5:7, 2:6] = 0x993366
    return grid


def second_round_tree():
    """depth 2, written out by hand: the level-1 leaf [0, 2)^3 and, beside it in x, the four unit leaves (2..3, 0..1, 1),
    all of one colour.  On the plane z = 2 the leaf's 2 x 2 and the four unit faces lie side by side: round 1 joins the
    unit faces to a 2 x 2 (two rows along u = x, then the rows along v = y), and only round 2 finds that 2 x 2 in the
    class (v0, h) = (0, 2) of the leaf's face and joins the two."""
    words = np.full(16, B.EMPTY, dtype=np.uint32)
    colour = leaf_words([0x00C0FFEE & 0xFFFFFF])[0]
    words[0] = colour            # the child (0, 0, 0) of the root: a level-1 leaf
    words[4] = 8 << 4            # the child (1, 0, 0): the group at word 8
    words[[9, 11, 13, 15]] = colour  # its children (x, y, 1): index x * 4 + y * 2 + 1
    return words


def uniform_root(value=0x123456):
    """a root group of 8 leaves of one colour"""
    return leaf_words([value] * 8)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (words, depth, dense grid or None): every tree the host and the GPU tests merge.  Nobody writes to them."""
    out = {}
    for name, grid, depth in (("ball", ball(64, 20), 6), ("block", block_grid(), 3), ("two colours", two_colour_grid(), 3)):
        coords, colours = B.dense_to_voxels(grid)
        out[name] = (B.build(coords, depth, colours), depth, grid)
    out["uniform root at depth 21"] = (uniform_root(), 21, None)
    out["uniform root at depth 1"] = (uniform_root(), 1, None)
    out["one voxel at depth 1"] = (one_leaf_root(), 1, None)
    out["empty"] = (EMPTY_ROOT.copy(), 5, None)
    out["mixed levels"] = (mixed_levels(), 6, None)
    out["second round"] = (second_round_tree(), 2, None)
    return out


@functools.lru_cache(maxsize=None)
def _quads_of(name, closed):
    words, depth, _ = cases()[name]
    return S.list_surface(words, words.size, depth, S.QUADS | (S.CLOSED_BOUNDARY if closed else 0))


def quads_of(name, closed=False):
    """the reference quads of a case, computed once per session"""
    return _quads_of(name, bool(closed))


@functools.lru_cache(maxsize=None)
def _merged(name, closed, rounds, any_value):
    return M.merge_rects(quads_of(name, closed), cases()[name][1], rounds, any_value)


def merged(name, closed=False, rounds=1, any_value=False):
    """merge_rects of a case, computed once per session and shared with the GPU tests"""
    return _merged(name, bool(closed), int(rounds), bool(any_value))


def check_cells(name, closed, rounds, any_value, uniform):
    """the rectangles cover the exposed faces' unit cells exactly once, each with the value of the faces under it; after
    the V phase nothing follows along v; along u nothing follows either in a uniform tree, or in any tree when a further
    round would join nothing"""
    depth = cases()[name][1]
    rects, values = merged(name, closed, rounds, any_value)
    quads = M.quads_to_rects(quads_of(name, closed), depth)
    shift = min([depth] + [int(x & -x).bit_length() - 1 for x in quads[0][:, 1:].reshape(-1).tolist() if x])  # the common scale
    shift = max(shift, depth - 7)
    scaled = lambda r: np.concatenate([np.asarray(r).astype(np.int64)[:, :1], np.asarray(r).astype(np.int64)[:, 1:] >> shift], axis=1)  # noqa: E731
    assert all((np.asarray(r).astype(np.int64)[:, 1:] & ((1 << shift) - 1) == 0).all() for r in (rects, quads[0]))
    want_count, want_value = M.raster(scaled(quads[0]), np.zeros_like(quads[1]) if any_value else quads[1], depth - shift)
    count, value = M.raster(scaled(rects), values, depth - shift)
    assert want_count.max(initial=0) <= 1, f"{name}: the input faces overlap"
    assert np.array_equal(count, want_count), f"{name}: {(count != want_count).sum()} cells painted too often or not at all"
    assert np.array_equal(value, want_value), f"{name}: a rectangle covers faces of another value"
    assert M.followers(rects, values, 1, any_value) == 0, f"{name}: a rectangle still follows another along v"
    if uniform or (rounds < 4 and len(merged(name, closed, rounds + 1, any_value)[0]) == len(rects)):
        assert M.followers(rects, values, 0, any_value) == 0, f"{name}: a rectangle still follows another along u"
    order = np.lexsort((rects[:, 3], rects[:, 4], rects[:, 2], rects[:, 1], rects[:, 0]))
    assert np.array_equal(order, np.arange(len(rects))), f"{name}: not ascending in (face, plane, u0, w, v0)"
    return rects, values


def test_the_restatements_agree_on_uniform_trees():
    for name in ("ball", "block"):
        _, depth, grid = cases()[name]
        for closed in (False, True):
            rects, values = check_cells(name, closed, 1, False, True)
            want = M.greedy_dense(grid, closed)
            assert rects.shape == want[0].shape and np.array_equal(rects, want[0]) and np.array_equal(values, want[1]), (name, closed)
            quads = quads_of(name, closed)[3].size
            if name == "block":
                assert (len(rects), quads) == (6, 96)
                assert sorted(rects[:, 0].tolist()) == list(range(6)) and (rects[:, 4:] == 4).all()
                assert rects[:, 1].tolist() == [1, 5, 3, 7, 2, 6]
            else:  # (nearly every cell of the ball has a colour of its own: only any_value joins much)
                joined, zeros = check_cells(name, closed, 1, True, True)
                assert 1000 < len(joined) < quads / 2 < len(rects) <= quads and not zeros.any()
                assert np.array_equal(joined, M.greedy_dense(grid != 0, closed)[0])
    # a second round changes nothing in a uniform tree
    for a, b in zip(merged("ball", rounds=2), merged("ball")):
        assert np.array_equal(a, b)


def test_small_cases():
    rects, values = check_cells("uniform root at depth 21", False, 1, False, True)
    side = 1 << 21
    assert rects.tolist() == [[f, (f & 1) * side, 0, 0, side, side] for f in range(6)] and (values == 0x123456).all()
    assert len(merged("uniform root at depth 21", closed=True)[0]) == 0
    rects, _ = check_cells("uniform root at depth 1", False, 1, False, True)
    assert rects.tolist() == [[f, (f & 1) * 2, 0, 0, 2, 2] for f in range(6)]
    rects, values = check_cells("one voxel at depth 1", False, 1, False, True)  # the child 5: the cell (1, 0, 1)
    assert rects.tolist() == [[0, 1, 0, 1, 1, 1], [1, 2, 0, 1, 1, 1], [2, 0, 1, 1, 1, 1], [3, 1, 1, 1, 1, 1], [4, 1, 1, 0, 1, 1], [5, 2, 1, 0, 1, 1]]
    assert (values == 0xABCDEF).all()
    for rounds in (1, 4):
        assert merged("empty", rounds=rounds)[0].shape == (0, 6) and merged("empty", rounds=rounds)[1].shape == (0,)
    for bad in (0, 5):
        try:
            M.merge_rects(quads_of("empty"), 5, bad)
            raise AssertionError("not refused")
        except ValueError:
            pass


def test_mixed_levels_over_the_rounds():
    quads = quads_of("mixed levels")[3].size
    for any_value in (False, True):  # (3 000 random voxels with random colours: few faces touch, fewer share a value)
        counts = []
        for rounds in (1, 2, 3, 4):
            for closed in (False, True) if rounds < 3 else (False,):
                check_cells("mixed levels", closed, rounds, any_value, False)
            counts.append(len(merged("mixed levels", rounds=rounds, any_value=any_value)[0]))
        assert all(a >= b for a, b in zip(counts, counts[1:])) and counts[0] <= quads, counts
        if any_value:
            assert counts[0] < quads - 300, counts
    assert set(np.unique(merged("mixed levels", any_value=True)[0][:, 4:]).tolist()) >= {1, 2, 4, 8}  # extents of several levels


def test_a_second_round_joins_a_coarse_face_and_the_unit_faces_beside_it():
    first, _ = check_cells("second round", False, 1, False, False)
    second, _ = check_cells("second round", False, 2, False, False)
    assert len(second) < len(first)
    top = lambda r: r[(r[:, 0] == 5) & (r[:, 1] == 2)].tolist()  # noqa: E731
    assert top(first) == [[5, 2, 0, 0, 2, 2], [5, 2, 2, 0, 2, 2]] and top(second) == [[5, 2, 0, 0, 4, 2]]
    assert len(first) - len(second) == 1  # (nowhere else do a coarse and a joined face share a class)
    assert np.array_equal(merged("second round", rounds=3)[0], second)


def test_any_value_joins_across_colours():
    for closed in (False, True):
        plain, values = check_cells("two colours", closed, 1, False, True)
        joined, zeros = check_cells("two colours", closed, 1, True, True)
        assert len(joined) < len(plain) and len(set(values.tolist())) == 2 and not zeros.any()
    assert len(merged("two colours")[0]) == 10 and len(merged("two colours", any_value=True)[0]) == 6
    assert len(merged("uniform root at depth 21", any_value=True)[0]) == 6


def tensors(*arrays):
    return [torch.from_numpy(np.asarray(a).astype(np.int32)) for a in arrays]


def signed_volume_x6(vertices, triangles):
    v, t = vertices.numpy().astype(np.int64), triangles.numpy().astype(np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return int((a * np.cross(b, c)).sum())


def test_rects_to_mesh_on_cpu_tensors(pkg, tmp_path):
    mesh = pkg.mesh
    # squares: the mesh of the quads
    xyz, value, level, face = quads_of("mixed levels")
    squares, _ = M.quads_to_rects((xyz, value, level, face), 6)
    for weld in (True, False):
        for integer in (True, False):
            got = mesh.rects_to_mesh(*tensors(squares, value), 6, weld=weld, integer=integer)
            want = mesh.quads_to_mesh(*tensors(xyz, face, level), 6, tensors(value)[0], weld=weld, integer=integer)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.numpy().tobytes() == w.numpy().tobytes(), (weld, integer)
    assert mesh.rects_to_mesh(*tensors(squares), None, 6)[2] is None
    recoloured = mesh.rects_to_mesh(*tensors(squares, value), 6, colours=tensors(value + 1)[0])[2]
    assert np.array_equal(recoloured.numpy(), np.repeat(value.astype(np.int32) + 1, 2))
    # merged: the area is the exposed unit faces', the normals point outwards
    for name in ("mixed levels", "ball", "second round"):
        depth = cases()[name][1]
        quads = M.quads_to_rects(quads_of(name), depth)[0]
        rects, values = merged(name, rounds=2)
        vi, tri, col = mesh.rects_to_mesh(*tensors(rects, values), depth, integer=True)
        assert vi.dtype == torch.int32 and tri.shape == (2 * len(rects), 3) and np.array_equal(col.numpy(), np.repeat(values.astype(np.int32), 2))
        v, t = vi.numpy().astype(np.int64), tri.numpy().astype(np.int64)
        normal = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        f2 = np.repeat(rects[:, 0].astype(np.int64), 2)
        area2 = np.repeat(rects[:, 4].astype(np.int64) * rects[:, 5], 2)
        assert np.array_equal(normal, np.eye(3, dtype=np.int64)[f2 >> 1] * (np.where(f2 & 1, 1, -1) * area2)[:, None])
        assert int(np.abs(normal).sum()) == 2 * int((quads[:, 4] * quads[:, 5]).sum())
        vf = mesh.rects_to_mesh(*tensors(rects, values), depth)[0]
        assert vf.dtype == torch.float32 and np.array_equal(vf.numpy().astype(np.float64), v / (1 << depth - 1) - 1)
    # a uniform-depth solid with the open boundary: the signed volume is the voxel count
    for name in ("ball", "block", "two colours"):
        words, depth, grid = cases()[name]
        for any_value in (False, True):
            vi, tri, _ = mesh.rects_to_mesh(*tensors(*merged(name, any_value=any_value)), depth, integer=True)
            assert signed_volume_x6(vi, tri) == 6 * int((grid != 0).sum()), name
    # the merged mesh goes through a Wavefront file bit for bit
    v, t, _ = mesh.rects_to_mesh(*tensors(*merged("ball")), 6)
    path = str(tmp_path / "ball.obj")
    mesh.save_obj(path, v, t)
    got_v, got_t, _ = mesh.load_obj(path)
    assert got_v.tobytes() == v.numpy().tobytes() and got_t.dtype == np.int32 and got_t.tobytes() == t.numpy().tobytes()
    # no rectangles: an empty mesh
    none = torch.zeros((0, 6), dtype=torch.int32)
    v, t, c = mesh.rects_to_mesh(none, none[:, 0], 5)
    assert v.shape == (0, 3) and t.shape == (0, 3) and c.shape == (0,)
    for bad in (0, 22):
        try:
            mesh.rects_to_mesh(none, none[:, 0], bad)
            raise AssertionError("not refused")
        except ValueError:
            pass


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_merge_surface.argtypes) == 5 and len(lib.svo_surface_merge_timing.argtypes) == 2
    assert callable(pkg.Render.surface_rects) and callable(pkg.Gpu.surface_merge_timing) and callable(pkg.mesh.rects_to_mesh)


def test_merge_params_have_the_headers_layout(pkg):
    P = pkg._lib.SurfaceMergeParams
    assert C.sizeof(P) == 32
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("flags", 0, 4), ("depth", 4, 4), ("rounds", 8, 4), ("reserved", 12, 4), ("n_words", 16, 8), ("max_entries", 24, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_surface_merge_params \{(.*?)\} svo_surface_merge_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [("uint32_t", "flags"), ("uint32_t", "depth"), ("uint32_t", "rounds"),
                                                             ("uint32_t", "reserved"), ("uint64_t", "n_words"), ("uint64_t", "max_entries")]
    assert re.search(r"int svo_nodes_merge_surface\(svo_ctx \*ctx, const svo_surface_merge_params \*p, uint32_t \*rect_out_dev, "
                     r"uint32_t \*value_out_dev,\s*uint64_t \*n_out\);", header)
    assert re.search(r"#define SVO_SURFACE_MERGE_TIMES 35\nint svo_surface_merge_timing\(svo_ctx \*ctx, float ms_out\[SVO_SURFACE_MERGE_TIMES\]\);", header)
    assert re.search(r"#define SVO_SURFACE_MERGE_ANY_VALUE\s+8u", header)
    assert len(pkg.Gpu.surface_merge_timing.__doc__) > 0
