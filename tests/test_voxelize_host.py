"""Mesh voxelisation (csrc/svo_voxelize.hip), CPU side: the entry points are exported with signatures and
declared in the header; the integer 13-axis test equals exact clipping in fractions (tests/voxelize_ref.py) on random
and degenerate triangles at every level's cell size, and the level refinement equals brute force over every cell on whole
small meshes; the widest arithmetic of depth 21 stays inside the widths the kernel uses; the order rule; the host helpers
of mesh.py (quantize_vertices, load_obj, fit_to_cube, the generators)."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import build_ref as B
import voxelize_ref as V
from conftest import GOLDEN, ROOT as REPO

NEW = ("svo_mesh_voxelize", "svo_voxelize_timing")


def random_mesh(seed, depth, n_tris, n_vertices=40, extent=None):
    """(vq, triangles, colours): random triangles over the whole grid (or, with extent, no longer than `extent` quantised
    steps per axis) with the degenerate kinds in front: three collinear vertices, two equal vertices, three equal vertices,
    a triangle in an axis plane"""
    rng = np.random.default_rng(seed)
    top = 1 << (depth + V.SUBBITS)
    vq = rng.integers(0, top, (n_vertices, 3))
    if extent is not None:
        corner = rng.integers(0, top - extent, (n_vertices // 3 + 1, 1, 3))
        vq = (corner + rng.integers(0, extent, (n_vertices // 3 + 1, 3, 3))).reshape(-1, 3)[:n_vertices]
        tris = (3 * rng.integers(0, n_vertices // 3, (n_tris, 1)) + np.arange(3)).reshape(-1, 3)
    else:
        tris = rng.integers(0, n_vertices, (n_tris, 3))
    half = np.sign(vq[2] - vq[0]) * (np.abs(vq[2] - vq[0]) // 2)
    vq[1], vq[2] = vq[0] + half, vq[0] + 2 * half  # vertex 1 is the midpoint of 0 and 2
    vq[5, 0] = vq[4, 0] = vq[3, 0]  # an x plane
    tris[0] = [0, 1, 2]
    tris[1] = [6, 7, 7]
    tris[2] = [8, 8, 8]
    tris[3] = [3, 4, 5]
    return vq, tris, rng.integers(1, 1 << 24, n_tris)


def planar_quad(depth):
    """(vq, triangles): a quad in the plane y = 2 cells exactly (q a multiple of 64) spanning cells 1..3 in x and z"""
    q = [[64, 128, 64], [64 * 3 + 32, 128, 64], [64 * 3 + 32, 128, 64 * 3 + 32], [64, 128, 64 * 3 + 32]]
    return np.array(q, dtype=np.int64), np.array([[0, 1, 2], [0, 2, 3]])


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_mesh_voxelize.argtypes) == 10 and len(lib.svo_voxelize_timing.argtypes) == 2
    assert pkg.mesh is not None and "mesh" in pkg.__all__
    for name in ("quantize_vertices", "voxelize", "load_obj", "fit_to_cube", "icosphere", "torus"):
        assert callable(getattr(pkg.mesh, name)), name
    assert callable(pkg.Render.build_nodes_mesh) and callable(pkg.Render.from_mesh) and callable(pkg.Gpu.voxelize_timing)
    assert pkg.mesh.SUBBITS == V.SUBBITS == 6


def test_params_have_the_headers_layout_and_the_header_declares_the_functions(pkg):
    P = pkg._lib.VoxelizeParams
    assert C.sizeof(P) == 24
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("depth", 0, 4), ("flags", 4, 4), ("default_colour", 8, 4), ("n_vertices", 12, 4), ("max_voxels", 16, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    assert "triangle meshes voxelised on the GPU (DESIGN.md 20)" in header
    body = re.search(r"typedef struct svo_voxelize_params \{(.*?)\} svo_voxelize_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [("uint32_t", "depth"), ("uint32_t", "flags"), ("uint32_t", "default_colour"),
                                                              ("uint32_t", "n_vertices"), ("uint64_t", "max_voxels")]
    assert re.search(r"#define SVO_VOX_SUBBITS 6\b", header)
    assert re.search(r"int svo_mesh_voxelize\(svo_ctx \*ctx, const svo_voxelize_params \*p,", header)
    assert re.search(r"#define SVO_VOXELIZE_TIMES \d+\nint svo_voxelize_timing\(svo_ctx \*ctx, float ms_out\[SVO_VOXELIZE_TIMES\]\);", header)
    assert "HIGHEST TRIANGLE INDEX COLOURS A" in header


def random_case(rng, S):
    """a triangle of odd coordinates near a box of side S with even bounds; kind: 0 collinear (unless cut at the grid's
    faces), 1 two equal vertices, 2 a point, 3 in an axis plane, else general"""
    grid = 1 << 28  # the doubled coordinates of depth 21: everything stays inside
    lo = [rng.randrange(0, min(6, grid // S)) * S for _ in range(3)]
    span = rng.choice((S // 8, S, 4 * S))

    def point():
        return [min(grid - 1, max(1, lo[a] + S // 2 + 2 * rng.randrange(-span, span) + 1)) for a in range(3)]

    a, b, c = point(), point(), point()
    kind = rng.randrange(8)
    if kind == 0:
        c = [min(grid - 1, max(1, a[i] + 2 * (b[i] - a[i]))) for i in range(3)]
    elif kind == 1:
        c = list(b)
    elif kind == 2:
        b, c = list(a), list(a)
    elif kind == 3:
        axis = rng.randrange(3)
        b[axis] = c[axis] = a[axis]
    return [a, b, c], lo, kind


def test_the_integer_test_equals_exact_clipping_at_every_level_size():
    rng = random.Random(20)
    total = hits = 0
    kinds = {}
    for level_bits in range(7, 28):  # S = 2^(depth - l + 7): 2^7 at the leaves, 2^27 at level 1 of depth 21
        S = 1 << level_bits
        cases = [random_case(rng, S) for _ in range(150)]
        many = V.overlaps_many(np.array([c[0] for c in cases]), np.array([c[1] for c in cases]), S)
        for (tri, lo, kind), m in zip(cases, many):
            want = V.overlaps_by_clipping(tri, lo, S)
            assert V.overlaps(tri, lo, S) == want == bool(m), (tri, lo, S)
            assert all(x % 2 == 1 for p in tri for x in p)
            total, hits = total + 1, hits + want
            kinds[kind] = kinds.get(kind, 0) + want
    assert total == 3150 and hits > 400 and all(kinds.get(k, 0) > 10 for k in range(4)), (hits, kinds)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_the_refinement_equals_brute_force_over_every_cell(depth):
    vq, tris, colours = random_mesh(depth, depth, 10, n_vertices=12)
    quad = planar_quad(depth) if depth >= 2 else None
    if quad is not None:
        tris = np.concatenate([tris, quad[1] + len(vq)])
        vq = np.concatenate([vq, quad[0]])
        colours = np.concatenate([colours, [5, 6]])
    xyz, colour, tri = V.voxelize(vq, tris, depth, colours)
    got = [(int(t), *c.tolist()) for t, c in zip(tri, xyz)]
    assert got == V.voxelize_brute(vq, tris, depth, V.overlaps)
    assert got == V.voxelize_brute(vq, tris, depth, V.overlaps_by_clipping)
    assert np.array_equal(colour, (colours & 0xFFFFFF)[tri])
    assert len(set(t for t, *_ in got)) == len(tris)  # every triangle, the degenerate ones too, has a cell
    if quad is not None:  # a wall on a grid plane is one cell thick: it falls into the cells above the plane
        wall = xyz[tri >= len(tris) - 2]
        assert len(wall) and (wall[:, 1] == 2).all()


def test_depth_21_corner_to_corner_stays_inside_the_widths():
    top = (1 << 27) - 1
    vq = [[0, 0, 0], [top, top, top], [top, top, top - 1], [0, top, 0], [top, 0, top]]
    stats, levels = {}, []
    stopped = V.voxelize(vq, [[0, 1, 2], [0, 1, 3], [3, 4, 0]], 21, cap=0, stats=stats, levels=levels)
    assert stopped == V.Stopped(1, levels[0]) and levels[0] >= 3 * 2
    assert 56 <= stats["edge_bits"] <= 62, stats        # int64, as the kernel computes them
    assert 64 < stats["plane_bits"] <= 127, stats       # past int64: the plane test is the kernel's 128-bit part
    # the pair counts never decrease, and a cap stops at the first level that passes it
    levels = []
    stopped = V.voxelize(vq, [[0, 1, 2]], 21, cap=4096, levels=levels)
    assert stopped.level == len(levels) and stopped.count == levels[-1] > 4096
    assert all(a <= b for a, b in zip(levels, levels[1:])) and all(n <= 4096 for n in levels[:-1])


def test_the_order_rule():
    vq, tris, colours = random_mesh(44, 4, 30)
    xyz, colour, tri = V.voxelize(vq, tris, 4, colours)
    assert (np.diff(tri.astype(np.int64)) >= 0).all() and set(tri.tolist()) == set(range(30))
    key = B.morton(xyz, 4).astype(np.int64)
    same = np.diff(tri.astype(np.int64)) == 0
    assert (np.diff(key)[same] > 0).all()  # strictly: a cell appears once per triangle
    cells = {}
    for t, c in zip(tri.tolist(), map(tuple, xyz.tolist())):
        cells.setdefault(c, []).append(t)
    assert any(len(ts) > 1 for ts in cells.values())  # shared cells appear once per triangle


def test_quantize_vertices(pkg):
    import torch
    q = pkg.mesh.quantize_vertices
    for depth in (1, 7, 21):
        top = 1 << (depth + 6)
        below_one = np.nextafter(np.float32(1), np.float32(0))
        got = q(np.array([[-1.0, 0.0, below_one]], dtype=np.float32), depth)
        assert got.dtype == np.int64 and got.tolist() == [[0, top // 2, min(top - 1, int((float(below_one) + 1.0) * (top // 2)))]]
        assert q(np.array([[1.0 - 2.0 ** -30] * 3]), depth).tolist() == [[top - 1] * 3]
        cell = 2.0 / (1 << depth)  # a vertex at a cell's world corner gets q = 64 * cell
        assert q(np.array([[-1.0 + cell, -1.0 + 1.5 * cell, 1.0 - cell]]), depth).tolist() == [[64, 96, top - 64]]
        # (the float64 next to 1 is refused too: v + 1 rounds to 2, the far face)
        for bad in (1.0, np.nextafter(1.0, 0.0), -1.0000001, 2.5, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                q(np.array([[0.0, bad, 0.0]]), depth)
    t = q(torch.tensor([[-1.0, 0.25, 0.5]]), 3)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.tolist() == [[0, 320, 384]]
    with pytest.raises(ValueError):
        q(torch.tensor([[1.0, 0.0, 0.0]]), 3)
    for depth in (0, 22):
        with pytest.raises(ValueError):
            q(np.zeros((1, 3)), depth)
    assert q(np.zeros((0, 3)), 5).shape == (0, 3)


def test_load_obj_reads_the_cube_of_quads(pkg, tmp_path):
    vertices, triangles, rgb = pkg.mesh.load_obj(os.path.join(GOLDEN, "cube_quads.obj"))
    assert vertices.dtype == np.float32 and vertices.shape == (8, 3) and triangles.dtype == np.int32 and triangles.shape == (12, 3)
    assert rgb is None and vertices[0].tolist() == [-0.5, -0.5, -0.5] and vertices[6].tolist() == [0.5, 0.5, 0.5]
    assert triangles.tolist() == [[0, 3, 2], [0, 2, 1], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [3, 7, 6], [3, 6, 2],
                                  [0, 4, 7], [0, 7, 3], [1, 2, 6], [1, 6, 5]]
    # every face of the cube is covered: per axis and side, two triangles lie in that plane
    for axis in range(3):
        for side in (-0.5, 0.5):
            assert sum(bool((vertices[t][:, axis] == side).all()) for t in triangles) == 2
    path = tmp_path / "coloured.obj"
    path.write_text("v 0 0 0 1 0 0\nv 1 0 0 0 1 0\nv 0 1 0 0 0 1\nv 1 1 0 0.5 0.5 0.5\nvn 0 0 1\nf 1 2 4 3 # a quad\nf -1//1 -2//1 -4//1\n")
    vertices, triangles, rgb = pkg.mesh.load_obj(str(path))
    assert triangles.tolist() == [[0, 1, 3], [0, 3, 2], [3, 2, 0]] and rgb.shape == (4, 3) and rgb[3].tolist() == [0.5, 0.5, 0.5]
    path.write_text("v 0 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        pkg.mesh.load_obj(str(path))


def test_generators_and_fit_to_cube(pkg):
    M = pkg.mesh
    for s, n_t, n_v in ((0, 20, 12), (1, 80, 42), (2, 320, 162)):
        v, t = M.icosphere(s, 0.7, (0.1, 0.0, -0.1))
        assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == (n_v, 3) and t.shape == (n_t, 3)
        assert np.allclose(np.linalg.norm(v - np.array([0.1, 0.0, -0.1], dtype=np.float32), axis=1), 0.7, atol=1e-6)
        assert sorted(set(t.reshape(-1).tolist())) == list(range(n_v))
        edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
        assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()  # closed: every edge has two triangles
    again = M.icosphere(2, 0.7, (0.1, 0.0, -0.1))
    assert again[0].tobytes() == v.tobytes() and again[1].tobytes() == t.tobytes()
    v, t = M.torus(10, 6, 0.5, 0.2)
    assert v.shape == (60, 3) and t.shape == (120, 3) and v.dtype == np.float32 and t.dtype == np.int32
    edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()
    assert np.allclose(np.hypot(np.hypot(v[:, 0], v[:, 2]) - 0.5, v[:, 1]), 0.2, atol=1e-6)
    f = M.fit_to_cube(np.array([[10.0, 0.0, 0.0], [14.0, 1.0, 2.0]], dtype=np.float32), margin=0.25)
    assert f.dtype == np.float32 and np.allclose(f, [[-0.75, -0.1875, -0.375], [0.75, 0.1875, 0.375]])
    assert float(np.abs(M.fit_to_cube(M.torus()[0] * 100)).max()) <= 0.98 + 1e-6
    M.quantize_vertices(M.fit_to_cube(M.icosphere(1)[0], 0.0) * np.float32(0.999), 21)
