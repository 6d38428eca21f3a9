"""Solid voxelisation (csrc/svo_solid.hip), CPU side: the contract's tie rule against a real generic point
in fractions; the 2D level refinement against brute force over every square and column; boxes, closed meshes, both
rules, the triangles' order, the seal against the surface voxeliser; the widths of depth 21; the ABI's text and symbols."""
import ctypes as C
import inspect
import os
import random
import re

import numpy as np
import pytest

import solid_ref as S
import voxelize_ref as V
from conftest import ROOT as REPO

NEW = ("svo_mesh_voxelize_solid", "svo_solid_timing")
RULES = (S.EVENODD, S.NONZERO)

# ---- meshes (quantised vertices q: the doubled coordinate is 2 q + 1) ----


def box_mesh(lo, hi):
    """(vq, triangles): the box [lo, hi] in quantised coordinates, 12 triangles whose normals point outwards"""
    corner = lambda bits: [hi[a] if bits >> (2 - a) & 1 else lo[a] for a in range(3)]  # noqa: E731
    tris = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            quad = [side << (2 - a) | cu << (2 - u) | cv << (2 - v) for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1))]
            quad = quad if side else quad[::-1]
            tris += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.array([corner(b) for b in range(8)], dtype=np.int64), np.array(tris, dtype=np.int64)


def join(*meshes):
    vq, tris, base = [], [], 0
    for v, t in meshes:
        vq.append(np.asarray(v, dtype=np.int64).reshape(-1, 3))
        tris.append(np.asarray(t, dtype=np.int64).reshape(-1, 3) + base)
        base += len(vq[-1])
    return np.concatenate(vq), np.concatenate(tris)


TETRA = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def tetra_soup(seed, depth, n):
    """n random tetrahedra over the whole grid, each a closed surface of one orientation"""
    rng = np.random.default_rng(seed)
    vq = rng.integers(0, 1 << (depth + S.SUBBITS), (4 * n, 3))
    return vq, (TETRA[None] + 4 * np.arange(n)[:, None, None]).reshape(-1, 3)


def cell_tetrahedra(seed, depth, n):
    """n tetrahedra, each inside one cell of its own and around that cell's centre; returns (vq, triangles, cells)"""
    rng = np.random.default_rng(seed)
    side = 1 << depth
    i = np.arange(n)
    cells = np.stack([i % side, i // side % side, i // (side * side)], axis=1)
    assert n <= side ** 3
    shape = np.array([[4, 6, 5], [60, 8, 9], [30, 7, 61], [31, 60, 33]])
    vq = cells[:, None, :] * 64 + shape[None] + rng.integers(-3, 4, (n, 4, 3))
    return vq.reshape(-1, 3), (TETRA[None] + 4 * i[:, None, None]).reshape(-1, 3), cells


def tie_mesh(depth):
    """designed ties on the 2^depth grid (depth >= 1): a quad split along the diagonal x = z, whose shared edge's projection
    runs through cell centres from (1, ., 1) to the far corner; a triangle in the plane y = x, which passes through the
    centres (c, c, .); triangles with axis-parallel edges; edge-on triangles (a vertical one, a segment, a point)"""
    top = (1 << (depth + S.SUBBITS)) - 1  # q: the doubled coordinate is 2 top + 1 = 2^(depth + 7) - 1
    half = top // 2 + 1                   # q = 2^(depth + 5): doubled 2^(depth + 6) + 1
    vq = [[0, 5, 0], [top, 9, top], [top, 7, 0], [0, 11, top],              # 0-3: the quad, diagonal 0-1
          [0, 0, 0], [top, top, 0], [half, half, top],                      # 4-6: in the plane y = x
          [3, 40, 3], [top - 3, 44, 3], [3, 50, top - 3],                   # 7-9: edges parallel to x and z
          [0, 0, 0], [top, 0, top], [half, top, half], [9, 9, 9], [70, 9, 9]]  # 10-14: edge-on
    tris = [[0, 1, 2], [0, 3, 1], [4, 5, 6], [7, 8, 9], [9, 8, 7], [10, 11, 12], [13, 14, 14], [13, 13, 13]]
    return np.array(vq, dtype=np.int64), np.array(tris, dtype=np.int64)


def as_set(cells):
    return set(map(tuple, np.asarray(cells).tolist()))


# ---- the tie rule ----
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_the_tie_rule_is_a_generic_point(depth):
    rng = np.random.default_rng(depth)
    top = 1 << (depth + S.SUBBITS)
    vq = rng.integers(0, top, (3 * 8, 3))
    vq[:, 1] = rng.integers(0, top, len(vq))
    # vertices on the centres' own lines as often as chance never gives: q with 2 q + 1 next to a centre
    vq[::4, 0] = 64 * rng.integers(0, 1 << depth, len(vq[::4])) + 32
    random_tris = np.arange(24).reshape(8, 3)
    for vq, tris in ((vq, random_tris), tie_mesh(depth), join((vq, random_tris), tie_mesh(depth), tetra_soup(depth, depth, 3))):
        for rule in RULES:
            want = S.cells_brute(vq, tris, depth, rule, by=S.inside_by_fractions)
            assert S.cells_brute(vq, tris, depth, rule) == want
            got = S.solid(vq, tris, depth, rule)
            assert as_set(got.cells) == want and len(got.cells) == len(want)


def test_the_designed_ties_are_ties():
    vq, tris = tie_mesh(2)
    Vs = S.doubled(vq, tris).tolist()
    # the diagonal's edge function is zero at the centres (c, c), and exactly one of the quad's two triangles covers each
    for c in range(4):
        ex, ez = Vs[0][1][0] - Vs[0][0][0], Vs[0][1][2] - Vs[0][0][2]
        assert ex * (128 * c + 64 - Vs[0][0][2]) - ez * (128 * c + 64 - Vs[0][0][0]) == 0
        assert S.covers(Vs[0], c, c) + S.covers(Vs[1], c, c) == 1
    # the plane y = x holds the centres (c, c, cz): a centre on the plane is above it, so k = c there, not c + 1
    n = S.normal(Vs[2])
    assert n[1] != 0 and sum(n[a] * (128 * 1 + 64 - Vs[2][0][a]) for a in range(3)) == 0
    assert S.covers(Vs[2], 1, 1) and S.height(Vs[2], 1, 1, 2) == 1 == S.height_closed_form(Vs[2], 1, 1, 2)
    # two triangles of opposite orientation over the same ground cancel; edge-on triangles cover nothing
    assert all(S.normal(Vs[k])[1] == 0 and not any(S.covers(Vs[k], x, z) for x in range(4) for z in range(4)) for k in (5, 6, 7))
    got = S.solid(vq, tris, 2, S.NONZERO)
    assert got.n_open > 0  # (it is no closed mesh)


def test_height_closed_form_equals_the_sign_test():
    rng = random.Random(5)
    for depth in (1, 2, 3, 5):
        top = 1 << (depth + S.SUBBITS)
        for _ in range(60):
            Vt = [[2 * rng.randrange(top) + 1 for _ in range(3)] for _ in range(3)]
            if S.normal(Vt)[1] == 0:
                continue
            cx, cz = rng.randrange(1 << depth), rng.randrange(1 << depth)
            assert S.height(Vt, cx, cz, depth) == S.height_closed_form(Vt, cx, cz, depth)


# ---- the level refinement ----
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_the_refinement_equals_brute_force_over_every_square(depth):
    vq, tris = join(tetra_soup(10 + depth, depth, 3), tie_mesh(depth), cell_tetrahedra(depth, depth, 2)[:2])
    Vd = S.doubled(vq, tris)
    levels = []
    t, col = S.refine(Vd, depth, levels=levels)
    Vs = Vd.tolist()
    live = [V3 for V3 in Vs if S.normal(V3)[1] != 0]
    assert 0 < len(live) < len(Vs)
    for level in range(1, depth):
        side = 1 << (depth - level + 7)
        count = 0
        for V3 in live:
            flat = [[p[0], 1, p[2]] for p in V3]
            for x in range(1 << level):
                for z in range(1 << level):
                    want = V.overlaps_by_clipping(flat, [x * side, 0, z * side], side)
                    assert S.square_overlaps(V3, (x * side, z * side), side) == want
                    count += want
        assert levels[level - 1] == count
    want = sorted((k, x, z) for k, V3 in enumerate(Vs) for x in range(1 << depth) for z in range(1 << depth) if S.covers(V3, x, z))
    assert sorted(zip(t.tolist(), col[:, 0].tolist(), col[:, 1].tolist())) == want and levels[-1] == len(want)
    assert all(a <= b for a, b in zip(levels[:-1], levels[1:-1]))  # below the last level the counts never fall
    stopped = S.solid(vq, tris, depth, max_pairs=levels[0] - 1)
    assert stopped == S.Stopped(1, levels[0])


# ---- whole meshes ----
def test_a_box_on_grid_planes_is_the_cells_between_its_faces():
    lo, hi = (1, 2, 0), (6, 5, 8)
    vq, tris = box_mesh([64 * c for c in lo], [64 * c - (c == 8) for c in hi])  # (the far face at the grid's last quantum)
    for rule in RULES:
        got = S.solid(vq, tris, 3, rule)
        want = {(x, y, z) for x in range(lo[0], hi[0]) for y in range(lo[1], hi[1]) for z in range(lo[2], hi[2])}
        assert as_set(got.cells) == want and got.n_open == 0
        assert got.spans.tolist() == [[x, z, lo[1], hi[1]] for x in range(lo[0], hi[0]) for z in range(lo[2], hi[2])]
        assert got.cells.tolist() == sorted(got.cells.tolist(), key=lambda c: (c[0], c[2], c[1]))


@pytest.fixture(scope="module")
def closed4(pkg):
    """closed meshes at depth 4: (vq, triangles) by name"""
    out = {"soup": tetra_soup(4, 4, 50)}
    for name, (v, t) in (("icosphere", pkg.mesh.icosphere(2, 0.7, (0.05, -0.1, 0.1))), ("torus", pkg.mesh.torus(16, 8, 0.55, 0.25, (0.0, 0.1, 0.0)))):
        out[name] = (pkg.mesh.quantize_vertices(v, 4), t.astype(np.int64))
    return out


@pytest.mark.parametrize("name", ["icosphere", "torus", "soup"])
def test_closed_meshes_have_no_open_column_and_ignore_order_and_flips(closed4, name):
    vq, tris = closed4[name]
    rng = np.random.default_rng(1)
    want = {rule: S.solid(vq, tris, 4, rule) for rule in RULES}
    assert all(w.n_open == 0 and len(w.cells) > 20 for w in want.values())
    if name != "soup":  # one surface, consistently oriented: the two rules agree
        assert np.array_equal(want[S.EVENODD].cells, want[S.NONZERO].cells)
    shuffled = tris[rng.permutation(len(tris))]
    for rule in RULES:
        got = S.solid(vq, shuffled, 4, rule)
        assert np.array_equal(got.spans, want[rule].spans) and np.array_equal(got.cells, want[rule].cells) and got.n_open == 0
    flipped = tris.copy()
    which = rng.random(len(tris)) < 0.5
    flipped[which] = flipped[which][:, ::-1]
    got = S.solid(vq, flipped, 4, S.EVENODD)
    assert np.array_equal(got.cells, want[S.EVENODD].cells) and got.n_open == 0


def test_two_overlapping_boxes_union_and_symmetric_difference():
    a, b = ((64, 70, 80), (400, 300, 500)), ((200, 130, 100), (700, 600, 420))
    vq, tris = join(box_mesh(*a), box_mesh(*b))
    cells = [as_set(S.solid(*box_mesh(*box), 4).cells) for box in (a, b)]
    assert cells[0] & cells[1] and cells[0] - cells[1] and cells[1] - cells[0]
    assert as_set(S.solid(vq, tris, 4, S.NONZERO).cells) == cells[0] | cells[1]
    assert as_set(S.solid(vq, tris, 4, S.EVENODD).cells) == cells[0] ^ cells[1]
    assert S.solid(vq, tris, 4, S.NONZERO).n_open == S.solid(vq, tris, 4, S.EVENODD).n_open == 0


def test_the_seal(pkg):
    """of two face-adjacent cells, one inside and one outside, the surface voxeliser lists at least one"""
    for v, t in (pkg.mesh.icosphere(2, 0.7, (0.05, -0.1, 0.1)), pkg.mesh.torus(24, 12, 0.55, 0.25, (0.0, 0.1, 0.0))):
        vq = pkg.mesh.quantize_vertices(v, 5)
        inside = np.zeros((34, 34, 34), dtype=bool)
        cells = S.solid(vq, t, 5).cells.astype(np.int64)
        inside[cells[:, 0] + 1, cells[:, 1] + 1, cells[:, 2] + 1] = True
        shell = np.zeros_like(inside)
        surface = V.voxelize(vq, t, 5)[0].astype(np.int64)
        shell[surface[:, 0] + 1, surface[:, 1] + 1, surface[:, 2] + 1] = True
        assert len(cells) > 1000 and not inside[0].any() and not inside[-1].any()
        for axis in range(3):
            lo = [np.take(m, range(1, 32), axis=axis) for m in (inside, shell)]  # the grid's cells 0..30 along the axis
            hi = [np.take(m, range(2, 33), axis=axis) for m in (inside, shell)]  # and their neighbours 1..31
            boundary = lo[0] != hi[0]
            assert boundary.any() and (lo[1] | hi[1])[boundary].all()


def test_depth_21_corner_to_corner_stays_inside_the_widths():
    top = (1 << 27) - 1
    Vt = [[1, 1, 1], [2 * top + 1, 2 * top + 1, 1], [1, 2 * top + 1, 2 * top + 1]]
    n = S.normal(Vt)
    assert all(abs(x) < 1 << 57 for x in n) and n[1] != 0
    last = (1 << 21) - 1
    for cx, cz in ((0, 0), (last, 0), (0, last), (last, last), (12345, 54321)):
        a = n[0] * (128 * cx + 64 - Vt[0][0]) + n[2] * (128 * cz + 64 - Vt[0][2])
        D = [a + n[1] * (128 * cy + 64 - Vt[0][1]) for cy in (0, last)]
        assert all(abs(d) < 1 << 87 for d in D) and max(abs(d) for d in D) > 1 << 64  # past int64, inside 128 bits
        k = S.height_closed_form(Vt, cx, cz, 21)
        assert 0 <= k <= 1 << 21
        # the sign test on both sides of k
        above = lambda cy: (d := a + n[1] * (128 * cy + 64 - Vt[0][1])) != 0 and S.sign(d) != S.sign(n[1])  # noqa: E731
        assert (k == 0 or above(k - 1)) and (k == 1 << 21 or not above(k))
        key = ((cx << 21 | cz) << 22) | k
        assert key < 1 << 64
    assert (((last << 21 | last) << 22) | (1 << 21)).bit_length() == 64  # the key fills 64 bits at depth 21 exactly


# ---- the ABI ----
def test_the_abi(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_mesh_voxelize_solid.argtypes) == 8 and len(lib.svo_solid_timing.argtypes) == 2
    P = pkg._lib.SolidParams
    assert C.sizeof(P) == 32
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("depth", 0, 4), ("flags", 4, 4), ("n_vertices", 8, 4), ("reserved", 12, 4), ("max_out", 16, 8), ("max_pairs", 24, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    assert "closed meshes voxelised solid on the GPU (DESIGN.md 24)" in header
    body = re.search(r"typedef struct svo_solid_params \{(.*?)\} svo_solid_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [("uint32_t", "depth"), ("uint32_t", "flags"), ("uint32_t", "n_vertices"),
                                                              ("uint32_t", "reserved"), ("uint64_t", "max_out"), ("uint64_t", "max_pairs")]
    for name, value in (("EVENODD", 0), ("NONZERO", 1), ("SPANS", 2)):
        assert re.search(rf"#define SVO_SOLID_{name}\s+{value}u\b", header)
    assert re.search(r"int svo_mesh_voxelize_solid\(svo_ctx \*ctx, const svo_solid_params \*p, const uint32_t \*vq_dev,", header)
    assert re.search(r"#define SVO_SOLID_TIMES 6\b.*\nint svo_solid_timing\(svo_ctx \*ctx, float ms_out\[SVO_SOLID_TIMES\]\);", header)
    assert "svo_mesh_voxelize_solid" in open(os.path.join(REPO, "include", "svo_render.hpp")).read()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "svo_mesh_voxelize_solid" in integration and "SvoSolidParams" in integration and "svo_solid_timing" in integration
    assert (pkg.mesh.SOLID_RULES, pkg.mesh.SOLID_SPANS) == ({"evenodd": S.EVENODD, "nonzero": S.NONZERO}, S.SPANS)
    assert callable(pkg.mesh.voxelize_solid) and callable(pkg.Gpu.solid_timing)
    for fn in (pkg.Render.from_mesh, pkg.Render.build_nodes_mesh):
        args = inspect.signature(fn).parameters
        assert [args[k].default for k in ("solid", "fill_colour", "rule", "allow_open")] == [False, None, "evenodd", False]
    # no context: refused before anything is looked at
    assert lib.svo_mesh_voxelize_solid(None, None, None, None, 0, None, None, None) == -1
