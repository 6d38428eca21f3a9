"""The visible surface of a tree in the node buffer (csrc/svo_surface.hip), CPU side: the entry points are
exported and SurfaceParams has the header's layout; the sequential restatement (tests/surface_ref.py) against shifted
copies of a dense grid on uniform-depth trees, and on the listing tests' mixed-level tree; mesh.quads_to_mesh on CPU
tensors (outward normals, areas, exact vertices, a closed surface) and the .obj round trip."""
import ctypes as C
import os
import re

import numpy as np
import torch

import build_ref as B
import surface_ref as S
from conftest import ROOT as REPO
from test_list_host import mixed_levels

NEW = ("svo_nodes_list_surface", "svo_surface_timing")
AXES = np.eye(3, dtype=np.int64)


def ball(side, radius):
    """the filled ball about the grid's centre as a [x, y, z] grid of colours, 0 outside"""
    r = np.arange(side) - (side - 1) / 2
    inside = r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2 <= radius * radius
    x, y, z = np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij")
    return np.where(inside, 1 + ((x * 73 + y * 179 + z * 283) & 0xFFFF), 0).astype(np.int64)


def dense_masks(grid, closed):
    """per cell of a [x, y, z] occupancy the 6-bit mask of the faces with no occupied cell behind them; `closed`: the
    cells around the grid count as occupied"""
    g = np.pad(np.asarray(grid) != 0, 1, constant_values=closed)
    side = g.shape[0] - 2
    masks = np.zeros((side,) * 3, dtype=np.uint32)
    for f in range(6):
        lo = [1, 1, 1]
        lo[f >> 1] += 1 if f & 1 else -1
        behind = g[lo[0]:lo[0] + side, lo[1]:lo[1] + side, lo[2]:lo[2] + side]
        masks |= (~behind).astype(np.uint32) << np.uint32(f)
    return masks


def test_new_entry_points_are_exported_with_signatures(pkg):
    lib = pkg._lib.lib()
    for name in NEW:
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.svo_nodes_list_surface.argtypes) == 7 and len(lib.svo_surface_timing.argtypes) == 2
    assert callable(pkg.Render.list_surface) and callable(pkg.Render.surface_quads) and callable(pkg.Gpu.surface_timing)
    assert callable(pkg.mesh.quads_to_mesh) and callable(pkg.mesh.extract_surface) and callable(pkg.mesh.save_obj)


def test_surface_params_have_the_headers_layout(pkg):
    P = pkg._lib.SurfaceParams
    assert C.sizeof(P) == 24
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("flags", 0, 4), ("depth", 4, 4), ("n_words", 8, 8), ("max_entries", 16, 8)]
    header = open(os.path.join(REPO, "include", "svo_hip.h")).read()
    body = re.search(r"typedef struct svo_surface_params \{(.*?)\} svo_surface_params;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|uint64_t) (\w+);", body) == [("uint32_t", "flags"), ("uint32_t", "depth"), ("uint64_t", "n_words"),
                                                             ("uint64_t", "max_entries")]
    assert re.search(r"int svo_nodes_list_surface\(svo_ctx \*ctx, const svo_surface_params \*p, uint32_t \*xyz_out_dev, "
                     r"uint32_t \*value_out_dev,\s*uint32_t \*level_out_dev[^,]*, uint32_t \*face_out_dev,\s*uint64_t \*n_out\);", header)
    assert re.search(r"#define SVO_SURFACE_TIMES 7\nint svo_surface_timing\(svo_ctx \*ctx, float ms_out\[SVO_SURFACE_TIMES\]\);", header)
    for name, bit in (("CLOSED_BOUNDARY", S.CLOSED_BOUNDARY), ("KEEP_HIDDEN", S.KEEP_HIDDEN), ("QUADS", S.QUADS)):
        assert re.search(rf"#define SVO_SURFACE_{name}\s+{bit}u", header)


def test_the_reference_equals_shifted_copies_of_a_dense_grid():
    rng = np.random.default_rng(23)
    grid = np.where(rng.random((16, 16, 16)) < 0.6, rng.integers(1, 1 << 24, (16, 16, 16)), 0)
    coords, colours = B.dense_to_voxels(grid)
    words = B.build(coords, 4, colours)
    for closed in (False, True):
        xyz, value, level, masks = S.face_masks(words, words.size, 4, closed)
        want = dense_masks(grid, closed)
        assert value.size == len(coords) and (level == 4).all()
        assert np.array_equal(masks, want[tuple(xyz.T.astype(np.int64))])
        assert np.array_equal(value, grid[tuple(xyz.T.astype(np.int64))])
        assert (masks == 0).sum() > 20 and (masks != 0).sum() > 1000  # (a cell is hidden with probability 0.6^6: about 100 of them)
        # the three modes are views of those masks
        flag = S.CLOSED_BOUNDARY if closed else 0
        got = S.list_surface(words, words.size, 4, flag)
        assert np.array_equal(got[0], xyz[masks != 0]) and np.array_equal(got[3], masks[masks != 0])
        kept = S.list_surface(words, words.size, 4, flag | S.KEEP_HIDDEN)
        assert all(np.array_equal(a, b) for a, b in zip(kept, (xyz, value, level, masks)))
        quads = S.list_surface(words, words.size, 4, flag | S.QUADS)
        assert quads[3].size == sum(bin(int(m)).count("1") for m in masks) and quads[3].max() <= 5
        assert np.array_equal(quads[0][0], got[0][0]) and (np.diff(quads[3][:bin(int(got[3][0])).count("1")].astype(int)) > 0).all()
    for flags in (8, S.QUADS | S.KEEP_HIDDEN):
        try:
            S.list_surface(words, words.size, 4, flags)
            raise AssertionError("not refused")
        except ValueError:
            pass


def test_mixed_levels_coarse_leaves_cover_and_finer_detail_exposes():
    mixed = mixed_levels()
    xyz, value, level, masks = S.face_masks(mixed, mixed.size, 6)
    cells = {}  # (level, cell) -> entry
    for i in range(value.size):
        l = int(level[i])
        cells[(l, tuple(int(v) >> (6 - l) for v in xyz[i]))] = i
    covered_by_coarse = exposed_to_finer = 0
    for (l, cell), i in cells.items():
        for f in range(6):
            n = list(cell)
            n[f >> 1] += 1 if f & 1 else -1
            if not 0 <= n[f >> 1] < 1 << l:
                assert masks[i] >> f & 1
                continue
            # a leaf of a coarser level that contains the neighbour cell covers the face
            coarse = [k for k in range(1, l) if (k, tuple(v >> (l - k) for v in n)) in cells]
            if coarse:
                assert not masks[i] >> f & 1
                covered_by_coarse += 1
                # and that coarse leaf's face back towards this finer voxel is exposed
                k = coarse[0]
                back = cells[(k, tuple(v >> (l - k) for v in n))]
                behind = [v >> (l - k) for v in cell]
                if behind != [v >> (l - k) for v in n]:
                    assert masks[back] >> (f ^ 1) & 1
                    exposed_to_finer += 1
            elif (l, tuple(n)) in cells:
                assert not masks[i] >> f & 1
            elif l == 6:
                assert masks[i] >> f & 1  # nothing finer than depth: the cell is empty
    assert covered_by_coarse > 20 and exposed_to_finer > 20
    # counter bits change nothing
    counted = mixed | np.random.default_rng(3).integers(0, 16, mixed.size).astype(np.uint32)
    assert np.array_equal(S.face_masks(counted, mixed.size, 6)[3], masks)
    # on the depth-8 grid the masks are the same, the corners scaled
    again = S.face_masks(mixed, mixed.size, 8)
    assert np.array_equal(again[3], masks) and np.array_equal(again[0], xyz << 2)


def solid_quads(depth=3):
    """the quads of a random uniform-depth solid, from the reference"""
    rng = np.random.default_rng(9)
    side = 1 << depth
    grid = np.where(rng.random((side,) * 3) < 0.5, 7, 0)
    coords, colours = B.dense_to_voxels(grid)
    words = B.build(coords, depth, colours)
    return S.list_surface(words, words.size, depth, S.QUADS)


def test_quads_to_mesh_on_cpu_tensors(pkg):
    M = pkg.mesh
    # mixed levels: normals, areas, vertices
    mixed = mixed_levels()
    xyz, value, level, face = S.list_surface(mixed, mixed.size, 6, S.QUADS)
    args = [torch.from_numpy(a.astype(np.int32)) for a in (xyz, face, level)]
    for weld in (True, False):
        vi, tri, col = M.quads_to_mesh(*args, 6, torch.from_numpy(value.astype(np.int32)), weld=weld, integer=True)
        vf, tri_f, _ = M.quads_to_mesh(*args, 6, weld=weld)
        assert vi.dtype == torch.int32 and vf.dtype == torch.float32 and tri.dtype == torch.int32 and torch.equal(tri, tri_f)
        assert tri.shape == (2 * face.size, 3) and np.array_equal(col.numpy(), np.repeat(value.astype(np.int32), 2))
        v, t = vi.numpy().astype(np.int64), tri.numpy().astype(np.int64)
        a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
        normal = np.cross(b - a, c - a)
        f2, s2 = np.repeat(face.astype(np.int64), 2), np.repeat((1 << (6 - level.astype(np.int64))) ** 2, 2)
        want = AXES[f2 >> 1] * np.where(f2 & 1, 1, -1)[:, None] * s2[:, None]  # twice the area s^2 / 2, along the outward axis
        assert np.array_equal(normal, want)
        # the plane and the extent of every quad
        q = v[t.reshape(-1, 2, 3)[:, :, :].reshape(-1, 6)]  # (Q, 6, 3)
        side = 1 << (6 - level.astype(np.int64))
        lo = xyz.astype(np.int64).copy()
        lo[np.arange(face.size), face >> 1] += (face & 1) * side
        hi = xyz.astype(np.int64) + side[:, None]
        hi[np.arange(face.size), face >> 1] = lo[np.arange(face.size), face >> 1]
        assert np.array_equal(q.min(axis=1), lo) and np.array_equal(q.max(axis=1), hi)
        assert np.array_equal(vf.numpy(), (v.astype(np.float64) / 64 * 2 - 1).astype(np.float32))
        assert np.array_equal(vf.numpy().astype(np.float64), v / 32 - 1)  # exact
        if weld:
            assert len(np.unique(v, axis=0)) == len(v) and (np.diff(v[:, 0]) >= 0).all()
        else:
            assert len(v) == 4 * face.size
    # depth 21: the float vertices are still exact
    vf, _, _ = M.quads_to_mesh(torch.tensor([[(1 << 21) - 1, 0, 12345]]), torch.tensor([1]), torch.tensor([21]), 21)
    assert np.array_equal(vf.numpy().astype(np.float64)[:, 0], np.full(4, 1.0)) and vf.numpy()[0, 2] == np.float32(12345 / (1 << 20) - 1)
    # a uniform-depth solid: every welded edge is used by an even number of quads
    xyz, value, level, face = solid_quads()
    _, tri, _ = M.quads_to_mesh(*[torch.from_numpy(a.astype(np.int32)) for a in (xyz, face, level)], 3, integer=True)
    corner = tri.numpy().astype(np.int64).reshape(-1, 6)[:, [0, 1, 2, 5]]  # the quad's corners 0, 1, 2, 3
    ends = np.sort(np.stack([corner, np.roll(corner, -1, axis=1)], axis=-1).reshape(-1, 2), axis=1)
    _, uses = np.unique(ends, axis=0, return_counts=True)
    assert uses.size > 100 and (uses % 2 == 0).all()
    # no quads: an empty mesh
    none = torch.zeros((0, 3), dtype=torch.int32)
    v, t, c = M.quads_to_mesh(none, none[:, 0], none[:, 0], 5)
    assert v.shape == (0, 3) and t.shape == (0, 3) and c is None


def test_obj_round_trip_is_bit_exact(pkg, tmp_path):
    M = pkg.mesh
    xyz, value, level, face = solid_quads()
    v, t, _ = M.quads_to_mesh(*[torch.from_numpy(a.astype(np.int32)) for a in (xyz, face, level)], 3)
    rng = np.random.default_rng(1)
    awkward = rng.standard_normal((len(v), 3)).astype(np.float32) * np.float32(1e-3)  # floats with long decimal forms
    rgb = rng.random((len(v), 3)).astype(np.float32)
    for name, vertices, colours in (("grid", v, None), ("awkward", awkward, rgb), ("tensor rgb", v, torch.from_numpy(rgb))):
        path = str(tmp_path / f"{name.replace(' ', '_')}.obj")
        M.save_obj(path, vertices, t, colours)
        got_v, got_t, got_rgb = M.load_obj(path)
        want = np.asarray(vertices, dtype=np.float32)
        assert got_v.dtype == np.float32 and got_v.tobytes() == want.tobytes(), name
        assert got_t.dtype == np.int32 and np.array_equal(got_t, t.numpy()), name
        assert (got_rgb is None) if colours is None else got_rgb.tobytes() == np.asarray(colours, dtype=np.float32).tobytes(), name
