"""Triangle meshes on their way into the node buffer (no reference counterpart): the GPU voxeliser behind
svo_mesh_voxelize, the quantisation it works on, a minimal Wavefront reader and two deterministic mesh generators.

    quantize_vertices  world coordinates in [-1, 1) -> the voxeliser's integer coordinates, 64 per cell
    voxelize           mesh -> device voxel list (coords, colours[, triangles]) for build_nodes, edit_nodes, CpuOctree.build
                       and World.build_world: one entry per (triangle, cell) that meet, triangles in order, cells in
                       Morton order; the highest triangle index colours a shared cell
    voxelize_solid     closed mesh -> the device list of the cells inside it, or their y-spans: with
                       voxelize's list behind it, a solid model with its surface's colours (Render.from_mesh(solid=True))
    quads_to_mesh      the exposed faces of a tree (Render.surface_quads) -> an indexed triangle mesh
    rects_to_mesh      the same faces merged into rectangles (Render.surface_rects) -> an indexed triangle mesh
    extract_surface    quads or rectangles and their mesh in one call: the inverse of voxelize
    load_obj, save_obj v / f lines of a Wavefront file, read and written
    fit_to_cube        uniform scale and centring into the cube
    icosphere, torus   generators for tests and tools/voxelize_probe.py
"""
import ctypes as C

import numpy as np
import torch

from ._device import device_u32, voxel_list, wait_for_torch
from ._lib import SolidParams, VoxelizeParams, lib

SUBBITS = 6  # SVO_VOX_SUBBITS: a cell is 64 quantised steps wide


def quantize_vertices(vertices, depth):
    """q = floor((v + 1) * 2^(depth + 5)) in float64, which is exact for float32 and float64 input: the vertex then
    stands at (q + 1/2) / 64 cells of the 2^depth grid, in the convention p = cell / 2^depth * 2 - 1.  vertices: (N, 3)
    floats in [-1, 1), numpy (returns int64 numpy) or a torch tensor (returns an int64 tensor on its device).  Raises
    ValueError for a vertex outside the cube; a float64 so close to the far face that v + 1 rounds to 2 counts as outside."""
    depth = int(depth)
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    scale = float(1 << (depth + SUBBITS - 1))
    tensor = isinstance(vertices, torch.Tensor)
    v = vertices.to(torch.float64) if tensor else np.asarray(vertices, dtype=np.float64)
    if not bool(((v >= -1.0) & (v + 1.0 < 2.0)).all()):  # (NaN included)
        raise ValueError("a vertex lies outside the cube [-1, 1)")
    q = (v + 1.0) * scale
    return torch.floor(q).to(torch.int64) if tensor else np.floor(q).astype(np.int64)


def voxelize(gpu, vertices, triangles, depth, colours=None, colour=0xFFFFFF, with_triangles=False, quantized=False):
    """Voxelise a triangle mesh on the GPU, conservatively and exactly (svo_mesh_voxelize).  vertices: (V, 3)
    floats in [-1, 1) (quantize_vertices is applied), or with quantized=True its integers; triangles: (T, 3) vertex
    indices; colours: T values 0x00RRGGBB or None (every triangle `colour`); numpy or torch tensors.  Returns device
    tensors (coords (N, 3) int32, colours (N) int32[, triangles (N) int32]): one entry per triangle and cell of the
    2^depth grid that meet, in ascending triangle index and Morton order within a triangle.  A count query and then a fill,
    like Render.list_voxels.  Raises SvoError for a bad vertex index or coordinate and for 2^31 entries or more."""
    dev = gpu.torch_device
    depth = int(depth)
    vq = device_u32(vertices if quantized else quantize_vertices(vertices, depth), dev, clamp=True, what="vertices")
    if vq.dim() != 2 or vq.shape[1] != 3:
        raise ValueError(f"vertices must be (V, 3), got {tuple(vq.shape)}")
    tri, col, n_tris, tri_ptr, col_ptr = voxel_list(gpu, triangles, colours, noun="triangles", what="triangles", rows="T")
    p = VoxelizeParams()
    p.depth = max(0, depth)
    p.default_colour = int(colour) & 0xFFFFFF
    p.n_vertices = vq.shape[0]
    args = (vq.data_ptr() if vq.numel() else None, tri_ptr, col_ptr, n_tris)
    n = C.c_uint64()
    wait_for_torch(gpu)
    gpu.check(lib().svo_mesh_voxelize(gpu._h, C.byref(p), *args, None, None, None, C.byref(n)))  # the count
    count = n.value
    coords = torch.empty((count, 3), dtype=torch.int32, device=dev)
    out_colours = torch.empty(count, dtype=torch.int32, device=dev)
    out_tris = torch.empty(count, dtype=torch.int32, device=dev) if with_triangles else None
    if count:
        p.max_voxels = count
        wait_for_torch(gpu)
        gpu.check(lib().svo_mesh_voxelize(gpu._h, C.byref(p), *args, coords.data_ptr(), out_colours.data_ptr(),
                                          out_tris.data_ptr() if with_triangles else None, C.byref(n)))
    gpu.sync()  # (the inputs may be released by the caller)
    return (coords, out_colours, out_tris) if with_triangles else (coords, out_colours)


SOLID_RULES = {"evenodd": 0, "nonzero": 1}  # SVO_SOLID_EVENODD, SVO_SOLID_NONZERO
SOLID_SPANS = 2  # SVO_SOLID_SPANS


def voxelize_solid(gpu, vertices, triangles, depth, rule="evenodd", spans=False, with_open=False, quantized=False, max_pairs=None):
    """The cells inside a closed triangle mesh, on the GPU and exactly (svo_mesh_voxelize_solid): a cell is
    inside when the triangles above its centre are odd in number (rule "evenodd") or their orientations do not cancel
    ("nonzero"); ties are decided as for a centre moved by an infinitesimal generic offset, so the order of the triangles
    never matters.  vertices and triangles as voxelize takes them.  Returns a device int32 tensor: (N, 3) cells (x, y, z)
    ascending in (x, z, y), the list build_nodes and edit_nodes take, or with spans=True (N, 4) runs (x, z, y0, y1) of
    inside cells [y0, y1) of a column, ascending in (x, z, y0); with with_open=True a pair of it and the number of open
    columns: columns where the mesh is not closed (0 for a watertight mesh).  A count query and then a fill, like voxelize.
    max_pairs caps the (triangle, column square) pairs of a level (None: 2^27).  Raises SvoError for a bad vertex index or
    coordinate, for a level over max_pairs and for 2^31 entries or more."""
    if rule not in SOLID_RULES:
        raise ValueError(f"rule must be one of {sorted(SOLID_RULES)} (got {rule!r})")
    dev = gpu.torch_device
    depth = int(depth)
    vq = device_u32(vertices if quantized else quantize_vertices(vertices, depth), dev, clamp=True, what="vertices")
    if vq.dim() != 2 or vq.shape[1] != 3:
        raise ValueError(f"vertices must be (V, 3), got {tuple(vq.shape)}")
    tri, _, n_tris, tri_ptr, _ = voxel_list(gpu, triangles, None, noun="triangles", what="triangles", rows="T")
    p = SolidParams()
    p.depth = max(0, depth)
    p.flags = SOLID_RULES[rule] | (SOLID_SPANS if spans else 0)
    p.n_vertices = vq.shape[0]
    p.max_pairs = 0 if max_pairs is None else int(max_pairs)
    args = (vq.data_ptr() if vq.numel() else None, tri_ptr, n_tris)
    n, n_open = C.c_uint64(), C.c_uint64()
    wait_for_torch(gpu)
    gpu.check(lib().svo_mesh_voxelize_solid(gpu._h, C.byref(p), *args, None, C.byref(n), C.byref(n_open)))  # the count
    count = n.value
    out = torch.empty((count, 4 if spans else 3), dtype=torch.int32, device=dev)
    if count:
        p.max_out = count
        wait_for_torch(gpu)
        gpu.check(lib().svo_mesh_voxelize_solid(gpu._h, C.byref(p), *args, out.data_ptr(), C.byref(n), C.byref(n_open)))
    gpu.sync()  # (the inputs may be released by the caller)
    return (out, n_open.value) if with_open else out


def load_obj(path):
    """A minimal Wavefront reader: `v x y z [r g b]` and `f` with i, i/j, i/j/k and i//k (negative indices count back from
    the last vertex read so far); polygons are fan-triangulated; everything else is ignored.  Returns (vertices (V, 3)
    float32, triangles (T, 3) int32, vertex_rgb (V, 3) float32 or None when not every vertex carries a colour)."""
    vertices, rgb, triangles = [], [], []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            part = line.split("#", 1)[0].split()
            if not part:
                continue
            if part[0] == "v":
                if len(part) < 4:
                    raise ValueError(f"{path}:{number}: a vertex needs three coordinates")
                vertices.append([float(x) for x in part[1:4]])
                rgb.append([float(x) for x in part[4:7]] if len(part) >= 7 else None)
            elif part[0] == "f":
                corner = []
                for word in part[1:]:
                    i = int(word.split("/", 1)[0])
                    i = i - 1 if i > 0 else len(vertices) + i
                    if i < 0 or i >= len(vertices):
                        raise ValueError(f"{path}:{number}: vertex index {word} outside the {len(vertices)} vertices read so far")
                    corner.append(i)
                if len(corner) < 3:
                    raise ValueError(f"{path}:{number}: a face needs three vertices")
                triangles += [[corner[0], corner[k], corner[k + 1]] for k in range(1, len(corner) - 1)]
    v = np.array(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.array(triangles, dtype=np.int32).reshape(-1, 3)
    colours = np.array(rgb, dtype=np.float32).reshape(-1, 3) if rgb and all(c is not None for c in rgb) else None
    return v, t, colours


def save_obj(path, vertices, triangles, vertex_rgb=None):
    """Writes `v x y z [r g b]` and `f a b c` lines (indices from 1) that load_obj reads back as the same arrays, bit for
    bit: a float32 is written as repr of the same number as a Python float, which names it exactly."""
    v = np.asarray(vertices.cpu() if isinstance(vertices, torch.Tensor) else vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles.cpu() if isinstance(triangles, torch.Tensor) else triangles, dtype=np.int64).reshape(-1, 3)
    rows = v if vertex_rgb is None else np.concatenate(
        [v, np.asarray(vertex_rgb.cpu() if isinstance(vertex_rgb, torch.Tensor) else vertex_rgb, dtype=np.float32).reshape(-1, 3)], axis=1)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError(f"a triangle names a vertex outside the {len(v)} vertices")
    with open(path, "w") as f:
        f.writelines("v " + " ".join(repr(x) for x in row) + "\n" for row in rows.astype(np.float64).tolist())
        f.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in t.tolist())


def _face_corners():
    """[f][k]: corner k of face f as unit steps along x, y, z from the leaf's minimum corner"""
    table = np.zeros((6, 4, 3), dtype=np.int64)
    for f in range(6):
        a = f >> 1
        corners = ((0, 0), (1, 0), (1, 1), (0, 1))  # in (u, v) for an odd face; an even face takes them in reverse
        for k, (cu, cv) in enumerate(corners if f & 1 else corners[::-1]):
            table[f, k, a], table[f, k, (a + 1) % 3], table[f, k, (a + 2) % 3] = f & 1, cu, cv
    return table


def quads_to_mesh(coords, faces, levels, depth, colours=None, weld=True, integer=False):
    """The quads of Render.surface_quads as an indexed triangle mesh, in plain torch on the tensors' device.  coords (Q, 3),
    faces (Q), levels (Q), colours (Q) or None.  A quad of a leaf at level l has side s = 2^(depth - l); with a = f >> 1,
    u = (a + 1) % 3, v = (a + 2) % 3 it lies in the plane min[a] + (f & 1) * s, and its corners are (0, 0), (s, 0), (s, s),
    (0, s) in (u, v) for odd f and in the reverse order for even f, so its normal points out of the leaf; its triangles
    are the corners (0, 1, 2) and (0, 2, 3).  Returns (vertices, triangles (T, 3) int32, triangle_colours (T) or None):
    vertices float32 cell / 2^depth * 2 - 1 (exact for depth <= 21), or with integer=True the int32 grid coordinates;
    weld: equal vertices are merged (torch.unique, sorted), else every quad keeps its own four."""
    depth = int(depth)
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    c = torch.as_tensor(coords).to(torch.int64).reshape(-1, 3)
    f = torch.as_tensor(faces).to(torch.int64).reshape(-1).to(c.device)
    side = torch.bitwise_left_shift(torch.ones_like(f), depth - torch.as_tensor(levels).to(torch.int64).reshape(-1).to(c.device))
    if not (len(f) == len(c) == len(side)):
        raise ValueError(f"coords, faces and levels must have one row per quad (got {len(c)}, {len(f)}, {len(side)})")
    if len(f) and not bool(((f >= 0) & (f < 6)).all()):
        raise ValueError("a face number outside 0..5")
    step = torch.from_numpy(_face_corners()).to(c.device)[f]  # (Q, 4, 3)
    return _mesh(c, step * side[:, None, None], depth, colours, weld, integer)


def _mesh(c, step, depth, colours, weld, integer):
    """the mesh of the faces at the corners c whose corner k is step[:, k] away: what quads_to_mesh documents"""
    cells = (c[:, None, :] + step).reshape(-1, 3)  # (4 Q, 3) grid coordinates in [0, 2^depth]
    index = torch.arange(4 * len(c), device=c.device)
    if weld:
        cells, index = torch.unique(cells, dim=0, sorted=True, return_inverse=True)
    quad = index.reshape(-1, 4)
    triangles = torch.stack([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]], dim=1).reshape(-1, 3).to(torch.int32)
    if integer:
        vertices = cells.to(torch.int32)
    else:  # (an integer below 2^22 over a power of two: every step is exact in float32)
        vertices = cells.to(torch.float32) / float(1 << depth) * 2.0 - 1.0
    tri_colours = None if colours is None else torch.as_tensor(colours).reshape(-1).to(c.device).repeat_interleave(2)
    return vertices, triangles, tri_colours


def rects_to_mesh(rects, values, depth, colours=None, weld=True, integer=False):
    """The rectangles of Render.surface_rects as an indexed triangle mesh, in plain torch on the tensors' device.  rects
    (R, 6): face, plane, u0, v0, w, h; values (R): the triangles' colours unless `colours` (R) is given (both None: no
    colours).  With a = face >> 1, u = (a + 1) % 3, v = (a + 2) % 3 a rectangle lies in the plane `plane` of axis a, and its
    corners are (0, 0), (w, 0), (w, h), (0, h) from (u0, v0) in (u, v) for an odd face and in the reverse order for an
    even one, so its normal points out of the leaves behind it.  Triangles, vertices, weld and integer are quads_to_mesh's,
    and for rectangles with w = h = s the result is what quads_to_mesh returns for the same quads.  The rectangles of a
    merged surface meet in T-junctions: the mesh covers the surface exactly but is no longer edge to edge."""
    depth = int(depth)
    if not 1 <= depth <= 21:
        raise ValueError(f"depth must be 1..21 (got {depth})")
    r = torch.as_tensor(rects).to(torch.int64).reshape(-1, 6)
    if colours is None:
        colours = values
    if colours is not None and len(torch.as_tensor(colours).reshape(-1)) != len(r):
        raise ValueError(f"rects and values must have one row per rectangle (got {len(r)}, {len(torch.as_tensor(colours).reshape(-1))})")
    f = r[:, 0]
    if len(f) and not bool(((f >= 0) & (f < 6)).all()):
        raise ValueError("a face number outside 0..5")
    a = f >> 1
    rows = torch.arange(len(r), device=r.device)
    c = torch.zeros((len(r), 3), dtype=torch.int64, device=r.device)
    c[rows, a], c[rows, (a + 1) % 3], c[rows, (a + 2) % 3] = r[:, 1], r[:, 2], r[:, 3]
    unit = torch.from_numpy(_face_corners()).to(r.device)[f]  # (R, 4, 3): 0 or 1 along each axis; along a it is the face's parity
    extent = torch.zeros((len(r), 3), dtype=torch.int64, device=r.device)
    extent[rows, (a + 1) % 3], extent[rows, (a + 2) % 3] = r[:, 4], r[:, 5]
    return _mesh(c, unit * extent[:, None, :], depth, colours, weld, integer)


def extract_surface(render, depth=None, closed_boundary=False, weld=True, merge=False, rounds=1):
    """The visible surface of the tree in render's node buffer as a triangle mesh: Render.surface_quads, then
    quads_to_mesh, both on the GPU; with merge=True Render.surface_rects (with `rounds`) and rects_to_mesh: the same
    surface in fewer triangles.  Returns (vertices float32, triangles int32, triangle_colours int32)."""
    d = int(render.gpu.tree_depth if depth is None else depth)
    if merge:
        rects, values = render.surface_rects(d, closed_boundary, rounds)
        return rects_to_mesh(rects, values, d, weld=weld)
    coords, colours, faces, levels = render.surface_quads(d, closed_boundary)
    return quads_to_mesh(coords, faces, levels, d, colours, weld=weld)


def fit_to_cube(vertices, margin=0.02):
    """The vertices scaled uniformly and centred so that their bounding box's longest side spans [-1 + margin, 1 - margin]
    (float64 in, float64 out; float32 otherwise)."""
    v = np.asarray(vertices)
    v = v.astype(np.float64 if v.dtype == np.float64 else np.float32)
    if v.size == 0:
        return v
    lo, hi = v.min(axis=0), v.max(axis=0)
    extent = float((hi - lo).max())
    scale = (1.0 - margin) * 2.0 / extent if extent > 0 else 1.0
    return ((v - (lo + hi) / 2) * scale).astype(v.dtype)


def icosphere(subdivisions=2, radius=0.8, centre=(0.0, 0.0, 0.0)):
    """An icosahedron subdivided `subdivisions` times onto the sphere: (vertices float32, triangles int32) with
    20 * 4^subdivisions triangles, the same arrays on every run."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = np.array(v, dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    t = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], dtype=np.int64)
    for _ in range(int(subdivisions)):
        # one new vertex per edge, in the order of the edges' (low, high) vertex pairs
        ends = np.sort(np.stack([t, np.roll(t, -1, axis=1)], axis=-1).reshape(-1, 2), axis=1)
        edge, mid = np.unique(ends[:, 0] * len(v) + ends[:, 1], return_inverse=True)
        new = v[edge // len(v)] + v[edge % len(v)]
        mid = mid.reshape(-1, 3) + len(v)  # per triangle: the midpoints of ab, bc, ca
        v = np.concatenate([v, new / np.linalg.norm(new, axis=1, keepdims=True)])
        a, b, c, ab, bc, ca = t[:, 0], t[:, 1], t[:, 2], mid[:, 0], mid[:, 1], mid[:, 2]
        t = np.stack([np.stack(x, axis=-1) for x in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))], axis=1).reshape(-1, 3)
    vertices = v * float(radius) + np.array(centre, dtype=np.float64)
    return vertices.astype(np.float32), t.astype(np.int32)


def torus(nu=24, nv=12, R=0.6, r=0.2, centre=(0.0, 0.0, 0.0)):
    """A torus around the y axis, nu segments around the axis and nv around the tube: (vertices float32, triangles int32)
    with 2 * nu * nv triangles, the same arrays on every run."""
    u = np.arange(nu, dtype=np.float64) * (2 * np.pi / nu)
    w = np.arange(nv, dtype=np.float64) * (2 * np.pi / nv)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    ring = R + r * np.cos(ww)
    vertices = np.stack([ring * np.cos(uu), r * np.sin(ww), ring * np.sin(uu)], axis=-1).reshape(-1, 3) + np.array(centre, dtype=np.float64)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    triangles = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=2).reshape(-1, 3)
    return vertices.astype(np.float32), triangles.astype(np.int32)
