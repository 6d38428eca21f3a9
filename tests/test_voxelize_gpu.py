"""Triangle meshes voxelised on the GPU (csrc/svo_voxelize.hip): cells, colours and triangle indices bit
for bit against the level refinement of tests/voxelize_ref.py, on single triangles at depth 1, random and degenerate
triangles at depths 2 and 3, triangle counts and pair counts around the scan's tile, two meshes at depth 7 (with the trees
built and edited from their lists), and depth 21 next to the grid's far corner; the cap's refusal with its level and count;
the count query, the same bytes on every run, nothing written behind n or by any refused call, the node buffer never."""
import ctypes as C
import re

import numpy as np
import pytest

import build_ref as B
import edit_ref as E
import voxelize_ref as V
from pass_frame import SENTINEL, SLACK, SentinelOut, last_error, own_gpu  # noqa: F401
from test_edit_gpu import CAPACITY, PAD, ROOT, poison, set_base
from test_voxelize_host import planar_quad, random_mesh

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_CAP = -1, -3, -6
TOP21 = 1 << 27        # quantised coordinates of depth 21 lie below this


class Out(SentinelOut):
    """sentinel-filled device outputs of `room` entries"""

    def __init__(self, gpu, room):
        super().__init__(gpu, [(room, 3), room, room])
        self.xyz, self.colour, self.tri = self.t
        self.room = room


class Mesh:
    """a mesh's arrays on the device, as the entry point takes them"""

    def __init__(self, gpu, vq, tris, colours=None):
        import torch
        dev = torch.device("cuda", gpu.device)
        u32 = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)), device=dev)  # noqa: E731
        self.vq, self.tris = u32(np.asarray(vq).reshape(-1, 3)), u32(np.asarray(tris).reshape(-1, 3))
        self.colours = u32(colours) if colours is not None else None
        torch.cuda.current_stream(dev).synchronize()


def raw_voxelize(pkg, gpu, mesh, depth, out=None, max_voxels=None, params=True, n_out=True, colour_out=True, tri_out=True, flags=0,
                 n_tris=None, vq=True, tris=True, default_colour=0xFFFFFF):
    p = pkg._lib.VoxelizeParams()
    p.depth, p.flags, p.default_colour, p.n_vertices = depth, flags, default_colour, mesh.vq.shape[0]
    p.max_voxels = (out.room if out is not None else 0) if max_voxels is None else max_voxels
    n = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_mesh_voxelize(
        gpu._h, C.byref(p) if params else None, mesh.vq.data_ptr() if vq and mesh.vq.numel() else None,
        mesh.tris.data_ptr() if tris and mesh.tris.numel() else None, mesh.colours.data_ptr() if mesh.colours is not None else None,
        mesh.tris.shape[0] if n_tris is None else n_tris, out.xyz.data_ptr() if out is not None else None,
        out.colour.data_ptr() if out is not None and colour_out else None, out.tri.data_ptr() if out is not None and tri_out else None,
        C.byref(n) if n_out else None)
    gpu.sync()
    return rc, n.value


def check_mesh(pkg, gpu, vq, tris, depth, colours, what, want=None, colour=0xFFFFFF):
    """the mesh's list on the GPU == the reference; the count query agrees and writes nothing; nothing is written behind
    n.  Returns the list's three host arrays."""
    want = want if want is not None else V.voxelize(vq, tris, depth, colours, colour)
    mesh = Mesh(gpu, vq, tris, colours)
    rc, n = raw_voxelize(pkg, gpu, mesh, depth, default_colour=colour)
    assert rc == 0, f"{what}: count query: status {rc}: {last_error(pkg, gpu)}"
    assert n == want[1].size, f"{what}: count {n}, want {want[1].size}"
    out = Out(gpu, n + SLACK)
    rc, m = raw_voxelize(pkg, gpu, mesh, depth, out, default_colour=colour)
    assert rc == 0, f"{what}: status {rc}: {last_error(pkg, gpu)}"
    assert m == n, f"{what}: the fill's n {m}, the count query's {n}"
    got = out.host()
    for g, w, name in zip(got, want, ("xyz", "colour", "tri")):
        if not np.array_equal(g[:n], w):
            bad = np.flatnonzero((g[:n] != w).reshape(n, -1).any(axis=1))
            raise AssertionError(f"{what}: {bad.size} entries differ in {name}, first at {bad[:3]}: got {g[bad[:3]]} want {w[bad[:3]]}")
    assert out.untouched_from(n), f"{what}: written behind n"
    return tuple(g[:n] for g in got)


def test_depth_1_single_triangles(pkg, own_gpu):
    cases = {"inside an octant": ([[70, 70, 70], [100, 80, 75], [80, 110, 90]], 1),
             # the edge from (0, 1, 2) to (127, 126, 125) passes through the grid's centre, a point of all eight closed cubes
             "through all eight octants": ([[0, 1, 2], [127, 126, 125], [100, 5, 60]], 8),
             "a point": ([[5, 5, 5]] * 3, 1),
             "a segment": ([[5, 5, 5], [120, 5, 5], [120, 5, 5]], 2)}
    for name, (vq, cells) in cases.items():
        xyz, colour, tri = check_mesh(pkg, own_gpu, vq, [[0, 1, 2]], 1, None, name, colour=0x123456)
        assert len(xyz) == cells and (colour == 0x123456).all() and (tri == 0).all(), name
    xyz, _, tri = check_mesh(pkg, own_gpu, sum((c[0] for c in cases.values()), []), np.arange(12).reshape(4, 3), 1, [1, 2, 3, 4], "all four")
    assert np.bincount(tri).tolist() == [1, 8, 1, 2]


@pytest.mark.parametrize("depth", [2, 3])
def test_random_and_degenerate_triangles(pkg, own_gpu, depth):
    vq, tris, colours = random_mesh(100 + depth, depth, 50)
    quad = planar_quad(depth)
    tris = np.concatenate([tris, quad[1] + len(vq)])
    vq = np.concatenate([vq, quad[0]])
    colours = np.concatenate([colours, [0xFF000005, 6]])  # (the high byte is masked away)
    xyz, colour, tri = check_mesh(pkg, own_gpu, vq, tris, depth, colours, f"depth {depth}")
    assert set(tri.tolist()) == set(range(52))
    wall = xyz[tri >= 50]
    assert len(wall) >= 9 and (wall[:, 1] == 2).all()  # the quad on the grid plane y = 2 is one cell thick
    assert set(colour[tri == 50].tolist()) == {5}


def one_cell_triangles(seed, depth, n):
    """n triangles, each inside one random cell"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 1 << depth, (n, 1, 3))
    return (cells * 64 + rng.integers(0, 64, (n, 3, 3))).reshape(-1, 3), np.arange(3 * n).reshape(n, 3), cells.reshape(n, 3)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_triangle_counts_around_the_scans_tile(pkg, own_gpu, n):
    vq, tris, cells = one_cell_triangles(n, 5, n)
    colours = np.arange(1, n + 1)
    xyz, colour, tri = check_mesh(pkg, own_gpu, vq, tris, 5, colours, f"{n} one-cell triangles")
    assert np.array_equal(xyz, cells) and np.array_equal(tri, np.arange(n)) and np.array_equal(colour, colours)


def test_a_levels_pairs_span_several_tiles(pkg, own_gpu):
    vq, tris, colours = random_mesh(8, 8, 10000, n_vertices=6000, extent=200)
    xyz, colour, tri = check_mesh(pkg, own_gpu, vq, tris, 8, colours, "10 000 small triangles at depth 8")
    assert len(tri) > 5 * 4096


@pytest.fixture(scope="module")
def meshes7(pkg):
    """icosphere(2) and a torus at depth 7 with a colour per triangle: the quantised mesh and the reference list, once"""
    out = {}
    for name, (v, t) in (("icosphere", pkg.mesh.icosphere(2, 0.5, (0.05, -0.1, 0.2))), ("torus", pkg.mesh.torus(24, 12, 0.5, 0.2, (0.1, 0.0, -0.05)))):
        vq = pkg.mesh.quantize_vertices(v, 7)
        colours = 0x010000 + np.arange(len(t))
        out[name] = {"v": v, "t": t, "vq": vq, "colours": colours, "list": V.voxelize(vq, t, 7, colours)}
    assert len(out["icosphere"]["t"]) == 320
    return out


def last_wins(xyz, colour, depth):
    """the distinct cells in Morton order, each with the colour of its last entry"""
    key = B.morton(xyz, depth)
    keys, first = np.unique(key[::-1], return_index=True)
    return xyz[::-1][first], colour[::-1][first]


@pytest.mark.parametrize("name", ["icosphere", "torus"])
def test_depth_7_meshes_and_their_trees(pkg, own_gpu, meshes7, name):
    m = meshes7[name]
    want = m["list"]
    check_mesh(pkg, own_gpu, m["vq"], m["t"], 7, m["colours"], name, want)
    # the public call, from float vertices, with the triangle indices
    coords, colours, tris = pkg.mesh.voxelize(own_gpu, m["v"], m["t"], 7, m["colours"], with_triangles=True)
    assert coords.dtype == colours.dtype == tris.dtype and coords.dtype.is_signed and coords.shape == (len(want[1]), 3)
    for got, w in zip((coords, colours, tris), want):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), w)
    # voxelise and build: the words of the reference list's tree
    render = pkg.Render.from_mesh(own_gpu, (64, 64), m["v"], m["t"], 7, m["colours"], capacity=CAPACITY)
    words = B.build(want[0], 7, want[1])
    assert render.node_length == words.size and np.array_equal(render.read_nodes(), words)
    assert render.build_nodes_mesh(m["vq"], m["t"], 7, m["colours"], quantized=True) == words.size
    assert np.array_equal(render.read_nodes(), words)
    # the tree lists as the distinct cells, each with the colour of its highest triangle
    cells, cell_colours = last_wins(want[0], want[1], 7)
    assert len(cells) < len(want[1])  # (cells are shared between neighbouring triangles)
    listed = render.list_voxels(7)
    assert np.array_equal(listed[0].cpu().numpy().view(np.uint32), cells) and np.array_equal(listed[1].cpu().numpy().view(np.uint32), cell_colours)
    # the list edited into a tree that is not empty
    rng = np.random.default_rng(7)
    base = B.build(rng.integers(0, 128, (3000, 3)), 7, rng.integers(1, 1 << 24, 3000))
    edited = E.edit(base, base.size, want[0], 7, want[1])
    set_base(render, base, edited.size - base.size)
    assert render.edit_nodes(coords, 7, colours) == edited.size
    assert np.array_equal(render.read_nodes(), edited)


def test_depth_21_next_to_the_far_corner(pkg, own_gpu):
    vq = [[TOP21 - 1 - 64 * 300, TOP21 - 10, TOP21 - 20], [TOP21 - 1, TOP21 - 5, TOP21 - 70], [TOP21 - 64 * 150, TOP21 - 3, TOP21 - 30]]
    xyz, colour, tri = check_mesh(pkg, own_gpu, vq, [[0, 1, 2]], 21, [0xABCDEF], "depth-21 sliver")
    assert 300 <= len(xyz) < 2000 and xyz.max() == (1 << 21) - 1 and xyz.min() >= (1 << 21) - 302


def test_the_cap_stops_the_corner_to_corner_sliver_at_its_level(pkg, own_gpu):
    vq = [[0, 0, 0], [TOP21 - 1, TOP21 - 1, TOP21 - 1], [TOP21 - 1, TOP21 - 1, TOP21 - 2]]
    stopped = V.voxelize(vq, [[0, 1, 2]], 21, cap=4096)
    assert isinstance(stopped, V.Stopped) and stopped.count > 4096
    mesh = Mesh(own_gpu, vq, [[0, 1, 2]])
    out = Out(own_gpu, 4096 + SLACK)
    assert raw_voxelize(pkg, own_gpu, mesh, 21, out, max_voxels=4096) == (ERR_CAP, 12345)
    found = re.search(r"level (\d+) has (\d+) ", last_error(pkg, own_gpu))
    assert found and (int(found.group(1)), int(found.group(2))) == (stopped.level, stopped.count), last_error(pkg, own_gpu)
    assert "max_voxels = 4096" in last_error(pkg, own_gpu)
    assert out.untouched_from(0)


def test_count_query_runs_and_no_triangles(pkg, own_gpu, meshes7):
    m = meshes7["torus"]
    mesh = Mesh(own_gpu, m["vq"], m["t"], m["colours"])
    count = len(m["list"][1])
    assert raw_voxelize(pkg, own_gpu, mesh, 7, max_voxels=0) == (0, count)  # a count query does not look at max_voxels
    runs = []
    for _ in range(2):
        out = Out(own_gpu, count + SLACK)
        assert raw_voxelize(pkg, own_gpu, mesh, 7, out) == (0, count)
        runs.append(out.host())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    # without the triangle output
    out = Out(own_gpu, count + SLACK)
    assert raw_voxelize(pkg, own_gpu, mesh, 7, out, tri_out=False) == (0, count)
    assert np.array_equal(out.host()[0][:count], m["list"][0]) and (out.host()[2] == SENTINEL).all()
    # no triangles: success with 0, with and without outputs, with and without vertices
    for vq in (m["vq"], np.zeros((0, 3))):
        empty = Mesh(own_gpu, vq, np.zeros((0, 3)))
        out = Out(own_gpu, SLACK)
        assert raw_voxelize(pkg, own_gpu, empty, 7, out) == (0, 0) and raw_voxelize(pkg, own_gpu, empty, 7) == (0, 0)
        assert out.untouched_from(0)
    coords, colours, tris = pkg.mesh.voxelize(own_gpu, m["v"], np.zeros((0, 3), dtype=np.int32), 7, with_triangles=True)
    assert coords.shape == (0, 3) and colours.shape == (0,) and tris.shape == (0,)


def test_errors_in_their_order_write_nothing(pkg, own_gpu, meshes7):
    m = meshes7["icosphere"]
    count = len(m["list"][1])
    mesh = Mesh(own_gpu, m["vq"], m["t"], m["colours"])
    out = Out(own_gpu, count + SLACK)

    def refused(code, part, mesh=mesh, depth=7, **kw):
        got = raw_voxelize(pkg, own_gpu, mesh, depth, kw.pop("out", out), **kw)
        return got == (code, 12345) and part in last_error(pkg, own_gpu)

    # every cause alone, then with the next one in the contract's order: the earlier one is reported
    assert refused(ERR_ARG, "null params", params=False)
    assert refused(ERR_ARG, "null params", params=False, n_out=False)
    assert refused(ERR_ARG, "null n_out", n_out=False)
    assert refused(ERR_ARG, "null n_out", n_out=False, flags=1)
    for flags in (1, 1 << 31):
        assert refused(ERR_ARG, "flag", flags=flags)
    assert refused(ERR_ARG, "flag", flags=2, depth=0)
    for depth in (0, 22):
        assert refused(ERR_ARG, "depth", depth=depth)
    assert refused(ERR_ARG, "depth", depth=22, n_tris=1 << 31)
    assert refused(ERR_ARG, "n_tris", n_tris=1 << 31)
    assert refused(ERR_ARG, "n_tris", n_tris=1 << 40, vq=False)
    assert refused(ERR_ARG, "vq_dev", vq=False)
    assert refused(ERR_ARG, "tri_dev", tris=False)
    assert refused(ERR_ARG, "vq_dev", vq=False, colour_out=False)
    assert refused(ERR_ARG, "colour_out_dev", colour_out=False)
    # on the device: the first triangle with a vertex index that is no vertex, or with a coordinate outside the grid
    tris = m["t"].copy()
    tris[7, 1] = len(m["vq"])
    tris[3, 2] = 0x7FFFFFFF
    bad_index = Mesh(own_gpu, m["vq"], tris, m["colours"])
    assert refused(ERR_ARG, "triangle 3 has a vertex index", mesh=bad_index)
    assert refused(ERR_ARG, "triangle 3 has a vertex index", mesh=bad_index, out=None)
    assert refused(ERR_ARG, "colour_out_dev", mesh=bad_index, colour_out=False)
    assert refused(ERR_ARG, "triangle 3 has a vertex index", mesh=bad_index, max_voxels=1)  # before the cap
    vq = m["vq"].copy()
    vq[m["t"][5, 0], 2] = 1 << 13  # = 2^(depth + 6): the first coordinate outside
    at = int(np.flatnonzero((m["t"] == m["t"][5, 0]).any(axis=1)).min())
    assert refused(ERR_ARG, f"triangle {at} has a coordinate", mesh=Mesh(own_gpu, vq, m["t"], m["colours"]))
    vq[m["t"][5, 0], 2] = (1 << 13) - 1
    assert raw_voxelize(pkg, own_gpu, Mesh(own_gpu, vq, m["t"]), 7)[0] == 0
    tris = m["t"].copy()
    tris[at + 1] = len(m["vq"]) + 5
    vq[m["t"][5, 0], 0] = 0xFFFFFFFF
    assert refused(ERR_ARG, f"triangle {at} has a coordinate", mesh=Mesh(own_gpu, vq, tris))
    with pytest.raises(pkg.SvoError):
        pkg.mesh.voxelize(own_gpu, vq, tris, 7, quantized=True)
    with pytest.raises(ValueError):
        pkg.mesh.voxelize(own_gpu, m["v"] * 2, m["t"], 7)
    # room for one entry less than there are
    assert refused(ERR_CAP, f"level 7 has {count} ", max_voxels=count - 1)
    assert refused(ERR_CAP, "level ", max_voxels=0)
    assert out.untouched_from(0)
    assert raw_voxelize(pkg, own_gpu, mesh, 7, out, max_voxels=count) == (0, count) and out.untouched_from(count)


def test_the_node_buffer_is_never_touched_and_timing(pkg, own_gpu, meshes7):
    render = pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)
    rng = np.random.default_rng(3)
    base = B.build(rng.integers(0, 64, (2000, 3)), 6, rng.integers(1, 1 << 24, 2000))
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    assert np.array_equal(before[base.size:], poison(PAD))
    m = meshes7["icosphere"]
    coords, colours = pkg.mesh.voxelize(own_gpu, m["v"], m["t"], 7, m["colours"])
    assert np.array_equal(coords.cpu().numpy().view(np.uint32), m["list"][0])
    assert np.array_equal(render.read_nodes(base.size + PAD), before) and render.node_length == base.size
    ms = own_gpu.voxelize_timing()
    assert len(ms) == 5 and all(t >= 0 for t in ms) and ms[4] > 0 and ms[3] > 0
    assert ms == own_gpu.voxelize_timing()
    assert raw_voxelize(pkg, own_gpu, Mesh(own_gpu, m["vq"], m["t"]), 0)[0] == ERR_ARG  # a refused call leaves the times
    assert raw_voxelize(pkg, own_gpu, Mesh(own_gpu, m["vq"], m["t"]), 7, Out(own_gpu, 8), max_voxels=8)[0] == ERR_CAP
    assert ms == own_gpu.voxelize_timing()
    # a context with no node buffer voxelises; one that has not, has no times
    fresh = pkg.Gpu(0)
    try:
        with pytest.raises(pkg.SvoError):
            fresh.voxelize_timing()
        coords, colours = pkg.mesh.voxelize(fresh, m["v"], m["t"], 7, m["colours"])
        assert np.array_equal(colours.cpu().numpy().view(np.uint32), m["list"][1])
        assert fresh.voxelize_timing()[4] > 0
    finally:
        fresh.close()
