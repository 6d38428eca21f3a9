"""Closed meshes voxelised solid on the GPU (csrc/svo_solid.hip): cells, spans and the open-column count bit
for bit against tests/solid_ref.py under both rules, on a tetrahedron at depth 1, random soups and designed ties at depths
2 and 3, open meshes, counts around the scan's tile, one column of 4 098 crossings, the whole grid at depth 7 and the far
corner cell of depth 21, and 2^32 cells and more refused with their 64-bit count; the count query, the same bytes on every run, nothing written behind n or by any refused call, the
node buffer never; and a solid model through Render.from_mesh, sealed by its surface."""
import ctypes as C
import re

import numpy as np
import pytest

import build_ref as B
import solid_ref as S
from pass_frame import SENTINEL, SLACK, SentinelOut, last_error, own_gpu  # noqa: F401
from test_edit_gpu import CAPACITY, PAD, ROOT, poison, set_base
from test_solid_host import RULES, box_mesh, cell_tetrahedra, join, tetra_soup, tie_mesh
from test_voxelize_gpu import Mesh
from test_voxelize_host import planar_quad

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAP = -1, -6


def raw_solid(pkg, gpu, mesh, depth, flags=0, out=None, max_out=None, max_pairs=0, params=True, n_out=True, n_open=True, reserved=0,
              n_tris=None, vq=True, tris=True):
    """(status, *n_out, *n_open_out) of one call; out: a SentinelOut of one tensor, or None for a count query"""
    p = pkg._lib.SolidParams()
    p.depth, p.flags, p.n_vertices, p.reserved, p.max_pairs = depth, flags, mesh.vq.shape[0], reserved, max_pairs
    p.max_out = (out.t[0].shape[0] - SLACK if out is not None else 0) if max_out is None else max_out
    n, o = C.c_uint64(12345), C.c_uint64(54321)
    rc = pkg._lib.lib().svo_mesh_voxelize_solid(
        gpu._h, C.byref(p) if params else None, mesh.vq.data_ptr() if vq and mesh.vq.numel() else None,
        mesh.tris.data_ptr() if tris and mesh.tris.numel() else None, mesh.tris.shape[0] if n_tris is None else n_tris,
        out.t[0].data_ptr() if out is not None else None, C.byref(n) if n_out else None, C.byref(o) if n_open else None)
    gpu.sync()
    return rc, n.value, o.value


def check_solid(pkg, gpu, vq, tris, depth, what, want=None):
    """both rules, cells and spans: the count query and the fill agree with the reference, the query writes nothing and
    nothing is written behind n.  want: the reference's results by rule.  Returns them."""
    mesh = Mesh(gpu, vq, tris)
    want = want or {rule: S.solid(vq, tris, depth, rule) for rule in RULES}
    for rule in RULES:
        for flags, ref, width in ((rule, want[rule].cells, 3), (rule | S.SPANS, want[rule].spans, 4)):
            tag = f"{what}, flags {flags}"
            rc, n, n_open = raw_solid(pkg, gpu, mesh, depth, flags)
            assert rc == 0, f"{tag}: count query: status {rc}: {last_error(pkg, gpu)}"
            assert (n, n_open) == (len(ref), want[rule].n_open), f"{tag}: count {n} ({n_open} open), want {len(ref)} ({want[rule].n_open} open)"
            out = SentinelOut(gpu, [(n + SLACK, width)])
            rc, m, m_open = raw_solid(pkg, gpu, mesh, depth, flags, out)
            assert rc == 0, f"{tag}: status {rc}: {last_error(pkg, gpu)}"
            assert (m, m_open) == (n, n_open), f"{tag}: the fill's counts {m}, {m_open}, the query's {n}, {n_open}"
            got = out.host()[0]
            if not np.array_equal(got[:n], ref):
                bad = np.flatnonzero((got[:n] != ref).any(axis=1))
                raise AssertionError(f"{tag}: {bad.size} entries differ, first at {bad[:3]}: got {got[bad[:3]]} want {ref[bad[:3]]}")
            assert out.untouched_from(n), f"{tag}: written behind n"
    return want


def test_depth_1_single_tetrahedron(pkg, own_gpu):
    vq, tris, cells = cell_tetrahedra(1, 1, 1)
    want = check_solid(pkg, own_gpu, vq, tris, 1, "one tetrahedron")
    assert want[S.EVENODD].cells.tolist() == cells.tolist() == [[0, 0, 0]] and want[S.EVENODD].crossings == 2
    big = [[2, 3, 4], [125, 5, 6], [60, 4, 126], [63, 120, 62]]  # around the grid's centre: all eight cells' columns
    want = check_solid(pkg, own_gpu, big, tris, 1, "a tetrahedron over the grid")
    assert len(want[S.NONZERO].spans) >= 2


@pytest.mark.parametrize("depth", [2, 3])
def test_random_soups_and_ties(pkg, own_gpu, depth):
    rng = np.random.default_rng(depth)
    loose = rng.integers(0, 1 << (depth + S.SUBBITS), (30, 3)), np.arange(30).reshape(10, 3)
    vq, tris = join(tetra_soup(20 + depth, depth, 12), tie_mesh(depth), loose)
    want = check_solid(pkg, own_gpu, vq, tris, depth, f"depth {depth}")
    assert want[S.EVENODD].n_open > 0 and not np.array_equal(want[S.EVENODD].cells, want[S.NONZERO].cells)
    order = rng.permutation(len(tris))  # the triangles' order does not matter
    check_solid(pkg, own_gpu, vq, tris[order], depth, f"depth {depth}, shuffled", want)
    check_solid(pkg, own_gpu, *tetra_soup(30 + depth, depth, 12), depth, f"depth {depth}, closed")


def test_open_meshes_count_their_open_columns(pkg, own_gpu):
    want = check_solid(pkg, own_gpu, [[10, 200, 20], [240, 180, 30], [100, 220, 250]], [[0, 1, 2]], 2, "one triangle")
    assert want[S.EVENODD].n_open == want[S.EVENODD].crossings > 0 and len(want[S.EVENODD].cells) > 0
    quad = planar_quad(3)
    want = check_solid(pkg, own_gpu, quad[0], quad[1], 3, "a quad on the plane y = 2")
    assert want[S.NONZERO].n_open == 9 and want[S.NONZERO].spans[:, 2:].tolist() == [[0, 2]] * 9


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_counts_around_the_scans_tile(pkg, own_gpu, n):
    vq, tris, cells = cell_tetrahedra(n, 5, n)
    want = check_solid(pkg, own_gpu, vq, tris, 5, f"{n} one-cell tetrahedra")
    order = np.lexsort((cells[:, 1], cells[:, 2], cells[:, 0]))
    assert np.array_equal(want[S.EVENODD].cells, cells[order]) and want[S.EVENODD].crossings == 2 * n


def test_one_column_of_4098_crossings(pkg, own_gpu):
    """2 049 slabs, one quantum thick and one apart, stacked in one column at depth 7: most crossings share their height,
    the column's segment crosses a tile, and the cells' spans, apart by empty intervals alone, are one run"""
    x0, z0 = 64 * 37 + 10, 64 * 90 + 12
    vq, tris = join(*[box_mesh((x0, 2 * i + 1, z0), (x0 + 40, 2 * i + 2, z0 + 41)) for i in range(2049)])
    want = check_solid(pkg, own_gpu, vq, tris, 7, "2 049 slabs")
    assert want[S.EVENODD].crossings == 4098 and want[S.EVENODD].spans.tolist() == [[37, 90, 0, 64]] and want[S.NONZERO].n_open == 0
    # slabs that lie between the centres: every interval is empty, so no cell at all, and no column is open
    vq, tris = join(*[box_mesh((x0, 2 * i, z0), (x0 + 40, 2 * i + 1, z0 + 41)) for i in range(1, 300)])
    want = check_solid(pkg, own_gpu, vq, tris, 7, "slabs between the centres")
    assert len(want[S.EVENODD].cells) == 0 and want[S.EVENODD].crossings == 2 * 299 and want[S.EVENODD].n_open == 0


@pytest.fixture(scope="module")
def whole7():
    """one box spanning the whole grid at depth 7, with the reference's results"""
    vq, tris = box_mesh((0, 0, 0), (8191, 8191, 8191))
    return vq, tris, {rule: S.solid(vq, tris, 7, rule) for rule in RULES}


def test_the_whole_grid_at_depth_7(pkg, own_gpu, whole7):
    vq, tris, want = whole7
    assert len(want[S.EVENODD].cells) == 1 << 21 and len(want[S.EVENODD].spans) == 1 << 14
    check_solid(pkg, own_gpu, vq, tris, 7, "the whole grid", want)


def test_depth_21_far_corner_cell(pkg, own_gpu):
    last = (1 << 21) - 1
    vq, tris, _ = cell_tetrahedra(21, 1, 1)
    vq = vq + 64 * last
    want = check_solid(pkg, own_gpu, vq, tris, 21, "depth-21 corner cell")
    assert want[S.EVENODD].cells.tolist() == [[last] * 3] and want[S.NONZERO].spans.tolist() == [[last, last, last, last + 1]]
    # a roof over the corner column: 2^21 cells in one span are counted, and refused where the list would pass the room
    roof = [[64 * last + 2, 64 * last + 40, 64 * last + 3], [64 * last + 60, 64 * last + 41, 64 * last + 5], [64 * last + 30, 64 * last + 42, 64 * last + 62]]
    mesh = Mesh(own_gpu, roof, [[0, 1, 2]])
    assert raw_solid(pkg, own_gpu, mesh, 21, S.SPANS) == (0, 1, 1)
    assert raw_solid(pkg, own_gpu, mesh, 21, 0) == (0, 1 << 21, 1)
    out = SentinelOut(own_gpu, [(1000 + SLACK, 3)])
    assert raw_solid(pkg, own_gpu, mesh, 21, 0, out)[0] == ERR_CAP and f"{1 << 21} cells" in last_error(pkg, own_gpu)
    assert out.untouched_from(0)


def test_2_to_the_31_cells_or_more_are_refused_with_their_64_bit_count(pkg, own_gpu):
    """a roof over more than 2 048 whole columns of depth 21: 2^32 cells and more, counted in 64 bits, refused always"""
    last = (1 << 21) - 1
    base, top = 64 * (last - 80), 64 * last + 40
    roof = [[base + 2, top, base + 3], [base + 64 * 75 + 2, top + 1, base + 5], [base + 30, top + 2, base + 64 * 75]]
    levels = []
    t, col = S.refine(S.doubled(roof, [[0, 1, 2]]), 21, levels=levels)
    heights, _ = S._heights(S.doubled(roof, [[0, 1, 2]])[t], col, 21)
    columns, cells = len(col), int(heights.sum())
    assert columns > 2048 and (heights == 1 << 21).all() and cells == columns << 21 and cells >= 1 << 32
    assert cells & 0xFFFFFFFF != 0  # the low half alone would be a plausible count
    mesh = Mesh(own_gpu, roof, [[0, 1, 2]])
    for rule in RULES:
        # the spans are few and come back, each a whole column
        spans = SentinelOut(own_gpu, [(columns + SLACK, 4)])
        assert raw_solid(pkg, own_gpu, mesh, 21, rule | S.SPANS, spans) == (0, columns, columns)
        got = spans.host()[0][:columns]
        assert (got[:, 2] == 0).all() and (got[:, 3] == 1 << 21).all() and np.array_equal(got[:, :2], col[np.lexsort((col[:, 1], col[:, 0]))])
        # the cells are refused in a count query and in a fill, whatever the room, and nothing is written
        assert raw_solid(pkg, own_gpu, mesh, 21, rule) == (ERR_CAP, 12345, 54321)
        assert f"{cells} cells" in last_error(pkg, own_gpu) and "2^31" in last_error(pkg, own_gpu)
        out = SentinelOut(own_gpu, [(4096 + SLACK, 3)])
        for max_out in (4096, 1 << 40):
            assert raw_solid(pkg, own_gpu, mesh, 21, rule, out, max_out=max_out) == (ERR_CAP, 12345, 54321)
            assert f"{cells} cells" in last_error(pkg, own_gpu) and "2^31" in last_error(pkg, own_gpu)
        assert out.untouched_from(0)
    with pytest.raises(pkg.SvoError):
        pkg.mesh.voxelize_solid(own_gpu, roof, [[0, 1, 2]], 21, quantized=True)


def test_count_query_two_runs_and_no_triangles(pkg, own_gpu, whole7):
    vq, tris = join(tetra_soup(77, 6, 200), box_mesh((100, 100, 100), (3000, 2000, 1500)))
    mesh = Mesh(own_gpu, vq, tris)
    want = S.solid(vq, tris, 6, S.NONZERO)
    assert raw_solid(pkg, own_gpu, mesh, 6, S.NONZERO, max_out=0) == (0, len(want.cells), want.n_open)  # a query ignores max_out
    runs = []
    for _ in range(2):
        out = SentinelOut(own_gpu, [(len(want.cells) + SLACK, 3)])
        assert raw_solid(pkg, own_gpu, mesh, 6, S.NONZERO, out) == (0, len(want.cells), want.n_open)
        runs.append(out.host()[0])
    assert runs[0].tobytes() == runs[1].tobytes() and np.array_equal(runs[0][:len(want.cells)], want.cells)
    # n_open_out may be null
    assert raw_solid(pkg, own_gpu, mesh, 6, S.NONZERO, n_open=False) == (0, len(want.cells), 54321)
    # no triangles: success with 0, with and without an output, with and without vertices
    for v in (vq, np.zeros((0, 3))):
        empty = Mesh(own_gpu, v, np.zeros((0, 3)))
        out = SentinelOut(own_gpu, [(SLACK, 3)])
        assert raw_solid(pkg, own_gpu, empty, 6, 0, out) == (0, 0, 0) and raw_solid(pkg, own_gpu, empty, 6, S.SPANS) == (0, 0, 0)
        assert out.untouched_from(0)
    # the public call
    for rule, flag in (("evenodd", S.EVENODD), ("nonzero", S.NONZERO)):
        ref = S.solid(vq, tris, 6, flag)
        cells, n_open = pkg.mesh.voxelize_solid(own_gpu, vq, tris, 6, rule, with_open=True, quantized=True)
        spans = pkg.mesh.voxelize_solid(own_gpu, vq, tris, 6, rule, spans=True, quantized=True)
        assert cells.dtype == spans.dtype and cells.dtype.is_signed and n_open == ref.n_open
        assert np.array_equal(cells.cpu().numpy().view(np.uint32), ref.cells) and np.array_equal(spans.cpu().numpy().view(np.uint32), ref.spans)
    assert pkg.mesh.voxelize_solid(own_gpu, vq, np.zeros((0, 3), dtype=np.int32), 6, quantized=True).shape == (0, 3)
    assert pkg.mesh.voxelize_solid(own_gpu, vq, np.zeros((0, 3), dtype=np.int32), 6, spans=True, quantized=True).shape == (0, 4)
    with pytest.raises(ValueError):
        pkg.mesh.voxelize_solid(own_gpu, vq, tris, 6, "winding", quantized=True)


def test_errors_in_their_order_write_nothing(pkg, own_gpu):
    vq, tris = join(tetra_soup(5, 5, 40), box_mesh((64, 64, 64), (1500, 1200, 1900)))
    levels = []
    want = S.solid(vq, tris, 5, levels=levels)
    count = len(want.cells)
    mesh = Mesh(own_gpu, vq, tris)
    out = SentinelOut(own_gpu, [(count + SLACK, 3)])

    def refused(code, part, mesh=mesh, depth=5, flags=0, **kw):
        got = raw_solid(pkg, own_gpu, mesh, depth, flags, kw.pop("out", out), **kw)
        return got == (code, 12345, 54321) and part in last_error(pkg, own_gpu)

    # every cause alone, then with the next one in the contract's order: the earlier one is reported
    assert refused(ERR_ARG, "null params", params=False)
    assert refused(ERR_ARG, "null params", params=False, n_out=False)
    assert refused(ERR_ARG, "null n_out", n_out=False)
    assert refused(ERR_ARG, "null n_out", n_out=False, flags=4)
    for flags in (4, 1 << 31, 8 | S.SPANS):
        assert refused(ERR_ARG, "flag", flags=flags)
    assert refused(ERR_ARG, "flag", flags=4, reserved=1)
    assert refused(ERR_ARG, "reserved", reserved=1)
    assert refused(ERR_ARG, "reserved", reserved=7, depth=0)
    for depth in (0, 22):
        assert refused(ERR_ARG, "depth", depth=depth)
    assert refused(ERR_ARG, "depth", depth=22, n_tris=1 << 31)
    assert refused(ERR_ARG, "n_tris", n_tris=1 << 31)
    assert refused(ERR_ARG, "n_tris", n_tris=1 << 40, vq=False)
    assert refused(ERR_ARG, "vq_dev", vq=False)
    assert refused(ERR_ARG, "vq_dev", vq=False, tris=False)
    assert refused(ERR_ARG, "tri_dev", tris=False)
    # on the device: the first triangle with a vertex index that is no vertex, or with a coordinate outside the grid
    bad = tris.copy()
    bad[7, 1] = len(vq)
    bad[3, 2] = 0x7FFFFFFF
    bad_index = Mesh(own_gpu, vq, bad)
    assert refused(ERR_ARG, "triangle 3 has a vertex index", mesh=bad_index)
    assert refused(ERR_ARG, "triangle 3 has a vertex index", mesh=bad_index, out=None)
    assert refused(ERR_ARG, "triangle 3 has a vertex index", mesh=bad_index, max_pairs=1)  # before the caps
    far = vq.copy()
    far[tris[5, 0], 2] = 1 << 11  # = 2^(depth + 6): the first coordinate outside
    at = int(np.flatnonzero((tris == tris[5, 0]).any(axis=1)).min())
    assert refused(ERR_ARG, f"triangle {at} has a coordinate", mesh=Mesh(own_gpu, far, tris))
    bad = tris.copy()
    bad[at + 1] = len(vq) + 5
    assert refused(ERR_ARG, f"triangle {at} has a coordinate", mesh=Mesh(own_gpu, far, bad), flags=S.SPANS)
    with pytest.raises(pkg.SvoError):
        pkg.mesh.voxelize_solid(own_gpu, far, tris, 5, quantized=True)
    # a level over max_pairs: the first such level, with its count
    assert all(a <= b for a, b in zip(levels[:-1], levels[1:-1])) and levels[1] > levels[0]
    stopped = S.solid(vq, tris, 5, max_pairs=levels[1] - 1)
    assert stopped == S.Stopped(2, levels[1])
    assert refused(ERR_CAP, f"level 2 has {levels[1]} ", max_pairs=levels[1] - 1)
    assert refused(ERR_CAP, f"level 2 has {levels[1]} ", max_pairs=levels[1] - 1, max_out=0)
    assert levels[4] > levels[3]  # so that the cap below stops the last level, the crossings, and none before it
    assert refused(ERR_CAP, f"level 5 has {levels[4]} crossings", max_pairs=levels[4] - 1)
    assert raw_solid(pkg, own_gpu, mesh, 5, 0, max_pairs=max(levels))[:2] == (0, count)
    # room for one entry less than there are, cells and spans
    assert refused(ERR_CAP, f"{count} cells", max_out=count - 1)
    assert refused(ERR_CAP, f"{count} cells", max_out=0)
    spans_out = SentinelOut(own_gpu, [(len(want.spans) + SLACK, 4)])
    assert refused(ERR_CAP, f"{len(want.spans)} spans", flags=S.SPANS, out=spans_out, max_out=len(want.spans) - 1)
    assert re.search(r"max_out = \d+", last_error(pkg, own_gpu))
    assert out.untouched_from(0) and spans_out.untouched_from(0)
    assert raw_solid(pkg, own_gpu, mesh, 5, 0, out, max_out=count) == (0, count, want.n_open) and out.untouched_from(count)


def test_the_node_buffer_is_never_touched_and_timing(pkg, own_gpu):
    render = pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)
    rng = np.random.default_rng(3)
    base = B.build(rng.integers(0, 64, (2000, 3)), 6, rng.integers(1, 1 << 24, 2000))
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    assert np.array_equal(before[base.size:], poison(PAD))
    vq, tris = tetra_soup(9, 6, 100)
    cells = pkg.mesh.voxelize_solid(own_gpu, vq, tris, 6, quantized=True)
    assert np.array_equal(cells.cpu().numpy().view(np.uint32), S.solid(vq, tris, 6).cells)
    assert np.array_equal(render.read_nodes(base.size + PAD), before) and render.node_length == base.size
    ms = own_gpu.solid_timing()
    assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[5] > 0 and ms[4] > 0
    assert ms == own_gpu.solid_timing()
    assert raw_solid(pkg, own_gpu, Mesh(own_gpu, vq, tris), 0)[0] == ERR_ARG  # a refused call leaves the times
    assert raw_solid(pkg, own_gpu, Mesh(own_gpu, vq, tris), 6, max_pairs=1)[0] == ERR_CAP
    assert ms == own_gpu.solid_timing()
    # a context with no node buffer voxelises; one that has not, has no times
    fresh = pkg.Gpu(0)
    try:
        with pytest.raises(pkg.SvoError):
            fresh.solid_timing()
        spans = pkg.mesh.voxelize_solid(fresh, vq, tris, 6, "nonzero", spans=True, quantized=True)
        assert np.array_equal(spans.cpu().numpy().view(np.uint32), S.solid(vq, tris, 6, S.NONZERO).spans)
        assert fresh.solid_timing()[5] > 0
    finally:
        fresh.close()


def test_a_solid_model_end_to_end(pkg, own_gpu):
    import torch
    v, t = pkg.mesh.icosphere(2, 0.6, (0.05, -0.1, 0.2))
    colours = 0x010000 + np.arange(len(t))
    fill = 0x00BEEF
    assert fill not in set(colours.tolist())
    render = pkg.Render.from_mesh(own_gpu, (64, 64), v, t, 7, colours, capacity=1 << 22, solid=True, fill_colour=fill)
    shell, shell_colours = pkg.mesh.voxelize(own_gpu, v, t, 7, colours)
    inner = pkg.mesh.voxelize_solid(own_gpu, v, t, 7)
    both = torch.cat([inner, shell]).cpu().numpy().astype(np.int64)
    distinct = np.unique(B.morton(both, 7))
    listed, listed_colours = render.list_voxels(7)
    assert len(listed) == len(distinct) and len(inner) > len(shell) // 2
    assert np.array_equal(B.morton(listed.cpu().numpy().astype(np.int64), 7), distinct)
    # the ball's centre holds the fill colour; the surface keeps its triangles' colours
    centre = np.floor((np.array([0.05, -0.1, 0.2]) + 1.0) * 64).astype(np.int64)
    assert render.sample_voxels(centre[None, :], 7).tolist() == [fill]
    assert (listed_colours == fill).sum().item() > 0 and set(shell_colours.cpu().tolist()) >= set(listed_colours[listed_colours != fill].cpu().tolist())
    # the seal: no interior voxel shows a face
    surface_colours = render.list_surface(7)[1]
    assert len(surface_colours) > 0 and not (surface_colours == fill).any().item()
    # an open mesh is refused unless allowed, and the defaults still build the shell alone
    with pytest.raises(ValueError):
        render.build_nodes_mesh(v, t[:-1], 7, colours[:-1], solid=True)
    assert render.build_nodes_mesh(v, t[:-1], 7, colours[:-1], solid=True, allow_open=True) > 8
    render.build_nodes_mesh(v, t, 7, colours)
    assert len(render.list_voxels(7)[0]) == len(np.unique(B.morton(shell.cpu().numpy().astype(np.int64), 7)))
