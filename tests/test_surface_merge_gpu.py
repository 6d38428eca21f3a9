"""The visible surface merged into rectangles on the GPU (csrc/svo_surface_merge.hip), byte for byte against
the contract's numpy restatement (tests/surface_merge_ref.py: merge_rects): every case of test_surface_merge_host.py with
both boundaries, one and two rounds, with and without any_value; the count query agrees with the fill, nothing is written
behind n, on any error or to the node buffer; the same bytes for every layout and run; runs that cross scan tiles along
each axis; a slab whose V phase leaves one run; extents of 2^21; the errors in the header's order; the merged mesh made on
the GPU; the default extract_surface as before; the pass behind a carve and a simplification on one context."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import surface_merge_ref as M
import surface_ref as S
from pass_frame import SLACK, SentinelOut, last_error, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, PAD, ROOT, set_base
from test_surface_host import ball
from test_surface_merge_host import cases, merged, quads_of, signed_volume_x6, tensors

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_CAP = -1, -3, -6
CLOSED, ANY_VALUE = 1, 8
VARIANTS = tuple((closed, rounds, any_value) for closed in (False, True) for rounds in (1, 2) for any_value in (False, True))


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


class Out(SentinelOut):
    """sentinel-filled device outputs of `room` entries"""

    def __init__(self, gpu, room):
        super().__init__(gpu, [(room, 6), room])
        self.rects, self.values = self.t
        self.room = room


def raw_merge(pkg, gpu, flags, depth, rounds, n_words, out=None, max_entries=None, params=True, n_out=True, value=True):
    p = pkg._lib.SurfaceMergeParams()
    p.flags, p.depth, p.rounds, p.n_words = flags, depth, rounds, n_words
    p.reserved = 0xDEAD  # (not looked at)
    p.max_entries = (out.room if out is not None else 0) if max_entries is None else max_entries
    n = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_nodes_merge_surface(
        gpu._h, C.byref(p) if params else None, out.rects.data_ptr() if out is not None else None,
        out.values.data_ptr() if out is not None and value else None, C.byref(n) if n_out else None)
    gpu.sync()
    return rc, n.value


def check_merge(pkg, render, words, depth, what, want_of, variants=VARIANTS, loaded=False):
    """the words' merged surface on the GPU == want_of(closed, rounds, any_value), byte for byte, for each variant; the
    count query agrees and writes nothing; nothing is written behind n; the node buffer reads back unchanged.  Returns
    {variant: (rects, values)}."""
    if not loaded:
        set_base(render, words)
    before = render.read_nodes(words.size + PAD)
    assert np.array_equal(before[:words.size], words)
    got = {}
    for variant in variants:
        closed, rounds, any_value = variant
        flags = (CLOSED if closed else 0) | (ANY_VALUE if any_value else 0)
        want = want_of(closed, rounds, any_value)
        name = f"{what}, closed {closed}, rounds {rounds}, any_value {any_value}"
        rc, n = raw_merge(pkg, render.gpu, flags, depth, rounds, words.size)
        assert rc == 0, f"{name}: count query: status {rc}: {last_error(pkg, render.gpu)}"
        assert n == len(want[0]), f"{name}: count {n}, want {len(want[0])}"
        out = Out(render.gpu, n + SLACK)
        rc, m = raw_merge(pkg, render.gpu, flags, depth, rounds, words.size, out)
        assert rc == 0, f"{name}: status {rc}: {last_error(pkg, render.gpu)}"
        assert m == n, f"{name}: the fill's n {m}, the count query's {n}"
        host = out.host()
        for g, w, field in zip(host, want, ("rects", "values")):
            if g[:n].tobytes() != np.ascontiguousarray(w, dtype=np.uint32).tobytes():
                bad = np.flatnonzero((g[:n] != w).reshape(n, -1).any(axis=1))
                raise AssertionError(f"{name}: {bad.size} entries differ in {field}, first at {bad[:3]}: got {g[bad[:3]].tolist()} want {w[bad[:3]].tolist()}")
        assert out.untouched_from(n), f"{name}: written behind n"
        got[variant] = tuple(g[:n] for g in host)
    assert np.array_equal(render.read_nodes(words.size + PAD), before), f"{what}: the node buffer was written"
    return got


def reference_of(words, depth):
    """want_of for words that are no case of the host tests: the reference quads once per boundary"""
    quads = {}

    def want(closed, rounds, any_value):
        if closed not in quads:
            quads[closed] = S.list_surface(words, words.size, depth, S.QUADS | (S.CLOSED_BOUNDARY if closed else 0))
        return M.merge_rects(quads[closed], depth, rounds, any_value)
    return want


@pytest.mark.parametrize("name", sorted(cases()))
def test_host_cases_on_the_device(pkg, render, name):
    words, depth, _ = cases()[name]
    got = check_merge(pkg, render, words, depth, name, lambda *variant: merged(name, *variant))
    if name == "empty":
        assert all(len(g[1]) == 0 for g in got.values())
        assert [tuple(t.shape) for t in render.surface_rects(5)] == [(0, 6), (0,)]
        ms = render.gpu.surface_merge_timing()
        assert not any(ms[1:33]), "a phase ran on no rectangles"
    if name == "uniform root at depth 21":  # extents of 2^21 through the key fields
        side = 1 << 21
        assert got[(False, 1, False)][0].tolist() == [[f, (f & 1) * side, 0, 0, side, side] for f in range(6)]
        assert len(got[(True, 1, False)][1]) == 0
    if name == "second round":
        assert len(got[(False, 2, False)][1]) < len(got[(False, 1, False)][1])
    if name == "ball":
        assert len(got[(False, 1, True)][1]) < len(got[(False, 1, False)][1]) / 2


def test_every_layout_and_every_run_merge_identically(pkg, render):
    words = tree7_base()["words"]
    counted = words | np.random.default_rng(28).integers(0, 16, words.size).astype(np.uint32)
    want = reference_of(words, 7)
    variants = ((False, 2, False), (False, 1, True))
    put = check_merge(pkg, render, counted, 7, "edited with counters, put order", want, variants)
    again = check_merge(pkg, render, counted, 7, "second run", want, variants, loaded=True)
    same = lambda a, b: all(x.tobytes() == y.tobytes() for v in variants for x, y in zip(a[v], b[v]))  # noqa: E731
    assert same(put, again)
    set_base(render, words)
    render.compact_nodes(prune=True)
    assert same(put, check_merge(pkg, render, render.read_nodes(), 7, "compacted", want, variants))


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_runs_across_scan_tiles(pkg, render, axis):
    """a line of 5 000 unit voxels: about 20 000 quads, so a long side's run spans more than one 4 096-item tile; along
    each axis in turn it is a run of the U phase for one pair of faces and of the V phase for the other"""
    coords = np.full((5000, 3), 4000, dtype=np.int64)
    coords[:, axis] = 100 + np.arange(5000)
    words = B.build(coords, 13, colour=0x4488CC)
    got = check_merge(pkg, render, words, 13, f"line along axis {axis}", reference_of(words, 13), ((False, 1, False), (True, 2, True)))
    rects = got[(False, 1, False)][0].astype(np.int64)
    assert len(rects) == 6
    for f, plane, u0, v0, w, h in rects.tolist():
        a = f >> 1
        if a == axis:  # the two ends
            assert (plane, u0, v0, w, h) == (100 + (f & 1) * 5000, 4000, 4000, 1, 1)
        else:  # the long sides: the line runs along u where u's axis (a + 1) % 3 is the line's, else along v
            along_u = (a + 1) % 3 == axis
            assert plane == 4000 + (f & 1)
            assert (u0, v0, w, h) == ((100, 4000, 5000, 1) if along_u else (4000, 100, 1, 5000))


def test_a_slab_whose_rows_become_one_rectangle(pkg, render):
    grid = np.zeros((64, 64, 64), dtype=np.int64)
    grid[:, 20, :] = 0x77AA33
    render.build_nodes_dense(grid)
    words = render.read_nodes()
    got = check_merge(pkg, render, words, 6, "slab", reference_of(words, 6), ((False, 1, False), (True, 1, False)), loaded=True)
    want = M.greedy_dense(grid, False)
    assert got[(False, 1, False)][0].tolist() == want[0].tolist() and len(want[0]) == 6
    assert got[(True, 1, False)][0].tolist() == [[2, 20, 0, 0, 64, 64], [3, 21, 0, 0, 64, 64]]


def test_errors_write_nothing(pkg, render, own_gpu):
    base = tree7_base()["base"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    count = len(M.merge_rects(S.list_surface(base, base.size, 7, S.QUADS), 7)[0])
    out = Out(own_gpu, count + SLACK)
    refused = lambda code, part, *a, **kw: (raw_merge(pkg, own_gpu, *a, **kw) == (code, 12345)  # noqa: E731
                                            and part in last_error(pkg, own_gpu))
    # the contract's order: each call has every later cause too
    assert refused(ERR_ARG, "null params", 2, 0, 0, 12, out, params=False, value=False)
    assert refused(ERR_ARG, "null n_out", 2, 0, 0, 12, out, n_out=False, value=False)
    for flags in (2, 4, 16, 1 << 31):  # (KEEP_HIDDEN and QUADS are the surface call's)
        assert refused(ERR_ARG, "unknown or incompatible flag bits", flags, 0, 1, 12, out, value=False)
    for rounds in (0, 5, 1 << 31):
        assert refused(ERR_ARG, "unknown or incompatible flag bits", 0, 0, rounds, 12, out, value=False)
    for depth in (0, 22):
        assert refused(ERR_ARG, "depth", 0, depth, 1, 12, out, value=False)
    assert refused(ERR_ARG, "null value_out_dev", 0, 7, 1, 12, out, value=False)
    for n in (0, 12, base.size + 4, CAPACITY + 8):
        assert refused(ERR_ARG, "n_words", 0, 6, 1, n, out)
    # the tree is deeper than depth
    for flags in (0, CLOSED | ANY_VALUE):
        assert refused(ERR_ARG, "level 7", flags, 6, 2, base.size, out, max_entries=0)
        assert refused(ERR_ARG, "level 7", flags, 6, 2, base.size)
    with pytest.raises(pkg.SvoError):
        render.surface_rects(3)
    with pytest.raises(pkg.SvoError):
        render.surface_rects(7, rounds=5)
    # room for one entry less than there are; a count query does not look at max_entries
    assert refused(ERR_CAP, f"{count} entries", 0, 7, 1, base.size, out, max_entries=count - 1)
    assert refused(ERR_CAP, f"{count} entries", 0, 7, 1, base.size, out, max_entries=0)
    assert raw_merge(pkg, own_gpu, 0, 7, 1, base.size, max_entries=0) == (0, count)
    assert out.untouched_from(0)
    assert np.array_equal(render.read_nodes(base.size + PAD), before)

    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice", "32 levels": "deeper than 31"}
    found = malformed_cases()
    assert set(found) == set(causes)
    for name, words in found.items():
        set_base(render, words)
        before = render.read_nodes(words.size + PAD)
        for o in (out, None):
            assert raw_merge(pkg, own_gpu, 0, 21, 1, words.size, o, max_entries=0) == (ERR_STATE, 12345), name
            assert "malformed tree: " in last_error(pkg, own_gpu) and causes[name] in last_error(pkg, own_gpu), f"{name}: {last_error(pkg, own_gpu)}"
        assert np.array_equal(render.read_nodes(words.size + PAD), before), name
    assert out.untouched_from(0)

    fresh = pkg.Gpu(0)
    try:
        assert raw_merge(pkg, fresh, 0, 7, 1, 12)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
    finally:
        fresh.close()


def test_timing(pkg, render, own_gpu):
    words, depth, _ = cases()["second round"]
    set_base(render, words)
    rects, _ = render.surface_rects(depth, rounds=4)
    assert len(rects) == len(merged("second round", rounds=4)[0])
    ms = own_gpu.surface_merge_timing()
    assert len(ms) == 35 and all(t >= 0 for t in ms) and ms[0] > 0 and ms[34] > 0
    assert all(t > 0 for t in ms[1:25]), "rounds 1 and 2 joined something, so round 3 ran"
    assert not any(ms[25:33]), "a round ran after one that joined nothing"
    assert ms == own_gpu.surface_merge_timing()
    assert raw_merge(pkg, own_gpu, 0, 1, 1, words.size)[0] == ERR_ARG  # a refused call leaves the times
    assert ms == own_gpu.surface_merge_timing()


def test_the_merged_mesh_on_the_gpu(pkg, render):
    import torch
    words, depth, grid = cases()["ball"]
    set_base(render, words)
    for closed, rounds in ((False, 1), (True, 2)):
        for weld in (True, False):
            got = pkg.mesh.extract_surface(render, depth, closed_boundary=closed, weld=weld, merge=True, rounds=rounds)
            want = pkg.mesh.rects_to_mesh(*tensors(*merged("ball", closed, rounds)), depth, weld=weld)
            assert all(g.is_cuda for g in got) and got[0].dtype == torch.float32
            for g, w, name in zip(got, want, ("vertices", "triangles", "colours")):
                assert g.dtype == w.dtype and g.cpu().numpy().tobytes() == w.numpy().tobytes(), f"closed {closed}, weld {weld}: {name}"
    rects, values = render.surface_rects(depth, any_value=True)
    vi, tri, _ = pkg.mesh.rects_to_mesh(rects, values, depth, integer=True)
    assert vi.is_cuda and signed_volume_x6(vi.cpu(), tri.cpu()) == 6 * int((grid != 0).sum())
    assert len(tri) < len(pkg.mesh.extract_surface(render, depth)[1]) / 2


def test_the_default_path_returns_what_it_returned(pkg, render):
    words, depth, _ = cases()["mixed levels"]
    set_base(render, words)
    for closed in (False, True):
        xyz, value, level, face = quads_of("mixed levels", closed)
        for got in (pkg.mesh.extract_surface(render, depth, closed), pkg.mesh.extract_surface(render, depth, closed, True, False, 3)):
            want = pkg.mesh.quads_to_mesh(*tensors(xyz, face, level), depth, tensors(value)[0])
            for g, w, name in zip(got, want, ("vertices", "triangles", "colours")):
                assert g.is_cuda and g.dtype == w.dtype and g.cpu().numpy().tobytes() == w.numpy().tobytes(), f"closed {closed}: {name}"


def test_behind_a_carve_and_a_simplification_on_one_context(pkg, render):
    import torch
    grid = np.where(ball(32, 11) != 0, 0x808080, 0)
    render.build_nodes_dense(grid)
    block = cases()["block"][0]  # the source's cube is the scene: cells of 4^3 scene cells each
    source = torch.from_numpy(block.view(np.int32).copy()).to(render.gpu.torch_device)
    render.combine_nodes(source, "carve", depth=5)
    carved = render.read_nodes()
    variants = ((False, 1, False), (False, 2, False), (True, 2, True))
    got = check_merge(pkg, render, carved, 5, "carved", reference_of(carved, 5), variants, loaded=True)
    assert 0 < len(got[(False, 1, False)][1]) < S.list_surface(carved, carved.size, 5, S.QUADS)[3].size / 2
    assert render.simplify_nodes() < carved.size
    simple = render.read_nodes()
    got = check_merge(pkg, render, simple, 5, "simplified", reference_of(simple, 5), variants, loaded=True)
    assert len(got[(False, 2, False)][1]) <= len(got[(False, 1, False)][1])
