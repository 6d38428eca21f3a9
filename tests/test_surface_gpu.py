"""The visible surface found on the GPU (csrc/svo_surface.hip): the three modes, with the open and the
closed boundary, against the sequential restatement (tests/surface_ref.py) on the smallest trees, a depth-21 pair whose
carry crosses every level, a solid block, a filled ball, the edited depth-7 tree with counter bits and the mixed-level
tree; the count query agrees with the fill, nothing is written behind n, on any error or to the node buffer; the same
bytes for every layout and run; a tree rebuilt from the surface alone shows the same image; the mesh made on the GPU
equals the reference quads meshed on the CPU."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import surface_ref as S
from pass_frame import SLACK, SentinelOut, last_error, own_gpu, tree7_base  # noqa: F401
from test_compact_host import malformed_cases
from test_edit_gpu import CAPACITY, PAD, ROOT, frame, set_base
from test_list_gpu import value_image
from test_list_host import full_root, mixed_levels
from test_surface_host import ball

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_CAP = -1, -3, -6
CLOSED, KEEP, QUADS = S.CLOSED_BOUNDARY, S.KEEP_HIDDEN, S.QUADS
MODES = (0, KEEP, QUADS)
NAMES = ("xyz", "value", "level", "face")


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), ROOT, capacity=CAPACITY)


@pytest.fixture(scope="module")
def ball6(render):
    """the filled ball of radius 20 at depth 6, built on the GPU from its dense grid: (grid, words, reference masks with
    the open boundary)"""
    grid = ball(64, 20)
    render.build_nodes_dense(grid)
    words = render.read_nodes()
    entries = S.face_masks(words, words.size, 6)
    bits = np.array([bin(int(m)).count("1") for m in entries[3]])
    assert (bits == 0).sum() >= 1000 and ((bits >= 1) & (bits <= 5)).sum() >= 1000
    return grid, words, entries


class Out(SentinelOut):
    """sentinel-filled device outputs of `room` entries"""

    def __init__(self, gpu, room, levels=True):
        super().__init__(gpu, [(room, 3), room, room if levels else None, room])
        self.xyz, self.value, self.level, self.face = self.t
        self.room = room


def raw_surface(pkg, gpu, flags, depth, n_words, out=None, max_entries=None, params=True, n_out=True, value=True, face=True):
    p = pkg._lib.SurfaceParams()
    p.flags, p.depth, p.n_words = flags, depth, n_words
    p.max_entries = (out.room if out is not None else 0) if max_entries is None else max_entries
    n = C.c_uint64(12345)
    ptr = lambda t, given=True: t.data_ptr() if out is not None and given and t is not None else None  # noqa: E731
    rc = pkg._lib.lib().svo_nodes_list_surface(
        gpu._h, C.byref(p) if params else None, ptr(out and out.xyz), ptr(out and out.value, value), ptr(out and out.level),
        ptr(out and out.face, face), C.byref(n) if n_out else None)
    gpu.sync()
    return rc, n.value


def check_surface(pkg, render, words, depth, what, entries=None, loaded=False, closed=(False, True)):
    """the three modes of the words' surface on the GPU == the reference, for each boundary; the count query agrees and
    writes nothing; nothing is written behind n; the node buffer reads back unchanged.  `entries`: face_masks' result for
    the open boundary, when the caller has it.  Returns {flags: the four host arrays}."""
    if not loaded:
        set_base(render, words)
    before = render.read_nodes(words.size + PAD)
    assert np.array_equal(before[:words.size], words)
    got = {}
    for shut in closed:
        ref = entries if entries is not None and not shut else S.face_masks(words, words.size, depth, shut)
        for mode in MODES:
            flags = mode | (CLOSED if shut else 0)
            want = S.select(ref, flags)
            name = f"{what}, flags {flags}"
            rc, n = raw_surface(pkg, render.gpu, flags, depth, words.size)
            assert rc == 0, f"{name}: count query: status {rc}: {last_error(pkg, render.gpu)}"
            assert n == want[1].size, f"{name}: count {n}, want {want[1].size}"
            out = Out(render.gpu, n + SLACK)
            rc, m = raw_surface(pkg, render.gpu, flags, depth, words.size, out)
            assert rc == 0, f"{name}: status {rc}: {last_error(pkg, render.gpu)}"
            assert m == n, f"{name}: the fill's n {m}, the count query's {n}"
            host = out.host()
            for g, w, field in zip(host, want, NAMES):
                if not np.array_equal(g[:n], w):
                    bad = np.flatnonzero((g[:n] != w).reshape(n, -1).any(axis=1))
                    raise AssertionError(f"{name}: {bad.size} entries differ in {field}, first at {bad[:3]}: got {g[bad[:3]]} want {w[bad[:3]]}")
            assert out.untouched_from(n), f"{name}: written behind n"
            got[flags] = tuple(g[:n] for g in host)
    assert np.array_equal(render.read_nodes(words.size + PAD), before), f"{what}: the node buffer was written"
    return got


def test_smallest_trees(pkg, render):
    for depth in (1, 21):
        got = check_surface(pkg, render, ROOT, depth, f"empty root, depth {depth}")
        assert all(g[1].size == 0 for g in got.values())
    set_base(render, ROOT)
    assert [t.shape for t in render.list_surface(5, with_levels=True)] == [(0, 3), (0,), (0,), (0,)]
    full = full_root()
    outward = np.array([1 << (c >> 2 & 1) | 4 << (c >> 1 & 1) | 16 << (c & 1) for c in range(8)], dtype=np.uint32)
    for depth in (1, 21):
        got = check_surface(pkg, render, full, depth, f"full root, depth {depth}")
        assert np.array_equal(got[0][3], outward) and np.array_equal(got[KEEP][3], outward) and got[QUADS][3].size == 24
        assert got[CLOSED][1].size == 0 and got[CLOSED | QUADS][1].size == 0 and not got[CLOSED | KEEP][3].any()
        assert got[CLOSED | KEEP][3].size == 8


def test_depth_21_pair_whose_carry_crosses_every_level(pkg, render):
    half = 1 << 20
    cells = [[half - 1, 5, 1234567], [half, 5, 1234567]]
    for axis in range(3):  # the pair along x, y and z
        turned = [c[-axis:] + c[:-axis] if axis else c for c in cells]
        words = B.build(turned, 21, [0x00FF00, 0x0000FF])
        got = check_surface(pkg, render, words, 21, f"depth 21 pair along axis {axis}")
        xyz, value, level, face = got[KEEP]
        order = np.argsort(xyz[:, axis])
        assert xyz[order].tolist() == turned and (level == 21).all()
        assert face[order].tolist() == [63 & ~(2 << 2 * axis), 63 & ~(1 << 2 * axis)]  # each hides one face of the other
        assert got[QUADS][3].size == 10


def test_solid_block_astride_the_centre(pkg, render):
    cells = np.stack(np.meshgrid(*[np.arange(6, 10)] * 3, indexing="ij"), -1).reshape(-1, 3)
    words = B.build(cells, 4, np.arange(1, 65))
    got = check_surface(pkg, render, words, 4, "solid block")
    assert got[0][1].size == 56 and got[KEEP][1].size == 64 and got[QUADS][1].size == 6 * 16
    inner = (got[KEEP][0] >= 7).all(axis=1) & (got[KEEP][0] <= 8).all(axis=1)
    assert inner.sum() == 8 and not got[KEEP][3][inner].any() and got[KEEP][3][~inner].all()
    set_base(render, words)
    listed = render.list_voxels(4, with_levels=True)
    kept = render.list_surface(4, keep_hidden=True, with_levels=True)
    for a, b in zip(listed, (kept[0], kept[1], kept[3])):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    coords, colours, masks = render.list_surface(4)
    assert coords.shape == (56, 3) and masks.dtype == coords.dtype and bool((masks > 0).all())


def test_ball_more_groups_than_a_scan_tile(pkg, render, ball6):
    grid, words, entries = ball6
    got = check_surface(pkg, render, words, 6, "ball", entries)
    assert got[0][1].size < got[KEEP][1].size == (grid != 0).sum()


def test_edited_tree_with_counter_bits(pkg, render):
    words = tree7_base()["words"]
    counted = words | np.random.default_rng(6).integers(0, 16, words.size).astype(np.uint32)
    check_surface(pkg, render, counted, 7, "edited depth 7 with counters")


def test_mixed_levels(pkg, render):
    mixed = mixed_levels()
    got = check_surface(pkg, render, mixed, 6, "mixed levels")
    assert set(got[KEEP][2].tolist()) == {2, 3, 4, 5, 6}
    check_surface(pkg, render, mixed, 8, "mixed levels on the depth-8 grid", closed=(False,))


def test_every_layout_and_every_run_list_identically(pkg, render):
    words = tree7_base()["words"]
    entries = S.face_masks(words, words.size, 7)
    put = check_surface(pkg, render, words, 7, "edited, put order", entries, closed=(False,))
    again = check_surface(pkg, render, words, 7, "edited, second run", entries, loaded=True, closed=(False,))
    same = lambda a, b: all(x.tobytes() == y.tobytes() for mode in MODES for x, y in zip(a[mode], b[mode]))  # noqa: E731
    assert same(put, again)
    for prune in (False, True):
        set_base(render, words)
        render.compact_nodes(prune=prune)
        layout = render.read_nodes()
        assert same(put, check_surface(pkg, render, layout, 7, f"compacted, prune {prune}", entries, closed=(False,)))


def test_hollowing_preserves_the_image(pkg, render, ball6, O):
    grid, words, _ = ball6
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)  # (the camera stands outside the grid)
    set_base(render, words)
    solid = frame(pkg, render, u)
    coords, colours, masks = render.list_surface(6)
    assert render.build_nodes(coords, 6, colours) < words.size
    hollow, hollow_words = frame(pkg, render, u), render.read_nodes()
    assert (solid["value"] < words.size).sum() > 300  # (a disc of about 14 pixels' radius)
    assert np.array_equal(value_image(solid, words), value_image(hollow, hollow_words))
    assert np.array_equal(solid["t"], hollow["t"])


def test_errors_write_nothing(pkg, render, own_gpu):
    base = tree7_base()["base"]
    set_base(render, base)
    before = render.read_nodes(base.size + PAD)
    entries = S.face_masks(base, base.size, 7)
    count = S.select(entries, 0)[1].size
    out = Out(own_gpu, count + SLACK)
    refused = lambda code, part, *a, **kw: (raw_surface(pkg, own_gpu, *a, **kw) == (code, 12345)  # noqa: E731
                                            and part in last_error(pkg, own_gpu))
    # the contract's order: each call has every later cause too
    assert refused(ERR_ARG, "null params", 8, 0, 12, out, params=False, n_out=True, value=False)
    assert refused(ERR_ARG, "null n_out", 8, 0, 12, out, n_out=False, value=False)
    assert refused(ERR_ARG, "unknown or incompatible flag bits", 8, 0, 12, out, value=False)
    assert refused(ERR_ARG, "unknown or incompatible flag bits", QUADS | KEEP, 0, 12, out, value=False)
    assert refused(ERR_ARG, "unknown or incompatible flag bits", 1 << 31, 7, base.size, out)
    for depth in (0, 22):
        assert refused(ERR_ARG, "depth", 0, depth, 12, out, value=False)
    assert refused(ERR_ARG, "null face_out_dev or value_out_dev", 0, 7, 12, out, value=False)
    assert refused(ERR_ARG, "null face_out_dev or value_out_dev", 0, 7, 12, out, face=False)
    for n in (0, 12, base.size + 4, CAPACITY + 8):
        assert refused(ERR_ARG, "n_words", 0, 6, n, out)
    # the tree is deeper than depth
    for flags in (0, KEEP, QUADS | CLOSED):
        assert refused(ERR_ARG, "level 7", flags, 6, base.size, out, max_entries=0)
        assert refused(ERR_ARG, "level 7", flags, 6, base.size)
    with pytest.raises(pkg.SvoError):
        render.list_surface(3)
    with pytest.raises(pkg.SvoError):
        render.surface_quads(3)
    # room for one entry less than there are; a count query does not look at max_entries
    assert refused(ERR_CAP, f"{count} entries", 0, 7, base.size, out, max_entries=count - 1)
    quads = S.select(entries, QUADS)[1].size
    assert refused(ERR_CAP, f"{quads} entries", QUADS, 7, base.size, out, max_entries=count)
    assert raw_surface(pkg, own_gpu, 0, 7, base.size, max_entries=0) == (0, count)
    assert out.untouched_from(0)
    assert np.array_equal(render.read_nodes(base.size + PAD), before)

    causes = {"a pointer with pointer + 8 > n_words": "leaves the first n_words", "an unaligned pointer": "not a multiple of 8",
              "two parents sharing one group": "reached twice", "a cycle through the root": "reached twice", "32 levels": "deeper than 31"}
    cases = malformed_cases()
    assert set(cases) == set(causes)
    for name, words in cases.items():
        set_base(render, words)
        before = render.read_nodes(words.size + PAD)
        for flags in MODES:
            for o in (out, None):
                assert raw_surface(pkg, own_gpu, flags, 21, words.size, o, max_entries=0) == (ERR_STATE, 12345), name
                assert "malformed tree: " in last_error(pkg, own_gpu) and causes[name] in last_error(pkg, own_gpu), f"{name}: {last_error(pkg, own_gpu)}"
        assert np.array_equal(render.read_nodes(words.size + PAD), before), name
    assert out.untouched_from(0)

    fresh = pkg.Gpu(0)
    try:
        assert raw_surface(pkg, fresh, 0, 7, 12)[0] == ERR_STATE and "svo_nodes_alloc" in last_error(pkg, fresh)
    finally:
        fresh.close()


def test_timing(pkg, render, own_gpu):
    base = tree7_base()["base"]
    set_base(render, base)
    render.list_surface(7)
    ms = own_gpu.surface_timing()
    assert len(ms) == 7 and all(t >= 0 for t in ms) and all(t > 0 for t in ms[:6]) and ms[6] > 0
    assert ms == own_gpu.surface_timing()
    assert raw_surface(pkg, own_gpu, 0, 3, base.size)[0] == ERR_ARG  # a refused call leaves the times
    assert ms == own_gpu.surface_timing()


def test_mesh_on_the_gpu_equals_the_reference_quads_meshed_on_the_cpu(pkg, render):
    import torch
    mixed = mixed_levels()
    set_base(render, mixed)
    for closed in (False, True):
        xyz, value, level, face = S.list_surface(mixed, mixed.size, 6, QUADS | (CLOSED if closed else 0))
        for weld in (True, False):
            got = pkg.mesh.extract_surface(render, 6, closed_boundary=closed, weld=weld)
            want = pkg.mesh.quads_to_mesh(*[torch.from_numpy(a.astype(np.int32)) for a in (xyz, face, level)], 6,
                                          torch.from_numpy(value.astype(np.int32)), weld=weld)
            assert all(g.is_cuda for g in got) and got[0].dtype == torch.float32
            for g, w, name in zip(got, want, ("vertices", "triangles", "colours")):
                assert g.dtype == w.dtype and g.cpu().numpy().tobytes() == w.numpy().tobytes(), f"closed {closed}, weld {weld}: {name}"
