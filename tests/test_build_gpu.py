"""Trees built on the GPU (csrc/svo_build.hip): word for word against the relayouted host tree of every
.vox fixture and against the numpy restatement (tests/build_ref.py) on random voxel sets; the same words for any order
of distinct voxels and on every run; dense grids; errors that leave the node buffer untouched; frames traced from built
trees against the oracle, also after a tree is replaced through a context that shares the buffer."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
from conftest import GOLDEN, assert_hits_equal, set_uniforms_from_oracle
from pass_frame import assert_words, own_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

CAPACITY = 40_000_000
ERR_ARG, ERR_STATE, ERR_CAP = -1, -3, -6


@pytest.fixture(scope="module")
def render(pkg, own_gpu):
    return pkg.Render(own_gpu, (64, 64), np.full(8, B.EMPTY, dtype=np.uint32), capacity=CAPACITY)


def gpu_build(render, coords, depth, colours=None, **kw):
    n = render.build_nodes(coords, depth, colours, **kw)
    return render.read_nodes(n)


def height_field(seed, depth, side, origin=(0, 0)):
    """one surface voxel per column of a side x side patch: a smooth seeded height around the middle of the cube"""
    rng = np.random.default_rng(seed)
    x, z = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    f = rng.uniform(0.5, 3.0, 4)
    h = (np.sin(x * f[0] / side * 6) + np.cos(z * f[1] / side * 6) + 0.5 * np.sin((x + z) * f[2] / side * 9)) * side / 16
    y = ((1 << depth) // 2 + h).astype(np.int64)
    coords = np.stack([x.ravel() + origin[0], y.ravel(), z.ravel() + origin[1]], 1)
    colours = (coords[:, 1] * 2654435761) & 0xFFFFFF
    return coords, colours


@pytest.mark.parametrize("name", B.FIXTURES)
def test_fixtures_equal_the_relayouted_host_tree(pkg, render, name):
    for label, size, xyzi, pal in B.fixture_models(GOLDEN, name):
        want = pkg.scenes.relayout(pkg.CpuOctree.from_voxels(size, xyzi, pal).to_octree_words(), block_level=32)
        coords, colours, depth = B.vox_voxels(size, xyzi, pal)
        assert_words(gpu_build(render, coords, depth, colours), want, label)


def random_case(rng, depth, n, dup=True):
    side = 1 << depth
    coords = rng.integers(0, side, (n, 3))
    if n >= 2:
        coords[0] = 0
        coords[1] = side - 1
    if dup and n >= 8:
        coords[n // 2: n // 2 + n // 4] = coords[: n // 4]  # duplicates: the later one wins
    colours = rng.integers(0, 1 << 32, n)
    colours[::7] = 0  # colour 0: empty leaves on existing paths
    colours[1::11] = 0xFF000000  # only high bits: colour 0 too
    return coords, colours


@pytest.mark.parametrize("depth", [1, 2, 5, 9, 12, 16, 21])
def test_random_sets_match_numpy(render, depth):
    rng = np.random.default_rng(100 + depth)
    for n in (0, 1, 2, 3, 100, 5000, 40000):
        coords, colours = random_case(rng, depth, n)
        assert_words(gpu_build(render, coords, depth, colours), B.build(coords, depth, colours), f"depth {depth}, n {n}")
        got = gpu_build(render, coords, depth, None, colour=0xABCDEF)
        assert_words(got, B.build(coords, depth, None, colour=0xABCDEF), f"depth {depth}, n {n}, one colour")


def test_millions_of_voxels_match_numpy(render, own_gpu):
    """every radix pass and multi-tile scans: 4 M voxels clustered in a 256^3 block of a depth-16 cube"""
    rng = np.random.default_rng(5)
    n = 4_000_000
    coords = rng.integers(0, 256, (n, 3)) + np.array([40000, 1000, 23456])
    coords[n - 100_000:] = coords[:100_000]
    colours = rng.integers(0, 1 << 24, n)
    got = gpu_build(render, coords, 16, colours)
    assert_words(got, B.build(coords, 16, colours), "4 M voxels")
    ms = own_gpu.build_timing()
    assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[1] > 0


def test_same_words_for_any_order_and_every_run(render):
    rng = np.random.default_rng(9)
    coords = np.unique(rng.integers(0, 1 << 12, (300_000, 3)), axis=0)
    colours = rng.integers(0, 1 << 24, coords.shape[0])
    first = gpu_build(render, coords, 12, colours)
    for _ in range(2):
        assert np.array_equal(gpu_build(render, coords, 12, colours), first)
    perm = rng.permutation(coords.shape[0])
    assert np.array_equal(gpu_build(render, coords[perm], 12, colours[perm]), first)
    assert_words(first, B.build(coords, 12, colours), "distinct voxels")


@pytest.mark.parametrize("depth", [6, 8])
def test_dense_grid_equals_the_sparse_build(render, depth):
    import torch
    rng = np.random.default_rng(depth)
    side = 1 << depth
    grid = np.where(rng.random((side, side, side)) < 0.2, rng.integers(1, 1 << 32, (side, side, side)), 0).astype(np.uint32)
    grid[0, 0, 0], grid[-1, -1, -1], grid[1, 2, 3] = 0x01000000, 0x00FFFFFF, 0  # colour 0 but non-zero: an empty leaf
    coords, colours = B.dense_to_voxels(grid)
    want = B.build(coords, depth, colours)
    n = render.build_nodes_dense(torch.from_numpy(grid.view(np.int32)).cuda(render.gpu.device))
    assert_words(render.read_nodes(n), want, f"dense depth {depth}")
    assert_words(gpu_build(render, coords, depth, colours), want, f"sparse depth {depth}")
    assert render.build_nodes_dense(np.zeros((side, side, side), dtype=np.uint32)) == 8
    assert np.array_equal(render.read_nodes(8), np.full(8, B.EMPTY, dtype=np.uint32))


def raw_build(pkg, gpu, xyz, depth, max_words=0, n=None):
    p = pkg._lib.BuildParams()
    p.depth, p.default_colour, p.max_words = depth, 0xFFFFFF, max_words
    out = C.c_uint64(12345)
    rc = pkg._lib.lib().svo_nodes_build(gpu._h, xyz.data_ptr() if xyz is not None else None, None,
                                        xyz.shape[0] if n is None else n, C.byref(p), C.byref(out))
    gpu.sync()
    return rc, out.value


def test_errors_leave_the_node_buffer_untouched(pkg, render, own_gpu):
    import torch
    sentinel = np.arange(0xDEAD0000, 0xDEAD0000 + 4096, dtype=np.uint32)
    render.write_nodes(sentinel)
    dev = torch.device("cuda", own_gpu.device)
    ok = torch.tensor([[1, 2, 3], [7, 7, 7]], dtype=torch.int32, device=dev)
    bad = torch.tensor([[1, 2, 3], [8, 0, 0]], dtype=torch.int32, device=dev)
    neg = torch.tensor([[1, 2, 3], [0, -1, 0]], dtype=torch.int32, device=dev)
    assert raw_build(pkg, own_gpu, bad, 3)[0] == ERR_ARG
    assert "outside" in pkg._lib.lib().svo_last_error(own_gpu._h).decode()
    assert raw_build(pkg, own_gpu, neg, 3)[0] == ERR_ARG
    assert raw_build(pkg, own_gpu, ok, 0)[0] == ERR_ARG
    assert raw_build(pkg, own_gpu, ok, 22)[0] == ERR_ARG
    assert raw_build(pkg, own_gpu, None, 3, n=5)[0] == ERR_ARG
    assert raw_build(pkg, own_gpu, ok, 3, n=1 << 31)[0] == ERR_ARG
    assert raw_build(pkg, own_gpu, ok, 3, max_words=23)[0] == ERR_CAP  # needs 8 + 8 * 2 + 8 * 2 = 40
    assert raw_build(pkg, own_gpu, ok[:0], 3, max_words=7)[0] == ERR_CAP
    with pytest.raises(pkg.SvoError):
        render.build_nodes(bad, 3)
    with pytest.raises(pkg.SvoError):
        render.build_nodes_dense(np.ones((4, 4, 4), dtype=np.uint32), max_words=16)
    assert np.array_equal(render.read_nodes(sentinel.size), sentinel)
    assert raw_build(pkg, own_gpu, ok, 3, max_words=40) == (0, 40)
    fresh = pkg.Gpu(0)
    try:
        assert raw_build(pkg, fresh, ok, 3)[0] == ERR_STATE
    finally:
        fresh.close()


def test_torch_and_numpy_inputs_give_the_same_words(render, own_gpu):
    import torch
    rng = np.random.default_rng(3)
    coords, colours = random_case(rng, 10, 20000)
    want = B.build(coords, 10, colours)
    dev = torch.device("cuda", own_gpu.device)
    for c in (coords, coords.astype(np.int32), coords.astype(np.uint32),
              torch.from_numpy(coords).to(dev), torch.from_numpy(coords).to(dev, torch.int32)):
        for col in (colours, torch.from_numpy(colours).to(dev), torch.from_numpy(colours & 0xFFFFFF).to(dev, torch.int32)):
            assert_words(gpu_build(render, c, 10, col), want, f"{type(c)} {getattr(c, 'dtype', None)} / {getattr(col, 'dtype', None)}")


def frame(pkg, O, r, u):
    set_uniforms_from_oracle(r, u)
    got = pkg.render.hits_to_numpy(r.render())
    r.gpu.sync()
    return got


def test_built_trees_trace_like_the_oracle(pkg, O, own_gpu, monu9_words):
    (label, size, xyzi, pal), = B.fixture_models(GOLDEN, "monu9")
    coords, colours, depth = B.vox_voxels(size, xyzi, pal)
    r = pkg.Render.from_voxels(own_gpu, (96, 96), coords, depth, colours, capacity=8_000_000)
    words = r.read_nodes()
    u = O.make_uniforms(width=96, height=96, flags=O.F_PAUSE_ADAPTIVE)
    got = frame(pkg, O, r, u)
    want = O.trace_frame(words, u, threads=4)
    assert_hits_equal(got, want, "monu9 built on the GPU")
    assert (want["info"] >> 16 & 1).sum() > 500
    # against the host-built tree: the same records but for the voxel index, which relayout's perm translates
    host = np.asarray(monu9_words)
    _, perm = pkg.scenes.relayout(host, 32, with_perm=True)
    hw = O.trace_frame(host, u, threads=4).reshape(-1)
    g = got.reshape(-1)
    for f in ("t", "info", "normal_bits"):
        assert np.array_equal(g[f].view(np.uint32), hw[f].view(np.uint32)), f
    real = g["value"] < words.size
    assert np.array_equal(perm[g["value"][real]], hw["value"][real]) and np.array_equal(g["value"][~real], hw["value"][~real])

    # a depth-16 height field seen from just above it
    coords, colours = height_field(1, 16, 1024)
    n = r.build_nodes(coords, 16, colours)
    u = O.make_uniforms(pos=(-0.984, 0.03, -0.984), look=(0.25, -1.0, 0.3), width=96, height=96, flags=O.F_PAUSE_ADAPTIVE)
    got = frame(pkg, O, r, u)
    want = O.trace_frame(r.read_nodes(n), u, threads=4)
    assert_hits_equal(got, want, "depth-16 height field")
    assert (want["info"] >> 16 & 1).sum() > 500


def test_replacing_the_tree_through_either_sharing_context(pkg, O, own_gpu, small_words):
    a = np.asarray(small_words)
    r1 = pkg.Render(own_gpu, (80, 80), a, capacity=2_000_000)
    g2 = pkg.Gpu(0)
    try:
        r2 = pkg.Render.share_nodes(g2, r1)
        u = O.make_uniforms(width=80, height=80, flags=O.F_PAUSE_ADAPTIVE)
        assert_hits_equal(frame(pkg, O, r1, u), O.trace_frame(a, u, threads=4), "tree A")
        rng = np.random.default_rng(11)
        coords = rng.integers(0, 64, (30000, 3))
        colours = rng.integers(0, 1 << 24, 30000)
        want_b = B.build(coords, 6, colours)
        hits_b = O.trace_frame(want_b, u, threads=4)
        assert (hits_b["value"] != O.trace_frame(a, u, threads=4)["value"]).any()
        assert r1.build_nodes(coords, 6, colours) == want_b.size  # the same context
        assert_hits_equal(frame(pkg, O, r1, u), hits_b, "tree B built on the rendering context")
        assert_hits_equal(frame(pkg, O, r2, u), hits_b, "tree B seen by the sharing context")
        r1.write_nodes(a)
        assert_hits_equal(frame(pkg, O, r2, u), O.trace_frame(a, u, threads=4), "tree A again")
        r2.build_nodes(coords, 6, colours)  # through the sharing context
        g2.sync()
        assert_hits_equal(frame(pkg, O, r1, u), hits_b, "tree B built on the sharing context")
        assert_hits_equal(frame(pkg, O, r2, u), hits_b, "tree B on the context that built it")
    finally:
        g2.close()
