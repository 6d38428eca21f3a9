"""Chunk trees and streamable worlds built on the GPU (svo_cpu_octree_build / svo_world_build) against the
numpy restatement (tests/world_build_ref.py) node for node and byte for byte; the same bytes for any order of distinct
voxels and on every run; the round trip into the renderer and the streaming loop; errors that create nothing; and
generate_world's device mips against the host-mipped chunks."""
import os

import numpy as np
import pytest

import world_build_ref as R
from pass_frame import assert_octrees_equal, write_blocks
from test_adaptive_device_gpu import make_loop, run_frames

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAP = -1, -6


def top_mip(pkg, tree):
    """a tree's top_mip, as a root mipped over a block leaf that references it sees it (the world takes the tree over, so
    the tree keeps the world alive)"""
    w = pkg.World()
    w.insert(1, tree)
    tree._world = w
    root = pkg.CpuOctree()
    root.put_in_block((-1.0, -1.0, -1.0), 1, 1)
    w.insert(0, root)
    w.generate_mip_tree(0)
    return w.chunk(0).raw()[1][0]


def assert_tree(pkg, t, want, what):
    ptrs, rgb = t.raw()
    wp, wr, wt = want
    assert ptrs.size == wp.size, f"{what}: {ptrs.size} nodes, want {wp.size}"
    bad = np.flatnonzero((ptrs != wp) | (rgb != wr).any(1))
    assert bad.size == 0, f"{what}: {bad.size} nodes differ, first {bad[:5]}"
    assert np.array_equal(top_mip(pkg, t), wt), f"{what}: top_mip"


def random_set(rng, depth, n):
    side = 1 << depth
    coords = rng.integers(0, side, (n, 3))
    coords[0], coords[-1] = 0, side - 1
    if n >= 8:
        coords[n // 2: n // 2 + n // 4] = coords[: n // 4]  # duplicate cells: the later one wins
    colours = rng.integers(0, 1 << 32, n)
    colours[::7] = 0  # colour 0: empty leaves on existing paths
    colours[1::11] = 0xFF000000  # only high bits: colour 0 too
    return coords, colours


def height_field(depth, side):
    x, z = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    h = (np.sin(x * 2.3 / side * 6) + np.cos(z * 1.7 / side * 6)) * side / 16
    y = ((1 << depth) // 2 + h).astype(np.int64)
    coords = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    return coords, (coords[:, 1] * 2654435761 + coords[:, 0]) & 0xFFFFFF


@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8, 12, 21])
def test_cpu_octree_build_equals_reference(pkg, gpu, depth):
    rng = np.random.default_rng(depth)
    for n in (1, 7, 500, 20_000):
        coords, colours = random_set(rng, depth, n)
        t = pkg.CpuOctree.build(gpu, coords, depth, colours)
        assert_tree(pkg, t, R.tree(coords, depth, colours), f"depth {depth}, n {n}")


def test_cpu_octree_build_cube_heightfield_order_and_runs(pkg, gpu):
    import torch
    side = 24  # a dense-ish cube at depth 5
    cube = np.argwhere(np.ones((side,) * 3, dtype=bool)) + 4
    t = pkg.CpuOctree.build(gpu, cube, 5, colour=0x336699)
    assert_tree(pkg, t, R.tree(cube, 5, colour=0x336699), "cube")
    coords, colours = height_field(12, 1500)  # 2.25 M voxels
    want = R.tree(coords, 12, colours)
    t = pkg.CpuOctree.build(gpu, coords, 12, colours)
    assert_tree(pkg, t, want, "height field")
    ms = gpu.world_build_timing()
    assert len(ms) == 9 and min(ms) >= 0 and ms[8] > 0
    data = t.bin()
    perm = np.random.default_rng(1).permutation(coords.shape[0])  # distinct cells: any order
    assert pkg.CpuOctree.build(gpu, coords[perm], 12, colours[perm]).bin() == data
    assert pkg.CpuOctree.build(gpu, coords, 12, colours).bin() == data  # a second run
    dev = torch.device("cuda", gpu.device)
    tt = pkg.CpuOctree.build(gpu, torch.as_tensor(coords, device=dev), 12, torch.as_tensor(colours, device=dev))
    assert tt.bin() == data
    assert pkg.CpuOctree.build(gpu, np.zeros((0, 3), dtype=np.int64), 5) is None


def host_root(pkg, chunks, world_depth):
    """0.bin as generate_world builds it: put_in_block per chunk in id order, mips over the chunks' top_mips"""
    w, root = pkg.World(), pkg.CpuOctree()
    s = 1 << world_depth
    for cid in sorted(chunks):
        i = cid - R.CHUNK_OFFSET // 2
        w.insert(cid, pkg.CpuOctree.from_bin(chunks[cid][0]))
        w.generate_mip_tree(cid)
        root.put_in_block([float(v) * (2.0 / s) - 1.0 for v in (i // (s * s), i // s % s, i % s)], cid, world_depth)
    w.insert(0, root)
    w.generate_mip_tree(0)
    return w.chunk(0).bin()


@pytest.mark.parametrize("world_depth", [1, 2, 3])
def test_build_world_files_equal_reference(pkg, gpu, tmp_path, world_depth):
    depth = 7
    coords, colours = random_set(np.random.default_rng(10 + world_depth), depth, 3000)
    path = str(tmp_path / "world")
    world = pkg.World.build_world(path, gpu, coords, depth, colours, world_depth=world_depth)
    want = R.world(coords, depth, world_depth, colours)
    assert sorted(os.listdir(path)) == sorted(f"{i}.bin" for i in [0, *want])
    for cid, (data, _) in want.items():
        assert open(os.path.join(path, f"{cid}.bin"), "rb").read() == data, cid
    assert open(os.path.join(path, "0.bin"), "rb").read() == host_root(pkg, want, world_depth)
    assert world.chunk_ids() == [0]


def test_build_world_round_trip_into_the_renderer(pkg, gpu, tmp_path):
    depth, wd = 9, 2
    coords, colours = height_field(depth, 300)
    colours[::5] = 0x010203
    path = str(tmp_path / "world")
    world = pkg.World.build_world(path, gpu, coords, depth, colours, world_depth=wd)
    for cid in R.world(coords, depth, wd, colours):
        world.load_chunk(cid)
    octree = world.root_octree()
    world.expand(octree, depth)
    render = pkg.Render(gpu, (64, 64), np.full(8, 1 << 31, dtype=np.uint32), capacity=4_000_000)
    n = render.build_nodes(coords, depth, colours)
    assert np.array_equal(octree.raw_data(), render.read_nodes(n))
    # expanded to depth 4 the leaves carry the restated mips of the level-4 nodes
    shallow = world.root_octree()
    world.expand(shallow, 4)
    words = shallow.raw_data()
    got = np.sort(words[words > (1 << 27) << 4] >> 4) - (1 << 27)
    ptrs, rgb, _ = R.tree(coords, depth, colours)
    level = [c for c in range(8)]
    for _ in range(3):
        level = [int(ptrs[p]) + c for p in level if ptrs[p] < R.CHUNK_OFFSET for c in range(8)]
    inner = [p for p in level if ptrs[p] < R.CHUNK_OFFSET]
    want = np.sort(rgb[inner].astype(np.int64) @ np.array([1 << 16, 1 << 8, 1]))
    assert got.size > 0 and np.array_equal(got, want)


def test_build_world_streams_like_the_host_loop(pkg, gpu, tmp_path):
    depth, wd = 8, 2
    coords, colours = height_field(depth, 256)
    path = str(tmp_path / "world")
    pkg.World.build_world(path, gpu, coords, depth, colours, world_depth=wd)
    loops, worlds = [], []
    for on_device in (False, True):
        world = pkg.World.load_world(path)
        worlds.append(world)
        loops.append(make_loop(pkg, world, world.root_octree(), on_device, capacity=4_000_000))
    cams = [((0.0, 0.6 - 0.05 * f, -1.6 + 0.1 * f), (0.0, -0.3, 1.0)) for f in range(8)]

    def check(frame, results):
        assert worlds[0].chunk_ids() == worlds[1].chunk_ids(), f"frame {frame}: chunk sets differ"

    totals = run_frames(pkg, loops, cams, check)
    assert totals[0] > 0
    assert len(worlds[0].chunk_ids()) > 1  # chunks were streamed in
    loops[1][2].download()
    assert_octrees_equal(loops[0][2].octree, loops[1][2].octree, "built world")
    for g, *_ in loops:
        g.close()


def test_build_world_errors_create_nothing(pkg, gpu, tmp_path):
    coords, colours = random_set(np.random.default_rng(3), 6, 400)
    path = str(tmp_path / "world")
    os.makedirs(path)
    with pytest.raises(pkg.SvoError, match="already exists"):
        pkg.World.build_world(path, gpu, coords, 6, colours)
    os.rmdir(path)
    bad = [dict(depth=0), dict(depth=22), dict(world_depth=0), dict(world_depth=5), dict(world_depth=6)]
    for kw in bad:
        args = {"depth": 6, "world_depth": 1, **kw}
        with pytest.raises(pkg.SvoError, match=f"status {ERR_ARG}"):
            pkg.World.build_world(path, gpu, coords, args["depth"], colours, world_depth=args["world_depth"])
        assert not os.path.exists(path), kw
    far = coords.copy()
    far[17] = [0, 64, 0]
    with pytest.raises(pkg.SvoError, match=f"status {ERR_ARG}.*outside"):
        pkg.World.build_world(path, gpu, far, 6, colours)
    assert not os.path.exists(path)
    with pytest.raises(pkg.SvoError, match=f"status {ERR_CAP}"):
        pkg.World.build_world(path, gpu, coords, 6, colours, max_nodes=64)
    assert not os.path.exists(path)
    with pytest.raises(pkg.SvoError, match=f"status {ERR_CAP}"):
        pkg.CpuOctree.build(gpu, coords, 6, colours, max_nodes=64)
    pkg.World.build_world(path, gpu, coords, 6, colours)  # the context is still usable
    want = R.world(coords, 6, 1, colours)
    assert sorted(os.listdir(path)) == sorted(f"{i}.bin" for i in [0, *want])


def test_generate_world_equals_host_mipped_chunks(pkg, gpu, tmp_path):
    blocks = str(tmp_path / "blocks")
    write_blocks(pkg, blocks)
    path = str(tmp_path / "world")
    proc = pkg.Procedural(gpu)
    pkg.World.generate_world(path, proc, world_depth=1, chunk_depth=6, blocks_dir=blocks)
    t = proc.timing()
    assert t["world_copy_and_build"] > 0 and t["world_mips"] > 0 and t["world_writes"] > 0
    host = pkg.World.new("", blocks)
    root = pkg.CpuOctree()
    files = {"0.bin"}
    for (x, y, z), cid, pos in [((x, y, z), R.CHUNK_OFFSET // 2 + (x * 2 + y) * 2 + z, [v - 1.0 for v in (x, y, z)])
                                for x in range(2) for y in range(2) for z in range(2)]:
        chunk = proc.generate_chunk(pos, 1, 6)
        if chunk is None:
            continue
        host.insert(cid, chunk)
        host.generate_mip_tree(cid)
        data = host.chunk(cid).bin()
        assert open(os.path.join(path, f"{cid}.bin"), "rb").read() == data, cid
        files.add(f"{cid}.bin")
        root.put_in_block(pos, cid, 1)
    host.insert(0, root)
    host.generate_mip_tree(0)
    assert open(os.path.join(path, "0.bin"), "rb").read() == host.chunk(0).bin()
    assert set(os.listdir(path)) == files
