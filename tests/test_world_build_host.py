"""Chunk trees and worlds built on the GPU, CPU side: the entry points are exported with signatures, the
numpy restatement (tests/world_build_ref.py) equals the host path (sequential put_in_voxel + generate_mip_tree) node for
node, and the integer mean the mip kernel takes equals the host's f32 formula for every sum and divisor."""
import ctypes as C

import numpy as np
import pytest

import build_ref as B
import world_build_ref as R
from conftest import GOLDEN
from pass_frame import write_blocks


def test_entry_points_are_exported_with_signatures(pkg):
    L = pkg._lib.lib()
    for name in ("svo_cpu_octree_build", "svo_world_build", "svo_world_build_timing"):
        assert name in pkg._lib.DEVICE_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(L.svo_cpu_octree_build.argtypes) == 6 and len(L.svo_world_build.argtypes) == 6
    assert C.sizeof(pkg._lib.ChunkBuildParams) == 24
    assert callable(pkg.CpuOctree.build) and callable(pkg.World.build_world) and callable(pkg.Gpu.world_build_timing)


def test_integer_mean_equals_the_f32_formula():
    """average_children (world.rs:311-328): (sum as f32 / count as f32) as u8, max 1 -- for every count 1..8 and every
    sum of that many channel values, 0..255 * count (so every sum 0..2040 is met)"""
    for d in range(1, 9):
        s = np.arange(0, 255 * d + 1, dtype=np.int64)
        f = (s.astype(np.float32) / np.float32(d)).astype(np.float32)
        host = np.maximum(np.clip(np.trunc(f), 0, 255).astype(np.int64), 1)
        assert np.array_equal(host, np.maximum(s // d, 1)), d


def random_set(rng, depth, n):
    side = 1 << depth
    coords = rng.integers(0, side, (n, 3))
    if n >= 8:
        coords[n // 2: n // 2 + n // 4] = coords[: n // 4]  # duplicate cells: the later one wins
    colours = rng.integers(0, 1 << 24, n)
    colours[::7] = 0  # colour 0: empty leaves on existing paths
    if depth >= 3:  # a subtree of colour-0 voxels only
        corner = np.array([[side - 1, side - 1, side - 1], [side - 2, side - 1, side - 1]])
        coords = np.concatenate([coords, corner])
        colours = np.concatenate([colours, [0, 0]])
    return coords, colours


def assert_same_tree(got, want, what):
    (gp, gr, gt), (wp, wr, wt) = got, want
    assert gp.size == wp.size, f"{what}: {gp.size} nodes, want {wp.size}"
    bad = np.flatnonzero((gp != wp) | (gr != wr).any(1))
    assert bad.size == 0, f"{what}: {bad.size} nodes differ, first {bad[:5]}"
    assert np.array_equal(gt, wt), f"{what}: top_mip {gt} want {wt}"


@pytest.mark.parametrize("depth", range(1, 9))
def test_reference_equals_host_path_on_random_sets(pkg, depth):
    rng = np.random.default_rng(100 + depth)
    for n in (1, 5, 60, 300):
        coords, colours = random_set(rng, depth, n)
        assert_same_tree(R.tree(coords, depth, colours), R.host_tree(pkg, coords, depth, colours), f"depth {depth}, n {n}")


@pytest.mark.parametrize("name", ("small", "monu9", "blocks"))
def test_reference_equals_host_path_on_fixtures(pkg, name):
    for label, size, xyzi, pal in B.fixture_models(GOLDEN, name):
        t = pkg.CpuOctree.from_voxels(size, xyzi, pal)
        top = t.generate_mip_tree()
        want = (*R.relayout(*t.raw()), np.array([top.r, top.g, top.b], dtype=np.uint8))
        coords, colours, depth = B.vox_voxels(size, xyzi, pal)
        assert_same_tree(R.tree(coords, depth, colours), want, label)


def test_world_reference_splits_into_chunk_trees(pkg):
    """every chunk of the restated world is the restated tree of its own voxels in local cells"""
    rng = np.random.default_rng(7)
    depth, wd = 6, 2
    coords, colours = random_set(rng, depth, 500)
    chunks = R.world(coords, depth, wd, colours)
    cd, s = depth - wd, 1 << wd
    keys, col, cells = R.leaves(coords, depth, colours)
    assert len(chunks) == len({tuple(c) for c in (cells >> cd).tolist()})
    for cid, (data, top) in chunks.items():
        i = cid - R.CHUNK_OFFSET // 2
        sel = ((cells >> cd) == [i // (s * s), i // s % s, i % s]).all(1)
        ptr, rgb, t = R.tree(cells[sel] & ((1 << cd) - 1), cd, col[sel])
        assert data == R.to_bin(ptr, rgb) and np.array_equal(top, t)
        assert pkg.CpuOctree.from_bin(data).bin() == data


@pytest.mark.gpu
def test_restated_mips_of_a_generated_chunk_equal_host_mips(pkg, gpu, tmp_path):
    """generate_world's device mips restated: a generated chunk's block leaves take their block's top_mip, then the
    integer means bottom-up -- equal to World.generate_mip_tree on the host"""
    blocks_dir = write_blocks(pkg, tmp_path / "blocks")
    w = pkg.World.new(str(tmp_path / "w"), blocks_dir)
    proc = pkg.Procedural(gpu)
    chunk = proc.generate_chunk((-1.0, -1.0, -1.0), 1, 5)
    ptrs, rgb = chunk.raw()
    rgb = rgb.astype(np.int64)
    block = ptrs > R.CHUNK_OFFSET
    for b in np.unique(ptrs[block]):
        top = w.chunk(int(b - R.CHUNK_OFFSET)).generate_mip_tree()
        rgb[ptrs == b] = [top.r, top.g, top.b]
    order = []  # interior nodes, breadth-first
    todo = [c for c in range(8) if ptrs[c] < R.CHUNK_OFFSET]
    while todo:
        order += todo
        todo = [int(ptrs[p]) + c for p in todo for c in range(8) if ptrs[int(ptrs[p]) + c] < R.CHUNK_OFFSET]
    for p in reversed(order):
        rgb[p] = R.mip(rgb[None, int(ptrs[p]) + np.arange(8)])[0]
    want_top = R.mip(rgb[None, 0:8])[0]
    w.insert(R.CHUNK_OFFSET // 2, chunk)
    top = w.generate_mip_tree(R.CHUNK_OFFSET // 2)
    got_ptrs, got_rgb = w.chunk(R.CHUNK_OFFSET // 2).raw()
    assert np.array_equal(got_rgb, rgb.astype(np.uint8))
    assert [top.r, top.g, top.b] == want_top.tolist()
