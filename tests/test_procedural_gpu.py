"""Procedural world generator on the GPU (csrc/svo_proc.hip) against the numpy float32 restatement in
tests/proc_ref.py: the signed distance bit for bit, the classification cell for cell, the breadth-first chunk tree
word for word, the node cap, and a generated world streamed and traced end to end."""
import os

import numpy as np
import pytest

import proc_ref as R
from conftest import assert_hits_equal, set_uniforms_from_oracle
from pass_frame import write_blocks

pytestmark = pytest.mark.gpu

F = np.float32
CO = R.CHUNK_OFFSET
CHUNKS_1 = [pos for _, _, pos in R.chunk_layout(1)]  # the 8 chunks of a world_depth 1 world


@pytest.fixture(scope="module")
def proc(pkg, gpu):
    return pkg.Procedural(gpu)


@pytest.fixture(scope="module")
def ref_cls6():
    """numpy class bytes (id order) of the 8 chunks at base_depth 1, chunk_depth 6"""
    return [R.classify(pos, 1, 6) for pos in CHUNKS_1]


def test_sdf_is_bit_identical_to_numpy(proc):
    rng = np.random.default_rng(7)
    parts = [rng.uniform(-1.2, 1.2, (600000, 3)).astype(np.float32)]
    # cell corners (and the points one voxel above them) of all 8 chunks of depth 10 (base 1 + chunk 9)
    for pos in CHUNKS_1:
        cells = rng.integers(0, 512, (30000, 3))
        wx, wy, wz = R.world_of_cells(pos, 1, 9, cells[:, 0], cells[:, 1], cells[:, 2])
        parts.append(np.stack([wx, wy, wz], 1))
        parts.append(np.stack([wx + F(0), wy + F(2.0 / 1024), wz + F(0)], 1))
    # negative and integer coordinates, far outside the island too
    g = np.arange(-6, 6.5, 0.5, dtype=np.float32)
    parts.append(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    # points whose noise lattice coordinate v + dot(v, 1/3) lands on an integer (floor ties), and their neighbours
    n = np.arange(-4, 5, dtype=np.float32)
    lattice = np.stack(np.meshgrid(n, n, n, indexing="ij"), -1).reshape(-1, 3)
    for scale in ((1.6, 1.6, 1.6), (3.2, 3.2, 3.2), (2.3, 0.4, 2.3), (4.6, 0.8, 4.6)):
        p = (lattice / np.array(scale, dtype=np.float32)).astype(np.float32)
        diag = (np.repeat(n, 3).reshape(-1, 3) / np.array(scale, dtype=np.float32)).astype(np.float32)
        for q in (p, diag):
            parts += [q, np.nextafter(q, F(np.inf)), np.nextafter(q, F(-np.inf))]
    pts = np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)
    assert pts.shape[0] > 1000000
    got = proc.sdf(pts)
    want = R.sdf(pts[:, 0], pts[:, 1], pts[:, 2])
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{bad.size} of {pts.shape[0]} differ; first at {pts[bad[:3]]}: got {got[bad[:3]]} want {want[bad[:3]]}"
    assert (got < 0).any() and (got > 0).any()


def test_classify_matches_numpy_cell_for_cell(proc, ref_cls6):
    solid_chunks = 0
    for pos, want in zip(CHUNKS_1, ref_cls6):
        got = proc.classify(pos, 1, 6)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"chunk {pos}: {bad.size} cells differ, first ids {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"
        solid_chunks += bool(want.any())
        assert set(np.unique(got).tolist()) <= {0, 1, 3}
    assert solid_chunks >= 2
    assert sum(int((c == 3).sum()) for c in ref_cls6) > 0  # grass on top


def test_generate_chunk_matches_numpy_word_for_word(proc, ref_cls6):
    # every chunk of the world_depth 1 world touches the island; one in the sky of a world_depth 2 world does not
    sky = (0.5, 0.5, 0.5)
    cases = [(pos, 1, cls) for pos, cls in zip(CHUNKS_1, ref_cls6)] + [(sky, 2, R.classify(sky, 2, 6))]
    empty = 0
    for pos, base, cls in cases:
        want = R.build_tree(R.to_morton(cls, 6), 6)
        chunk = proc.generate_chunk(pos, base, 6)
        if want is None:
            assert chunk is None, f"chunk {pos}: numpy finds it empty"
            empty += 1
            continue
        ptr, rgb = chunk.raw()
        assert ptr.size == want.size, f"chunk {pos}: {ptr.size} nodes, numpy {want.size}"
        bad = np.flatnonzero(ptr != want)
        assert bad.size == 0, f"chunk {pos}: {bad.size} words differ, first {bad[:5]}: got {ptr[bad[:5]]} want {want[bad[:5]]}"
        assert not rgb.any()
        again = proc.generate_chunk(pos, base, 6)
        assert again.bin() == chunk.bin()  # same bytes every run (the reference's insertion order is racy)
    assert empty == 1


def _bfs_levels(words, depth):
    """Walk the tree level by level; assert its breadth-first layout on the way and return the leaves per level."""
    level, nxt = np.arange(8), 8
    leaves = []
    for lvl in range(1, depth + 1):
        w = words[level].astype(np.int64)
        inner = w[w < CO]
        if lvl == depth:
            assert inner.size == 0, "interior node at the chunk's last level"
        else:
            assert np.array_equal(inner, nxt + 8 * np.arange(inner.size)), f"level {lvl}: groups not breadth-first"
            assert not (w > CO).any(), f"block leaf above the last level (level {lvl})"
        leaves.append(w[w >= CO])
        level = (inner[:, None] + np.arange(8)).reshape(-1)
        nxt += 8 * inner.size
    assert level.size == 0 and nxt == words.size
    return leaves


def test_reference_size_chunk_is_well_formed_and_classified(proc):
    pos, depth = (-1.0, -1.0, -1.0), 9  # the lower-left-back chunk of the reference's world: the island's underside
    chunk = proc.generate_chunk(pos, 1, depth)
    assert chunk is not None
    words, _ = chunk.raw()
    n_interior = int((words < CO).sum())
    assert words.size == 8 + 8 * n_interior and n_interior > 1000
    last = _bfs_levels(words, depth)[-1]
    assert set(np.unique(last).tolist()) <= {CO, CO + 1, CO + 3} and (last > CO).any()
    rng = np.random.default_rng(9)
    cells = rng.integers(0, 512, (200000, 3))
    want = R.classify_cells(pos, 1, depth, cells[:, 0], cells[:, 1], cells[:, 2])
    got = R.descend(words, depth, cells[:, 0], cells[:, 1], cells[:, 2])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} sampled cells differ, first {cells[bad[:3]]}: tree {got[bad[:3]]} numpy {want[bad[:3]]}"
    assert (want != 0).sum() > 1000
    t = proc.timing()
    assert t["classify"] > 0 and t["emit"] > 0


def test_node_cap_is_an_error_and_the_context_stays_usable(pkg, O, gpu, proc):
    pos = CHUNKS_1[0]
    full = proc.generate_chunk(pos, 1, 6)
    with pytest.raises(pkg.SvoError, match="max_nodes") as e:
        proc.generate_chunk(pos, 1, 6, max_nodes=len(full) - 8)
    assert "status -6" in str(e.value)
    assert len(proc.generate_chunk(pos, 1, 6, max_nodes=len(full))) == len(full)
    with pytest.raises(pkg.SvoError, match="chunk_depth"):
        proc.generate_chunk(pos, 1, 1)
    with pytest.raises(pkg.SvoError, match="chunk_depth"):
        proc.generate_chunk(pos, 1, 10)
    # the context still renders a small frame bit-exactly
    words = pkg.scenes.random_tree(seed=3, max_depth=7, p_split=0.55, p_solid=0.35, max_words=1 << 18)
    u = O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    render = pkg.Render(gpu, (64, 64), words, capacity=max(words.size, 1024))
    set_uniforms_from_oracle(render, u)
    got = pkg.render.hits_to_numpy(render.render())
    gpu.sync()
    assert_hits_equal(got, O.trace_frame(words, u, threads=4), "frame after a refused chunk")


def test_generate_world_end_to_end(pkg, O, gpu, proc, ref_cls6, tmp_path):
    blocks = str(tmp_path / "blocks")
    write_blocks(pkg, blocks)
    path = str(tmp_path / "world")
    pkg.World.generate_world(path, proc, world_depth=1, chunk_depth=6, blocks_dir=blocks)
    with pytest.raises(ValueError, match="already exists"):
        pkg.World.generate_world(path, proc, world_depth=1, chunk_depth=6, blocks_dir=blocks)
    layout = pkg.procedural.chunk_layout(1)
    present = [cid for (_, cid, _), cls in zip(layout, ref_cls6) if cls.any()]
    assert sorted(os.listdir(path)) == sorted(f"{i}.bin" for i in [0] + present)
    for (_, cid, pos), cls in zip(layout, ref_cls6):
        if cls.any():
            want = R.build_tree(R.to_morton(cls, 6), 6)
            blob = np.fromfile(os.path.join(path, f"{cid}.bin"), dtype=np.uint32).reshape(-1, 2)
            assert np.array_equal(blob[:, 0], want)  # the pointers as generated; the colours are mips now
    t = proc.timing()
    assert t["world_gpu"] > 0 and t["world_writes"] > 0

    world = pkg.World.load_world(path)
    assert world.chunk_ids() == [0]
    for cid in present:
        world.load_chunk(cid)
    rng = np.random.default_rng(4)
    for (_, cid, pos), cls in zip(layout, ref_cls6):
        side = 64
        ids = rng.integers(0, side ** 3, 300)
        ids[:150] = rng.choice(np.flatnonzero(cls), 150) if cls.any() else ids[:150]
        for i in ids.tolist():
            x, y, z = i % side, i // side % side, i // side // side
            centre = [p + (c + 0.5) * 2.0 / 128 for p, c in zip(pos, (x, y, z))]
            ch, idx, d, _ = world.find_voxel(centre, 7)
            ptr = int(world.chunk(ch).raw()[0][idx])
            if cls[i]:
                assert (ch, d, ptr) == (cid, 7, CO + int(cls[i])), (pos, (x, y, z))
            else:
                assert ptr == CO, (pos, (x, y, z))

    # the streaming loop down to the generated cells, then one frame on the GPU against the oracle
    octree = world.root_octree()
    world.expand(octree, max_depth=7)
    words = octree.raw_data()
    assert pkg._lib.lib().svo_nodes_max_depth(words.ctypes.data, words.size) == 7
    u = O.make_uniforms(width=128, height=128, flags=O.F_PAUSE_ADAPTIVE)
    render = pkg.Render(gpu, (128, 128), words, capacity=max(words.size, 1024))
    set_uniforms_from_oracle(render, u)
    got = pkg.render.hits_to_numpy(render.render())
    gpu.sync()
    want = O.trace_frame(words, u, threads=4)
    assert_hits_equal(got, want, "generated world")
    assert (want["info"] >> 16 & 1).sum() > 100  # the island is in view
