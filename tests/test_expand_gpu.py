"""World.expand on the GPU (svo_adaptive_expand, DeviceAdaptive.expand, Render.from_world) against the host
call it restates: words, positions, hole stack, length, count and chunk set, bit for bit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_hits_equal, set_uniforms_from_oracle
from pass_frame import assert_octrees_equal, monu9_world, write_blocks

pytestmark = pytest.mark.gpu

VOXEL_OFFSET = 1 << 27
SIZE = (96, 64)


def attach(pkg, world, octree, capacity):
    g = pkg.Gpu(0)
    g.set_option(pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, 1)
    render = pkg.Render.new(g, SIZE, octree, capacity=capacity)
    return g, render, pkg.adaptive.DeviceAdaptive(g, render, octree, world)


def check_expand(pkg, make_world, max_depth, cam=None, lod_c=0.0, max_words=None, capacity=200_000, calls=1, same_chunks=True,
                 min_sub=1):
    """Two identical worlds, one expanded on the host and one on the device, `calls` times each: everything equal."""
    wa, wb = make_world(), make_world()
    oa, ob = wa.root_octree(), wb.root_octree()
    g, render, dev = attach(pkg, wb, ob, capacity)
    counts = []
    for call in range(calls):
        host_cap = min(max_words, capacity) if max_words else capacity
        want = wa.expand(oa, max_depth, cam=cam, lod_c=lod_c, max_words=host_cap)
        got = dev.expand(max_depth, cam=cam, lod_c=lod_c, max_words=max_words)
        print(f"expand({max_depth}, {cam}, {lod_c}, max_words={max_words}) call {call}: host {want} subdivisions, {len(oa)} words; "
              f"device {got}, {dev.length}; chunks loaded {dev.last['chunks_loaded']}; timing {dev.expand_timing()}")
        assert got == want and dev.last["n_sub"] == want, f"call {call}: {got} subdivisions, the host made {want}"
        assert dev.length == len(oa) == dev.last["length"] and render.node_length >= dev.length
        assert np.array_equal(render.read_nodes(dev.length), oa.raw_data()), f"call {call}: device words differ"
        if same_chunks:
            assert wa.chunk_ids() == wb.chunk_ids(), f"call {call}: chunk sets differ"
        else:
            assert set(wa.chunk_ids()) <= set(wb.chunk_ids()), f"call {call}: the device lacks chunks the host loaded"
        counts.append(want)
    assert sum(counts) >= min_sub, counts
    assert len(ob) == 8  # the host octree is stale until download()
    dev.download()
    assert_octrees_equal(oa, ob, "after download")
    g.close()
    return counts, wa, oa


def test_monu9_no_camera(pkg, gpu):
    counts, _, oa = check_expand(pkg, lambda: monu9_world(pkg), 6)
    assert (counts[0], len(oa)) == (1831, 14656)


@pytest.mark.parametrize("max_depth,cam,lod_c", [(8, (0.3, 0.4, -1.6), 40.0), (7, (0.1, 0.2, -1.5), 12.0)])
def test_monu9_camera(pkg, gpu, max_depth, cam, lod_c):
    check_expand(pkg, lambda: monu9_world(pkg), max_depth, cam=cam, lod_c=lod_c, min_sub=50)


@pytest.mark.parametrize("max_words", [5000, 4001])
def test_cap_max_words(pkg, gpu, max_words):
    """5000 ends on a level boundary, 4001 cuts a level (monu9 has one chunk, so the chunk sets stay equal)."""
    counts, _, oa = check_expand(pkg, lambda: monu9_world(pkg), 6, max_words=max_words)
    assert len(oa) == max_words // 8 * 8 and counts[0] == (len(oa) - 8) // 8


@pytest.mark.parametrize("max_words", [None, 1 << 27])
def test_cap_is_the_capacity(pkg, gpu, max_words):
    """No max_words, or one above the capacity: the node buffer's capacity is where expansion stops, without an error."""
    counts, _, oa = check_expand(pkg, lambda: monu9_world(pkg), 6, max_words=max_words, capacity=4001)
    assert len(oa) == 4000 and counts[0] == 499


def test_streamed_world_loads_chunks(pkg, gpu, tmp_path):
    """A generated world opened with only 0.bin resident: the first expand loads chunks (the leaves that ask are skipped),
    the second refines into them; host and device load the same chunks and skip the same leaves."""
    blocks = str(tmp_path / "blocks")
    write_blocks(pkg, blocks)
    path = str(tmp_path / "world")
    pkg.World.generate_world(path, pkg.Procedural(gpu), world_depth=1, chunk_depth=5, blocks_dir=blocks)

    def make_world():
        world = pkg.World.load_world(path)
        assert world.chunk_ids() == [0]
        return world

    counts, wa, _ = check_expand(pkg, make_world, 7, calls=3, capacity=8_000_000)
    assert len(wa.chunk_ids()) > 1, "no chunk was loaded"
    # the root's leaves name the streamed chunks: the first call only loads them, the second refines into them
    assert counts[0] == 0 and counts[1] > 1000, counts


def test_streamed_world_with_camera_and_cap(pkg, gpu, tmp_path):
    """The same world under a camera rule with a cap that cuts a level: the tree still equals the host's; the device may
    have loaded chunks for leaves behind the cut."""
    blocks = str(tmp_path / "blocks")
    write_blocks(pkg, blocks)
    path = str(tmp_path / "world")
    pkg.World.generate_world(path, pkg.Procedural(gpu), world_depth=1, chunk_depth=5, blocks_dir=blocks)
    check_expand(pkg, lambda: pkg.World.load_world(path), 8, cam=(0.0, 0.25, -1.2), lod_c=64.0, max_words=3003, calls=2,
                 capacity=100_000, same_chunks=False)


def shell_world(pkg, depth=4):
    """tests/config_scenes.py config3 at a smaller shell depth: a spherical shell whose leaves instance blocks 1..8."""
    z = np.load(os.path.join(GOLDEN, "blocks_vox.npz"))
    world = pkg.World.new("")
    for i, name in enumerate(pkg.world.BLOCK_NAMES):
        world.insert(i + 1, pkg.CpuOctree.from_voxels(16, z[name + "_xyzi"], z[name + "_palette"]))
        world.generate_mip_tree(i + 1)
    tree = pkg.CpuOctree.new(0)
    n = 1 << depth
    ax = (np.arange(n) + 0.5) / n * 2 - 1
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    r = np.sqrt(X * X + Y * Y + Z * Z)
    for i, j, k in np.argwhere(np.abs(r - 0.75) < 1.0 / n):
        tree.put_in_voxel((float(ax[i]), float(ax[j]), float(ax[k])), pkg.Voxel(1, 1, 1), depth)
    world.insert(0, pkg.CpuOctree.load_octree(tree.to_rsvo(), depth))
    world.generate_mip_tree(0)
    return world


def test_block_instanced_shell(pkg, gpu):
    counts, wa, oa = check_expand(pkg, lambda: shell_world(pkg), 8, capacity=8_000_000)
    assert wa.chunk_ids() == list(range(9))
    assert counts[0] > 10_000, counts  # far more groups than the shell has cells: the blocks are instanced
    check_expand(pkg, lambda: shell_world(pkg), 8, cam=(0.3, 0.4, -1.6), lod_c=100.0, capacity=8_000_000, min_sub=1000)


def test_tree_with_a_hole_is_refused(pkg, gpu):
    world = monu9_world(pkg)
    octree = world.root_octree()
    world.expand(octree, 3)
    interior = np.nonzero((octree.raw_data() >> 4) < VOXEL_OFFSET)[0]
    # collapse a node whose children are all leaves: its group goes to the hole stack
    words = octree.raw_data()
    node = next(int(i) for i in interior[::-1] if np.all((words[(words[i] >> 4):(words[i] >> 4) + 8] >> 4) >= VOXEL_OFFSET))
    assert pkg.adaptive.process_unsubdivision(np.array([node], dtype=np.uint32), octree, world) == 1
    assert octree.hole_stack().size == 1
    n = len(octree)
    g, render, dev = attach(pkg, world, octree, 100_000)
    before = render.read_nodes(n)
    with pytest.raises(pkg.SvoError, match="svo_world_expand"):
        dev.expand(6)
    assert dev.length == n and np.array_equal(render.read_nodes(n), before)
    dev.download()
    assert len(octree) == n and octree.hole_stack().size == 1
    with pytest.raises(pkg.SvoError, match="status -1"):
        dev.expand(32)
    g.close()


def test_two_device_runs_are_identical(pkg, gpu):
    runs = []
    for _ in range(2):
        g = pkg.Gpu(0)
        render, dev = pkg.Render.from_world(g, SIZE, monu9_world(pkg), 8, cam=(0.3, 0.4, -1.6), lod_c=40.0, capacity=100_000)
        runs.append((render.read_nodes(dev.length), dev.download().positions().view(np.uint32).copy()))
        g.close()
    assert runs[0][0].size > 3000
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_from_world_then_streaming_frames(pkg, gpu):
    """Render.from_world + AdaptiveLoop(device=...) equals host expand + Render.new + AdaptiveLoop(on_device=True), frame by
    frame: records, counts and device arrays."""
    view = dict(cam=(0.1, 0.2, -1.5), lod_c=12.0)
    wa = monu9_world(pkg)
    oa = wa.root_octree()
    wa.expand(oa, 7, **view)
    ga = pkg.Gpu(0)
    ra = pkg.Render.new(ga, (160, 96), oa, capacity=200_000)
    la = pkg.adaptive.AdaptiveLoop(ga, ra, pkg.Compute.new(ga, ra), oa, wa, on_device=True)
    wb = monu9_world(pkg)
    gb = pkg.Gpu(0)
    rb, dev = pkg.Render.from_world(gb, (160, 96), wb, 7, capacity=200_000, **view)
    assert len(dev.octree) == 8 and dev.length == len(oa)
    lb = pkg.adaptive.AdaptiveLoop(gb, rb, pkg.Compute.new(gb, rb), dev.octree, wb, device=dev)
    assert lb.device is dev
    settings = pkg.Settings()
    moved = 0
    for frame in range(6):
        character = pkg.Character((0.1 + 0.03 * frame, 0.2, -1.5), (0.0, 0.0, 1.5))
        out = []
        for g, r, loop in ((ga, ra, la), (gb, rb, lb)):
            r.set_flags(pause_adaptive=False, shadows=True)
            hits, n_sub, n_unsub = loop.frame(settings, character, deterministic=True)
            g.sync()
            out.append((pkg.render.hits_to_numpy(hits).view(np.uint32).copy(), (n_sub, n_unsub), r.read_nodes(loop.device.length)))
        assert np.array_equal(out[0][0], out[1][0]), f"frame {frame}: records differ"
        assert out[0][1] == out[1][1], f"frame {frame}: counts {out[0][1]} != {out[1][1]}"
        assert np.array_equal(out[0][2], out[1][2]), f"frame {frame}: device arrays differ"
        moved += sum(out[0][1])
    assert moved > 0, "the frames exercised neither list"
    la.download()
    lb.download()
    assert_octrees_equal(la.octree, lb.octree, "after the frames")
    assert wa.chunk_ids() == wb.chunk_ids()
    ga.close()
    gb.close()


def test_trace_of_device_expanded_tree_equals_oracle(pkg, gpu, O):
    world = monu9_world(pkg)
    octree = world.root_octree()
    world.expand(octree, 7, cam=(0.1, 0.2, -1.5), lod_c=12.0)
    W, H = 128, 96
    u = O.make_uniforms(width=W, height=H, flags=O.F_PAUSE_ADAPTIVE)
    want = O.trace_frame(octree.raw_data(), u, threads=4).reshape(-1)
    g = pkg.Gpu(0)
    render, dev = pkg.Render.from_world(g, (W, H), monu9_world(pkg), 7, cam=(0.1, 0.2, -1.5), lod_c=12.0, capacity=100_000)
    set_uniforms_from_oracle(render, u)
    got = pkg.render.hits_to_numpy(render.render())
    g.sync()
    assert int((want["info"] >> 16 & 1).sum()) > 100
    assert_hits_equal(got, want, "device-expanded monu9")
    g.close()
