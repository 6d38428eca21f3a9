"""The adaptive step on the GPU (svo_adaptive_step) against the host path it replaces:
svo_adaptive_subdivide(sorted(sub)) then svo_adaptive_unsubdivide(sorted(unsub)), bit for bit."""

import numpy as np
import pytest

from pass_frame import assert_octrees_equal, monu9_world, write_blocks

pytestmark = pytest.mark.gpu

VOXEL_OFFSET = 1 << 27  # octree.rs:5: words at or above VOXEL_OFFSET << 4 are leaves


def make_loop(pkg, world, octree, on_device, capacity=200_000, size=(160, 96)):
    g = pkg.Gpu(0)
    render = pkg.Render.new(g, size, octree, capacity=capacity)
    render.set_flags(pause_adaptive=False, shadows=True)
    compute = pkg.Compute.new(g, render)
    loop = pkg.adaptive.AdaptiveLoop(g, render, compute, octree, world, incremental=True, on_device=on_device)
    return g, render, loop


def device_nodes(render, loop):
    n = loop.device.length if loop.device is not None else len(loop.octree)
    return render.read_nodes(n)


def run_frames(pkg, loops, cameras, check):
    settings = pkg.Settings()
    totals = np.zeros(2, dtype=np.int64)
    for frame, (pos, look) in enumerate(cameras):
        character = pkg.Character(pos, look)
        results = []
        for g, render, loop in loops:
            hits, n_sub, n_unsub = loop.frame(settings, character, deterministic=True)
            g.sync()
            results.append((pkg.render.hits_to_numpy(hits).view(np.uint32).copy(), n_sub, n_unsub, device_nodes(render, loop)))
        a = results[0]
        for b in results[1:]:
            assert np.array_equal(a[0], b[0]), f"frame {frame}: records differ"
            assert a[1:3] == b[1:3], f"frame {frame}: counts {a[1:3]} != {b[1:3]}"
            assert np.array_equal(a[3], b[3]), f"frame {frame}: device arrays differ"
        totals += (a[1], a[2])
        check(frame, results)
    return totals


MOVING = [((0.1 + 0.02 * f, 0.2, -1.5), (0.0, 0.0, 1.5)) for f in range(12)]


def test_device_step_equals_host_loop_frame_by_frame(pkg, gpu):
    """monu9, a moving camera: the device loop and the host loop (incremental, sorted lists) agree after every frame."""
    loops = []
    for on_device in (False, True):
        world = monu9_world(pkg)
        loops.append(make_loop(pkg, world, world.root_octree(), on_device))
    totals = run_frames(pkg, loops, MOVING, lambda f, r: None)
    assert totals[0] > 0 and totals[1] > 0, f"both lists must be exercised: {totals}"
    host, dev = loops[0][2], loops[1][2]
    dev.download()
    assert_octrees_equal(host.octree, dev.octree, "after download")
    assert len(dev.octree) > 1000
    for g, *_ in loops:
        g.close()


def test_device_step_deterministic(pkg, gpu):
    loops = []
    for _ in range(2):
        world = monu9_world(pkg)
        loops.append(make_loop(pkg, world, world.root_octree(), True))
    run_frames(pkg, loops, MOVING[:8], lambda f, r: None)
    for _, _, loop in loops:
        loop.download()
    assert_octrees_equal(loops[0][2].octree, loops[1][2].octree, "two device runs")
    for g, *_ in loops:
        g.close()


def _parents(words):
    parent = np.full(words.size, -1, dtype=np.int64)
    ptr = words >> 4
    interior = np.nonzero(ptr < VOXEL_OFFSET)[0]
    for i in interior:
        p = int(ptr[i])
        if p + 8 <= words.size:
            parent[p:p + 8] = i
    return parent


def test_nested_unsubdivision_one_pass(pkg, gpu):
    """An expanded tree seen from one side: cold subtrees list parents and children alike; one pass collapses them."""
    cam = (0.0, 0.0, -3.0)
    trees = []
    for _ in range(2):
        world = monu9_world(pkg)
        octree = world.root_octree()
        world.expand(octree, 6)
        trees.append((world, octree))
    (wa, oa), (wb, ob) = trees
    assert_octrees_equal(oa, ob, "expanded trees")
    # one traced frame from the front gives the lists
    g, render, loop = make_loop(pkg, wa, oa, False, capacity=3 * len(oa), size=(96, 64))
    render.update(pkg.Settings(), pkg.Character(cam, (0.0, 0.0, 1.0)))
    render.render()
    loop.compute.update(len(oa))
    sub, unsub = loop.compute.read_lists()
    sub.sort()
    unsub.sort()
    assert unsub.size > 100
    words = oa.raw_data()
    parent = _parents(words)
    listed = np.zeros(words.size, dtype=bool)
    listed[unsub] = True
    nested = 0
    for e in unsub:  # a listed ancestor has a lower index, so a lower rank in the sorted list
        p = parent[e]
        while p >= 0:
            if listed[p]:
                nested += 1
                break
            p = parent[p]
    assert nested > 0, "no unsubdivide entry has a listed ancestor"
    gb = pkg.Gpu(0)
    gb.set_option(pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, 1)
    rb = pkg.Render.new(gb, (96, 64), ob, capacity=3 * len(ob))
    dev = pkg.adaptive.DeviceAdaptive(gb, rb, ob, wb)
    n_sub = pkg.adaptive.process_subdivision(sub, oa, wa)
    n_unsub = pkg.adaptive.process_unsubdivision(unsub, oa, wa)
    # the device gets the lists unsorted
    rng = np.random.default_rng(5)
    got = dev.step(rng.permutation(sub), rng.permutation(unsub))
    assert got == (n_sub, n_unsub)
    assert np.array_equal(rb.read_nodes(dev.length), oa.raw_data())
    dev.download()
    assert_octrees_equal(oa, ob, "after one nested pass")
    assert wa.chunk_ids() == wb.chunk_ids()
    g.close()
    gb.close()


def test_streamed_world_loads_and_removes(pkg, gpu, tmp_path):
    """A generated world opened with only 0.bin resident: chunk loads (and failed block loads), then removals."""
    blocks = str(tmp_path / "blocks")
    write_blocks(pkg, blocks)
    path = str(tmp_path / "world")
    pkg.World.generate_world(path, pkg.Procedural(gpu), world_depth=1, chunk_depth=5, blocks_dir=blocks)
    loops, worlds = [], []
    for on_device in (False, True):
        world = pkg.World.load_world(path)
        assert world.chunk_ids() == [0]
        worlds.append(world)
        loops.append(make_loop(pkg, world, world.root_octree(), on_device))
    # approach the island, then look away: the cold tree collapses and the streamed chunks go
    cams = [((0.0, 0.9 - 0.05 * f, -1.6 + 0.1 * f), (0.0, -0.4, 1.0)) for f in range(14)]
    cams += [((0.0, 0.0, -3.0), (0.0, 0.0, -1.0))] * 4
    events = {"loaded": 0, "removed": 0}

    def check(frame, results):
        last = loops[1][2].device.last
        events["loaded"] += last["chunks_loaded"] > 0
        events["removed"] += len(last["removed"]) > 0
        assert worlds[0].chunk_ids() == worlds[1].chunk_ids(), f"frame {frame}: chunk sets differ"

    run_frames(pkg, loops, cams, check)
    assert events["loaded"] > 0 and events["removed"] > 0, events
    loops[1][2].download()
    assert_octrees_equal(loops[0][2].octree, loops[1][2].octree, "streamed world")
    for g, *_ in loops:
        g.close()


def test_refusals_leave_node_buffer_untouched(pkg, gpu):
    world = monu9_world(pkg)
    octree = world.root_octree()
    world.expand(octree, 3)
    n = len(octree)
    g = pkg.Gpu(0)
    g.set_option(pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, 1)
    render = pkg.Render.new(g, (64, 64), octree, capacity=n)  # no room for one more group
    dev = pkg.adaptive.DeviceAdaptive(g, render, octree, world)
    before = render.read_nodes(n)
    leaves = np.nonzero((octree.raw_data() >> 4) >= VOXEL_OFFSET)[0].astype(np.uint32)
    cases = [(np.array([leaves[0], leaves[0]], dtype=np.uint32), "status -3"),
             (np.array([n + 3], dtype=np.uint32), "status -3"),
             (leaves, "status -6")]
    for sub, status in cases:
        with pytest.raises(pkg.SvoError, match=status):
            dev.step(sub, np.zeros(0, dtype=np.uint32))
        assert np.array_equal(render.read_nodes(n), before)
    # the host path does subdivide one of the leaves, so the last refusal is a real capacity limit
    assert pkg.adaptive.process_subdivision(leaves, octree, world) > 0
    g.close()
