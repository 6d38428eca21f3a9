"""CPU-side checks of the device adaptive step's boundary: the entry points exist, the loop keeps its
default, and the host accessors the GPU tests compare with agree with the per-node ones."""
import ctypes as C
import inspect

import numpy as np


def test_entry_points_declared(pkg):
    for name in ("svo_adaptive_attach", "svo_adaptive_step", "svo_adaptive_download", "svo_adaptive_length",
                 "svo_adaptive_timing"):
        assert name in pkg._lib.DEVICE_SYMBOLS
        assert hasattr(pkg._lib.lib(), name)
    fields = [f for f, _ in pkg._lib.AdaptiveResult._fields_]
    assert fields == ["n_sub", "n_unsub", "chunks_loaded", "length", "n_removed", "removed"]
    assert C.sizeof(pkg._lib.AdaptiveResult) == 40


def test_loop_default_stays_on_host(pkg):
    sig = inspect.signature(pkg.adaptive.AdaptiveLoop.__init__)
    assert sig.parameters["on_device"].default is False
    assert sig.parameters["incremental"].default is False


def test_octree_bulk_accessors(pkg):
    size = 16
    xyz = np.array([[x, y, z, 1] for x in range(0, 16, 3) for y in range(0, 16, 5) for z in range(0, 16, 7)], dtype=np.uint8)
    pal = np.arange(256, dtype=np.uint32) * 0x010101
    world = pkg.adaptive.World(pkg.CpuOctree.from_voxels(size, xyz, pal))
    octree = world.root_octree()
    world.expand(octree, 3)
    pos = octree.positions()
    assert pos.shape == (len(octree), 3)
    for i in range(0, len(octree), 7):
        assert tuple(pos[i]) == octree.position(i)
    assert octree.hole_stack().size == 0
    interior = np.nonzero((octree.raw_data() >> 4) < pkg.octree.VOXEL_OFFSET)[0]
    node = int(interior[-1])
    group = int(octree.raw_data()[node] >> 4)
    assert octree.unsubdivide(node)
    assert octree.hole_stack().tolist() == [group]
