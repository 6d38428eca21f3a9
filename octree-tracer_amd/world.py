"""Chunk table with block instancing: reference src/world.rs (World)."""
import ctypes as C
import os

import numpy as np

from ._lib import lib
from .cpu_octree import CpuOctree
from .octree import Voxel

BLOCK_NAMES = ("stone", "dirt", "grass", "wood", "leaf", "slate", "crystal", "glass")  # ids 1..8, world.rs:19-58


class World:
    """world.rs:5-9.  Chunk 0 is the root tree; a leaf whose pointer is CHUNK_OFFSET + id continues in chunk
    `id` (ids 1..8: the 16^3 block models; ids >= CHUNK_OFFSET / 2: streamed terrain chunks)."""

    def __init__(self, path="", _handle=None):
        self._h = _handle if _handle else lib().svo_world_new(str(path).encode())
        self.path = str(path)

    @classmethod
    def new(cls, path="", blocks_dir=None):
        """World::new.  The reference loads blocks/<name>.vox as chunks 1..8 from its working directory
        (world.rs:19-58); here that happens only when the directory is given."""
        w = cls(path)
        if blocks_dir is not None:
            for i, name in enumerate(BLOCK_NAMES):
                w.insert(i + 1, CpuOctree.load_file(os.path.join(blocks_dir, name + ".vox"), 0))
                w.generate_mip_tree(i + 1)
        return w

    @classmethod
    def load_world(cls, path):
        """world.rs:159-174"""
        if not os.path.exists(path):
            raise ValueError("File doesn't exist!")
        err = C.create_string_buffer(256)
        h = lib().svo_world_load(str(path).encode(), err, 256)
        if not h:
            raise ValueError(err.value.decode())
        return cls(path, _handle=h)

    @staticmethod
    def generate_world(path, procedural, world_depth=1, chunk_depth=9, blocks_dir=None):
        """world.rs:63-139: write a new world to directory `path` (which must not exist; the reference's rule that
        empties an existing directory named "tmp" is not kept).  Every non-empty chunk becomes <id>.bin, the root
        0.bin; open the result with World.load_world(path).  The mips need blocks 1..8 (blocks_dir, as World.new)."""
        if os.path.exists(path):
            raise ValueError("File already exists")
        if blocks_dir is None:
            raise ValueError("generate_world needs blocks_dir: the mips of the chunks take blocks 1..8's colours")
        w = World.new(path, blocks_dir)
        procedural.gpu.check(lib().svo_world_generate(procedural.gpu._h, w._h, int(world_depth), int(chunk_depth)))

    @staticmethod
    def build_world(path, gpu, coords, depth, colours=None, world_depth=1, colour=0xFFFFFF, max_nodes=None):
        """Write a new streamable world to directory `path` (which must not exist) from (N, 3) voxel cells in
        [0, 2^depth), built on the GPU (svo_world_build): chunk (cx, cy, cz) = the top world_depth bits of
        the cells, <id>.bin per non-empty chunk with its mips, 0.bin the root as generate_world makes it.  colours:
        0x00RRGGBB per voxel (None: `colour`).  A chunk of more than max_nodes nodes (default 256 000 000) raises
        SvoError and nothing is created.  Returns World.load_world(path)."""
        from .cpu_octree import _chunk_inputs
        w = World(path)
        (xyz, col, n, p), tensors = _chunk_inputs(gpu, coords, depth, colours, colour, world_depth, max_nodes)  # (the tensors: held across the call)
        gpu.check(lib().svo_world_build(gpu._h, w._h, xyz, col, n, C.byref(p)))
        return World.load_world(path)

    @staticmethod
    def save_nodes(path, render, depth, world_depth=1):
        """Save the tree in `render`'s node buffer as a new streamable world in directory `path` (which must not exist):
        Render.list_voxels(depth, expand=True) followed by build_world of that list; nothing but the chunk
        files leaves the device.  A tree deeper than `depth` raises SvoError and nothing is created.  Returns
        World.load_world(path)."""
        coords, colours = render.list_voxels(depth, expand=True)
        return World.build_world(path, render.gpu, coords, depth, colours, world_depth)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (module globals are gone at interpreter exit)
            lib().svo_world_free(self._h)
        self._h = None

    def _check(self, rc):
        if rc < 0:
            raise RuntimeError(lib().svo_world_last_error(self._h).decode())  # the reference panics (unwrap)
        return rc

    def insert(self, chunk_id, chunk: CpuOctree):
        """chunks.insert(id, chunk): the world owns the chunk from here on."""
        self._check(lib().svo_world_insert(self._h, chunk_id, chunk._h))
        chunk._owned = False

    def remove(self, chunk_id):
        return lib().svo_world_remove(self._h, chunk_id) == 0

    def contains(self, chunk_id):
        return bool(lib().svo_world_chunk(self._h, chunk_id))

    def chunk(self, chunk_id):
        h = lib().svo_world_chunk(self._h, chunk_id)
        if not h:
            raise KeyError(chunk_id)
        return CpuOctree(_handle=h, _owned=False)  # borrowed: valid while the world holds the chunk

    def chunk_ids(self):
        n = lib().svo_world_chunk_ids(self._h, None, 0)
        ids = np.empty(n, dtype=np.uint32)
        lib().svo_world_chunk_ids(self._h, ids.ctypes.data, n)
        return ids.tolist()

    def find_voxel(self, pos, max_depth=None):
        """world.rs:201-232 -> (chunk, index, depth, pos)"""
        ch, idx, d, out = C.c_uint32(), C.c_uint64(), C.c_uint32(), (C.c_float * 3)()
        self._check(lib().svo_world_find_voxel(self._h, (C.c_float * 3)(*pos), -1 if max_depth is None else max_depth,
                                               C.byref(ch), C.byref(idx), C.byref(d), out))
        return ch.value, idx.value, d.value, tuple(out)

    def generate_mip_tree(self, chunk_id):
        """world.rs:234-336; returns the chunk's top_mip"""
        top = (C.c_uint8 * 3)()
        self._check(lib().svo_world_generate_mip_tree(self._h, chunk_id, top))
        return Voxel(*top)

    def save_chunk(self, chunk_id):
        self._check(lib().svo_world_save_chunk(self._h, chunk_id))

    def load_chunk(self, chunk_id):
        self._check(lib().svo_world_load_chunk(self._h, chunk_id))

    def get_node_mask(self, first_child, chunk_id=0):
        return self.chunk(chunk_id).get_node_mask(first_child)

    def root_octree(self):
        """App::new (app.rs:47-48): the device tree starts as the root chunk's 8 mip-coloured children."""
        from .octree import Octree
        return Octree.new(self.get_node_mask(0))

    def expand(self, octree, max_depth, cam=None, lod_c=0.0, max_words=1 << 27):
        """Fixed point of the subdivision loop for a distance rule (svo_world_expand); returns #subdivisions."""
        camv = (C.c_float * 3)(*(cam if cam is not None else (0.0, 0.0, 0.0)))
        return lib().svo_world_expand(self._h, octree._h, max_depth, camv, float(lod_c if cam is not None else 0.0),
                                      max_words)
