"""Voxel structures for scattering over a tree (reference src/cpu_octree.rs:213-230, CpuOctree::load_structure;
DESIGN.md 22): a .vox model of any size as offsets from its foot, ready for Render.stamp_structures, place_structures and
scatter_structures.

    Structure        offsets (m, 3) int32, index (m) uint32, colours (m) uint32, in the file's voxel order
    load_structure   a .vox file -> Structure
"""
import ctypes as C

import numpy as np

from ._device import device_u32
from ._lib import lib


class Structure:
    """offsets: (size.x / 2 - x, z, y - size.y / 2) per voxel, integer division as in the reference: the model stands on
    y = 0, centred on its x and z.  index: voxel.i + 1, the reference's block id of the voxel (kept for put_in_block
    instancing; nothing here reads it).  colours: 0x00RRGGBB of the voxel's palette entry; 0 removes a cell when stamped."""

    def __init__(self, offsets, index, colours):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, 3)
        self.index = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1)
        self.colours = np.ascontiguousarray(colours, dtype=np.uint32).reshape(-1)
        if not len(self.offsets) == self.index.size == self.colours.size:
            raise ValueError(f"{len(self.offsets)} offsets, {self.index.size} indices and {self.colours.size} colours")
        self._device = {}

    def __len__(self):
        return len(self.offsets)

    def on(self, dev):
        """(offsets (m, 3), colours (m)) as int32 tensors on `dev`, made once per device"""
        if dev not in self._device:
            self._device[dev] = (device_u32(self.offsets, dev, signed=True), device_u32(self.colours.astype(np.int64), dev))
        return self._device[dev]

    @classmethod
    def _load(cls, path, data):
        err = C.create_string_buffer(256)
        args = (path, data, len(data) if data is not None else 0)
        n = lib().svo_structure_load(*args, None, None, None, 0, err, 256)
        if n < 0:
            raise ValueError(err.value.decode() or "load failed")
        offsets, index, colours = np.empty((n, 3), dtype=np.int32), np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        lib().svo_structure_load(*args, offsets.ctypes.data, index.ctypes.data, colours.ctypes.data, n, err, 256)
        return cls(offsets, index, colours)

    @classmethod
    def from_vox_bytes(cls, data: bytes):
        """model 0 of a .vox held in memory (svo_structure_load)"""
        return cls._load(None, bytes(data))


def load_structure(path):
    """cpu_octree.rs:213-230: model 0 of the .vox file at `path` (svo_structure_load)"""
    return Structure._load(str(path).encode(), None)
