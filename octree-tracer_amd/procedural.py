"""Procedural world generator: reference src/procedural.rs (Procedural) over the HIP kernels of csrc/svo_proc.hip.

The reference's generator inserts cells into one tree with unsynchronised atomics, so its node order differs from run to
run; this one emits the canonical breadth-first form of the same tree and gives the same bytes every run."""
import ctypes as C

import numpy as np

from ._lib import ProcParams, SvoError, lib
from .cpu_octree import CHUNK_OFFSET, CpuOctree

MAX_NODES = 256000000  # procedural.rs:4
SVO_ERR_CAP = -6
TIMES = ("classify", "pyramid_and_ranks", "emit", "chunk_gpu_wall", "chunk_copy", "chunk_build",
         "world_gpu", "world_copy_and_build", "world_mips", "world_writes")  # svo_proc_timing, ms


def _params(pos, base_depth, chunk_depth, max_nodes=None):
    p = ProcParams()
    p.pos[:] = [float(v) for v in pos]
    p.base_depth = int(base_depth)
    p.chunk_depth = int(chunk_depth)
    p.max_nodes = 0 if max_nodes is None else int(max_nodes)
    return p


def chunk_layout(world_depth):
    """The chunks of generate_world in its loop order (world.rs:100-130): (i, chunk id, lower corner)."""
    n = 1 << world_depth
    vs = np.float32(2.0) / np.float32(n)
    out = []
    for i, (x, y, z) in enumerate((x, y, z) for x in range(n) for y in range(n) for z in range(n)):
        pos = tuple(float(np.float32(c) * vs - np.float32(1.0)) for c in (x, y, z))
        out.append((i, CHUNK_OFFSET // 2 + i, pos))
    return out


class Procedural:
    """procedural.rs:23-29; holds the device context (the reference keeps its own pipeline and buffers)."""

    def __init__(self, gpu):
        self.gpu = gpu

    @classmethod
    def new(cls, gpu):
        return cls(gpu)

    def generate_chunk(self, pos, base_depth, chunk_depth=9, max_nodes=None):
        """procedural.rs:101-199: the chunk with lower corner `pos` as a CpuOctree, or None when no cell is solid.
        A chunk of more than max_nodes nodes (default 256 000 000) raises SvoError; the reference panics."""
        out = C.c_void_p()
        p = _params(pos, base_depth, chunk_depth, max_nodes)
        self.gpu.check(lib().svo_proc_generate_chunk(self.gpu._h, C.byref(p), C.byref(out)))
        return CpuOctree(_handle=out.value) if out.value else None

    def sdf(self, xyz):
        """diagnostic: the island's signed distance at points (n, 3) float32"""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = np.empty(xyz.shape[0], dtype=np.float32)
        self.gpu.check(lib().svo_proc_sdf(self.gpu._h, xyz.ctypes.data, xyz.shape[0], out.ctypes.data))
        return out

    def classify(self, pos, base_depth, chunk_depth=9):
        """diagnostic: class bytes (0 empty, 1 stone, 3 grass) in the reference's id order x + side*y + side^2*z"""
        out = np.empty(1 << (3 * chunk_depth), dtype=np.uint8)
        p = _params(pos, base_depth, chunk_depth)
        self.gpu.check(lib().svo_proc_classify(self.gpu._h, C.byref(p), out.ctypes.data))
        return out

    def timing(self):
        """ms of the last generate_chunk / generate_world phases (svo_proc_timing), by name"""
        return dict(zip(TIMES, self.gpu._timing(lib().svo_proc_timing, len(TIMES))))


__all__ = ["Procedural", "chunk_layout", "MAX_NODES", "SvoError"]
