"""View-dependent LOD streaming on top of the device scan: reference src/adaptive.rs
(process_subdivision :6-68, process_unsubdivision :70-126) and the frame update of src/app.rs:94-118.
The list processing itself is native: on the host (svo_adaptive_subdivide / svo_adaptive_unsubdivide) or, with
AdaptiveLoop(on_device=True) / DeviceAdaptive, on the GPU (svo_adaptive_step).  DeviceAdaptive.expand is
the device form of World.expand (svo_adaptive_expand)."""
import ctypes as C

import numpy as np
import torch

from ._device import wait_for_torch
from ._lib import AdaptiveResult, lib
from .gpu import OPT_SCAN_CLEARS_COUNTERS
from .world import World as _World


def World(chunk0=None, path=""):
    """A world around one root chunk (App::new, app.rs:33-36): insert as chunk 0 and build its mip colours."""
    w = _World(path)
    if chunk0 is not None:
        w.insert(0, chunk0)
        w.top_mip = w.generate_mip_tree(0)
    return w


def _list(nodes):
    return np.ascontiguousarray(nodes, dtype=np.uint32)


def process_subdivision(compute_lists, octree, world):
    """adaptive.rs:29-61 over the subdivide list: hot leaves get their 8 children from the CPU world (the
    root group of the referenced chunk at a block leaf).  Returns the number of subdivisions."""
    nodes = _list(compute_lists)
    done = lib().svo_adaptive_subdivide(world._h, octree._h, nodes.ctypes.data, nodes.size, None)
    return world._check(done)


def process_unsubdivision(compute_lists, octree, world):
    """adaptive.rs:93-121 over the unsubdivide list: cold interior nodes collapse to their mip colour."""
    nodes = _list(compute_lists)
    done = lib().svo_adaptive_unsubdivide(world._h, octree._h, nodes.ctypes.data, nodes.size)
    return world._check(done)


def _device_list(gpu, nodes):
    """A node list as a contiguous 32-bit tensor on the context's device (torch has no uint32: int32 carries the bits)."""
    dev = gpu.torch_device
    if isinstance(nodes, torch.Tensor):
        t = nodes.to(dev).reshape(-1)
        if t.dtype != torch.int32:
            t = t.to(torch.int64).to(torch.int32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(nodes, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    return t.contiguous()


class DeviceAdaptive:
    """The subdivide / unsubdivide step on the GPU (svo_adaptive_step): the octree's positions, hole stack and length and
    a mirror of the world's resident chunks live with gpu's context; the words stay in render's node buffer.  `world` owns
    the chunk data (loads and removals go through it) and must be kept alive.  Needs OPT_SCAN_CLEARS_COUNTERS = 1."""

    def __init__(self, gpu, render, octree, world):
        self.gpu, self.render, self.octree, self.world = gpu, render, octree, world
        gpu.check(lib().svo_adaptive_attach(gpu._h, world._h, octree._h))
        self.length = len(octree)
        self.last = None  # the last step's svo_adaptive_result, as a dict

    def step(self, sub=None, unsub=None):
        """One step over explicit lists (torch tensors or arrays of node indices, any order) or, with both None, over the
        scan's own lists in place.  Returns (n_sub, n_unsub)."""
        res = AdaptiveResult()
        if sub is None and unsub is None:
            self.gpu.check(lib().svo_adaptive_step(self.gpu._h, None, 0, None, 0, C.byref(res)))
        else:
            s = _device_list(self.gpu, sub if sub is not None else [])
            u = _device_list(self.gpu, unsub if unsub is not None else [])
            wait_for_torch(self.gpu)
            # (an empty list still needs a device pointer: both or neither)
            ps = s.data_ptr() if s.numel() else u.data_ptr() if u.numel() else self._dummy().data_ptr()
            pu = u.data_ptr() if u.numel() else ps
            self.gpu.check(lib().svo_adaptive_step(self.gpu._h, ps, s.numel(), pu, u.numel(), C.byref(res)))
        self.length = res.length
        self.render.node_length = max(self.render.node_length, res.length)
        self.last = {"n_sub": res.n_sub, "n_unsub": res.n_unsub, "chunks_loaded": res.chunks_loaded, "length": res.length,
                     "removed": [res.removed[i] for i in range(res.n_removed)]}
        return res.n_sub, res.n_unsub

    def expand(self, max_depth, cam=None, lod_c=0.0, max_words=None):
        """World.expand(octree, max_depth, cam, lod_c, max_words) on the device state (svo_adaptive_expand): the words,
        positions, length and the returned number of subdivisions equal the host call's, bit for bit; the host octree is
        stale until download().  max_words: None or 0 for the node buffer's capacity (a larger value is clamped to it).
        Raises SvoError for a tree with free groups in its hole stack (expand that one on the host)."""
        res = AdaptiveResult()
        camv = (C.c_float * 3)(*(float(c) for c in cam)) if cam is not None else None
        self.gpu.check(lib().svo_adaptive_expand(self.gpu._h, int(max_depth), camv, float(lod_c if cam is not None else 0.0),
                                                 int(max_words or 0), C.byref(res)))
        self.length = res.length
        self.render.node_length = max(self.render.node_length, res.length)
        self.last = {"n_sub": res.n_sub, "n_unsub": 0, "chunks_loaded": res.chunks_loaded, "length": res.length, "removed": []}
        return res.n_sub

    def expand_timing(self):
        """Of the last expand: ms listing the leaves, choosing candidates, subdividing (device events), host wall ms, levels."""
        out = self.gpu._timing(lib().svo_adaptive_expand_timing, 5)
        return out[:4] + [int(out[4])]

    def _dummy(self):
        if getattr(self, "_one", None) is None:
            self._one = torch.zeros(1, dtype=torch.int32, device=self.gpu.torch_device)
        return self._one

    def download(self):
        """Make the host Octree equal to the device state (words, positions, hole stack, length)."""
        self.gpu.check(lib().svo_adaptive_download(self.gpu._h, self.octree._h))
        return self.octree

    def timing(self):
        """ms of the last step: sort, subdivide, unsubdivide (device events), host wall time."""
        return self.gpu._timing(lib().svo_adaptive_timing, 4)


class AdaptiveLoop:
    """App::update (app.rs:94-118): uniforms -> trace (counters live) -> scan -> CPU (un)subdivide -> re-upload.

    incremental=True replaces the reference's re-upload of the WHOLE array (which is also what resets the hit
    counters: host words carry counter 0) by its device-side equivalent: the scan zeroes the counters it has read
    (SVO_OPT_SCAN_CLEARS_COUNTERS) and only the words the list processing changed are sent (svo_nodes_scatter).
    The device array after a frame is the same either way.

    on_device=True (implies incremental) keeps the list processing on the GPU too (DeviceAdaptive): trace -> scan ->
    svo_adaptive_step over the scan's lists in place; no list and no word crosses PCIe.  The frames equal those of
    incremental=True with deterministic=True; the host `octree` is stale until download().

    device=<DeviceAdaptive> (implies on_device) continues from a state that is already attached, e.g. the one
    Render.from_world returns: no second attach, and `octree` may be its stale host octree."""

    def __init__(self, gpu, render, compute, octree, world, incremental=False, on_device=False, device=None):
        self.gpu, self.render, self.compute, self.octree, self.world = gpu, render, compute, octree, world
        on_device = on_device or device is not None
        self.incremental = incremental or on_device
        gpu.set_option(OPT_SCAN_CLEARS_COUNTERS, 1 if self.incremental else 0)
        octree.take_dirty()  # the device already holds the octree as it is now
        self.device = device if device is not None else DeviceAdaptive(gpu, render, octree, world) if on_device else None

    def frame(self, settings, character, deterministic=False):
        self.render.update(settings, character)
        hits = self.render.render()
        if self.render.uniforms.flags & 1:  # pause_adaptive (app.rs:97)
            return hits, 0, 0
        if self.device is not None:  # the lists are always sorted on the device
            self.compute.update(self.device.length)
            n_sub, n_unsub = self.device.step()
            return hits, n_sub, n_unsub
        self.compute.update(len(self.octree))
        sub, unsub = self.compute.read_lists()
        if deterministic:  # the device appends in no particular order; sorted lists make runs repeatable
            sub.sort()
            unsub.sort()
        n_sub = process_subdivision(sub, self.octree, self.world)
        n_unsub = process_unsubdivision(unsub, self.octree, self.world)
        if self.incremental:
            idx, val = self.octree.take_dirty()
            self.render.scatter_nodes(idx, val, node_length=len(self.octree))
        else:
            # app.rs:113-118: the whole array goes back (host words carry counter 0, which also clears the counters)
            self.render.write_nodes(self.octree.raw_data())
        return hits, n_sub, n_unsub

    def download(self):
        """on_device: refresh the host octree from the device state."""
        if self.device is not None:
            self.device.download()
        return self.octree
