"""Trace dispatch: reference src/render.rs (Render::{new, update, render, resize}, Uniforms)."""
import ctypes as C

import numpy as np
import torch

from . import sharding
from ._device import device_u32, voxel_list, wait_for_torch
from ._lib import BuildParams, CombineParams, CompactParams, ComponentsParams, DistanceParams, EditParams, HeightmapParams, ListParams, MorphParams, PlaceParams, RegionParams, SampleParams, SimplifyParams, SitesParams, StampParams, SurfaceMergeParams, SurfaceParams, TopsParams, TransformParams, SvoError, Uniforms, lib
from .camera import camera_matrices

F_PAUSE_ADAPTIVE, F_SHOW_STEPS, F_SHOW_HITS, F_SHADOWS, F_MISC_BOOL = 1, 2, 4, 8, 16
HIT_DTYPE = np.dtype([("value", "<u4"), ("t", "<f4"), ("info", "<u4"), ("normal_bits", "<u4")])
DEFAULT_NODE_CAPACITY = 10_000_000  # render.rs:53
EMPTY_WORD = (1 << 27) << 4  # an empty slot: (VOXEL_OFFSET + colour 0) << 4
# what sample_voxels / sample_dense return in place of a value (svo_hip.h): the tree is interior at `depth` in the cell; a
# coordinate is outside the grid; the path met a pointer that is unaligned or leaves the tree's words
SAMPLE_FINER, SAMPLE_OUTSIDE, SAMPLE_BROKEN = 1 << 28, 1 << 29, 1 << 30
TOP_NONE = -1  # what column_tops returns for a column that holds nothing: SVO_TOP_NONE = 0xFFFFFFFF read as int32
# structure_sites and stamp_structures know a bound of their list before they call (the columns, placements x voxels): up
# to this many entries they fill room for the bound in one call and return its first part, without the count query
ONE_CALL_ENTRIES = 1 << 20
COMBINE_OPS = ("over", "under", "paint", "carve", "keep", "replace")  # combine_nodes: SVO_COMBINE_OVER .. SVO_COMBINE_REPLACE
MORPH_OPS = ("grow", "shrink", "close", "open")  # morph_nodes: SVO_MORPH_GROW, SVO_MORPH_SHRINK and their two compositions
HEIGHTMAP_MODES = (None, "empty", "voxels", "set")  # edit_heightmap's below / above: 0, SVO_REGION_EMPTY, _VOXELS, _SET


def _heightmap_mode(mode, which):
    if mode not in HEIGHTMAP_MODES:
        raise ValueError(f"{which} must be None, 'empty', 'voxels' or 'set' (got {mode!r})")
    return HEIGHTMAP_MODES.index(mode)


class Render:
    """Owns the device node buffer and the uniforms, like the reference's Render.

    Render.new(gpu, size, octree)  render.rs:18-180 (node buffer = octree.expanded(capacity))
    update(settings, character)    render.rs:191-215
    render(...)                    render.rs:217-284: one pass over every pixel
    resize(size)                   render.rs:182-189
    """

    def __init__(self, gpu, size, octree_words, capacity=None):
        self.gpu = gpu
        self.size = (int(size[0]), int(size[1]))
        words = np.ascontiguousarray(octree_words, dtype=np.uint32)
        cap = capacity if capacity is not None else max(DEFAULT_NODE_CAPACITY, words.size)
        cap = max(cap, words.size, 8)
        gpu.check(lib().svo_nodes_alloc(gpu._h, cap))
        self.capacity = cap
        self.node_length = 0
        self.uniforms = Uniforms()
        self.uniforms.sun_dir[:] = [-1.7, -1.0, 0.8, 0.0]  # render.rs:312
        self.uniforms.flags = F_SHADOWS                     # render.rs:313-316 defaults
        self.write_nodes(words)

    @classmethod
    def share_nodes(cls, gpu, other):
        """A second Render on another context (its own stream) over the SAME device node buffer (zero copy):
        svo_nodes_share.  Used to keep more than one frame in flight.  The contexts share the buffer's generation counter:
        a write through either one (write_nodes, scatter_nodes, the adaptive loop) makes every one of them rebuild its top
        table and schedule before its next trace, which also waits on the device for that write.  A write does not wait
        for frames other lanes still have in flight -- sync them first."""
        self = cls.__new__(cls)
        self.gpu, self.size = gpu, other.size
        gpu.check(lib().svo_nodes_share(gpu._h, other.gpu._h))
        self.capacity, self.node_length = other.capacity, other.node_length
        self.uniforms = Uniforms()
        C.memmove(C.byref(self.uniforms), C.byref(other.uniforms), C.sizeof(Uniforms))
        self.upload_uniforms()
        return self

    @classmethod
    def new(cls, gpu, size, octree, capacity=None):
        words = octree.raw_data() if hasattr(octree, "raw_data") else octree
        return cls(gpu, size, words, capacity)

    @classmethod
    def from_world(cls, gpu, size, world, max_depth, cam=None, lod_c=0.0, capacity=None):
        """A Render whose tree is `world` expanded to a view's level of detail on the GPU: the root
        chunk's 8 children are uploaded, the device adaptive state is attached (OPT_SCAN_CLEARS_COUNTERS is set) and
        DeviceAdaptive.expand(max_depth, cam, lod_c) refines them in place, as World.expand does on the host.  Returns
        (render, device_adaptive); device_adaptive.octree is the 8-node host octree, stale until download(), and can be
        handed to AdaptiveLoop(..., device=device_adaptive) to go on streaming without a second attach."""
        from .adaptive import DeviceAdaptive
        from .gpu import OPT_SCAN_CLEARS_COUNTERS
        octree = world.root_octree()
        self = cls(gpu, size, octree.raw_data(), capacity)
        gpu.declare_depth(max_depth)
        gpu.set_option(OPT_SCAN_CLEARS_COUNTERS, 1)
        device = DeviceAdaptive(gpu, self, octree, world)
        device.expand(max_depth, cam=cam, lod_c=lod_c)
        return self, device

    def write_nodes(self, words, offset=0):
        """queue.write_buffer(&node_buffer, 0, nodes) (app.rs:113-118)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        self.gpu.check(lib().svo_nodes_write(self.gpu._h, offset, words.ctypes.data, words.size))
        self.gpu.sync()  # the host array may be released by the caller
        self.node_length = max(self.node_length, offset + words.size)

    @classmethod
    def from_voxels(cls, gpu, size, coords, depth, colours=None, capacity=None):
        """A Render whose tree is built on the GPU from a voxel list (build_nodes)."""
        self = cls(gpu, size, np.full(8, EMPTY_WORD, dtype=np.uint32), capacity)
        self.build_nodes(coords, depth, colours)
        return self

    @classmethod
    def from_mesh(cls, gpu, size, vertices, triangles, depth, colours=None, capacity=None, solid=False, fill_colour=None,
                  rule="evenodd", allow_open=False, merge=False):
        """A Render whose tree is a triangle mesh voxelised and built on the GPU (build_nodes_mesh)."""
        self = cls(gpu, size, np.full(8, EMPTY_WORD, dtype=np.uint32), capacity)
        self.build_nodes_mesh(vertices, triangles, depth, colours, solid=solid, fill_colour=fill_colour, rule=rule, allow_open=allow_open,
                              merge=merge)
        return self

    def build_nodes_mesh(self, vertices, triangles, depth, colours=None, colour=0xFFFFFF, max_words=None, quantized=False,
                         solid=False, fill_colour=None, rule="evenodd", allow_open=False, merge=False):
        """Voxelise a triangle mesh on the GPU (mesh.voxelize) and build the tree of its cells into the node
        buffer from word 0 (build_nodes).  vertices: (V, 3) floats in [-1, 1), or with quantized=True the integers of
        mesh.quantize_vertices; triangles: (T, 3) vertex indices; colours: T values 0x00RRGGBB or None (every triangle
        `colour`).  The highest triangle index colours a cell that several triangles touch.  solid: the cells inside the
        mesh (mesh.voxelize_solid with `rule`) in fill_colour (None: `colour`) stand in front of the surface's
        list, so the surface keeps its triangles' colours (the last entry in input order wins); a mesh with open columns
        raises ValueError unless allow_open.  merge: the lossless simplify_nodes() after the build, so that a solid model
        comes in with coarse interior leaves (mind its docstring before putting voxels in by edit_nodes).  Returns the
        word count."""
        from .mesh import voxelize, voxelize_solid
        coords, cell_colours = voxelize(self.gpu, vertices, triangles, depth, colours, colour, quantized=quantized)
        if solid:
            inner, n_open = voxelize_solid(self.gpu, vertices, triangles, depth, rule, with_open=True, quantized=quantized)
            if n_open and not allow_open:
                raise ValueError(f"the mesh is not closed: {n_open} columns are open (allow_open=True fills them by the rule all the same)")
            fill = int(colour if fill_colour is None else fill_colour) & 0xFFFFFF
            coords = torch.cat([inner, coords])
            cell_colours = torch.cat([torch.full((len(inner),), fill, dtype=torch.int32, device=inner.device), cell_colours])
        n = self.build_nodes(coords, depth, cell_colours, max_words=max_words)
        return self.simplify_nodes() if merge else n

    def build_nodes(self, coords, depth, colours=None, colour=0xFFFFFF, max_words=None):
        """Build the tree of a voxel list on the GPU into the node buffer from word 0 (svo_nodes_build).
        coords: (N, 3) integer cells in [0, 2^depth), a torch tensor on this context's device or numpy (copied there);
        colours: N values 0x00RRGGBB or None (every voxel `colour`).  Returns the word count."""
        xyz, col, n, xyz_ptr, col_ptr = voxel_list(self.gpu, coords, colours)
        p = self._build_params(depth, colour, max_words)
        out = C.c_uint64()
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_build(self.gpu._h, xyz_ptr, col_ptr, n, C.byref(p), C.byref(out)))
        self.gpu.sync()  # (the inputs may be released by the caller)
        self.node_length = out.value
        return out.value

    def edit_nodes(self, coords, depth, colours=None, colour=0xFFFFFF, max_words=None):
        """Put voxels into the tree that is in the node buffer, in place (svo_nodes_edit): what put_in_voxel
        per distinct cell makes of the first node_length words; colour 0 removes a voxel; a coarser leaf on the way is split
        into empty children.  Inputs as build_nodes.  A cell the tree refines below `depth` raises SvoError and nothing is
        written.  Returns the new length (node_length)."""
        xyz, col, n, xyz_ptr, col_ptr = voxel_list(self.gpu, coords, colours)
        depth = int(depth)
        self.gpu.declare_depth(depth)
        p = EditParams()
        p.depth = max(0, depth)
        p.default_colour = int(colour) & 0xFFFFFF
        p.n_words = int(self.node_length)
        p.max_words = int(max_words or 0)
        out = C.c_uint64()
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_edit(self.gpu._h, xyz_ptr, col_ptr, n, C.byref(p), C.byref(out)))
        self.gpu.sync()  # (the inputs may be released by the caller)
        self.node_length = out.value
        return out.value

    def edit_region(self, shapes, depth=None, max_words=None):
        """Fill, carve and paint the tree that is in the node buffer by shapes, in place (svo_nodes_edit_region, DESIGN.md
        25).  shapes: region.box(...) and region.ball(...) in the order they apply, at most 1 024; per cell of the `depth`
        grid a shape inside which the cell lies, and whose mode names the cell's state, sets the cell to its colour (0
        empties it).  A node wholly inside a SET shape becomes one leaf, a node wholly outside is not looked at, a coarse
        leaf on a shape's surface is split and keeps its colour in the children.  Boxes are clipped to the grid.  Where the
        tree is finer than `depth` under a shape that does not replace it, SvoError is raised and nothing is written.
        depth=None: the depth declared for this tree.  Returns the new length (node_length)."""
        from .region import pack
        depth = int(self.gpu.tree_depth if depth is None else depth)
        arr, n = pack(shapes, depth)
        self.gpu.declare_depth(depth)
        p = RegionParams()
        p.depth = max(0, depth)
        p.n_words = int(self.node_length)
        p.max_words = int(max_words or 0)
        out = C.c_uint64()
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_edit_region(self.gpu._h, arr, n, C.byref(p), C.byref(out)))
        self.gpu.sync()
        self.node_length = out.value
        return out.value

    def _heightmap(self, heights, layers, origin_xz, depth):
        """the height map and its rectangle as the library takes them: -> (params without modes and lengths, the int32
        device tensor [sx, sz] of u32 bit patterns, its address or None)"""
        depth = int(self.gpu.tree_depth if depth is None else depth)
        if not isinstance(heights, torch.Tensor):
            heights = np.ascontiguousarray(heights)
            if heights.dtype.kind == "u":  # (torch has no arithmetic for the wide unsigned types)
                heights = np.minimum(heights, 0xFFFFFFFF).astype(np.int64)
        t = torch.as_tensor(heights)
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise TypeError(f"heights: integer input expected, got {t.dtype}")
        if t.dim() != 2:
            raise ValueError(f"heights must be (size_x, size_z), got {tuple(t.shape)}")
        t = t.to(self.gpu.torch_device)
        if t.dtype != torch.int32:  # a negative height is 0, one above 2^32 - 1 is that: the library clamps to the grid
            t = t.to(torch.int64).clamp(0, 0xFFFFFFFF)
            t = torch.where(t >= 1 << 31, t - (1 << 32), t)
        t = t.to(torch.int32).contiguous()
        o = [int(v) for v in origin_xz]
        if len(o) != 2 or min(o) < 0 or max(o) >= 1 << 32:
            raise ValueError(f"origin_xz must be 2 values in [0, 2^32), got {o}")
        layers = [(int(th), int(colour)) for th, colour in layers]
        if len(layers) > len(HeightmapParams().layers):
            raise ValueError(f"{len(layers)} layers, more than {len(HeightmapParams().layers)}")
        if any(th < 0 or th >= 1 << 32 for th, _ in layers):
            raise ValueError(f"a layer's thickness must be in [0, 2^32), got {[th for th, _ in layers]}")
        p = HeightmapParams()
        p.depth = max(0, depth)
        p.n_layers = len(layers)
        p.origin_xz[:] = o
        p.size_xz[:] = list(t.shape)
        for k, (th, colour) in enumerate(layers):
            p.layers[k].thickness, p.layers[k].colour = th, colour & 0xFFFFFF
        return p, t, (t.data_ptr() if t.numel() else None)

    def edit_heightmap(self, heights, layers=((0, 0xFFFFFF),), origin_xz=(0, 0), depth=None, below="set", above=None, above_colour=0,
                       max_words=None):
        """Shape the tree that is in the node buffer by a height map, in place (svo_nodes_edit_heightmap):
        raise, lower and layer terrain.  heights: a device int32 tensor [size_x, size_z] (u32 bit patterns; or numpy or any
        integer tensor, copied there, negative values taken as 0), the number of ground cells of the column (origin_xz[0] +
        i, origin_xz[1] + k) of the `depth` grid, y up; a height above the grid is clamped.  layers: up to 8 (thickness,
        colour) from the ground's top cell down; the last one's thickness is ignored, it reaches down to y = 0; a colour of
        0 is empty.  below / above: what the cells under the ground / at and above it must be to be set, None (leave that
        side alone), "empty", "voxels" or "set" (both); the cells under the ground get their layer's colour, the others
        above_colour (0 carves).  Coarse leaves stay coarse away from the ground's surface: a cube wholly below, within one
        layer, or wholly above becomes or stays one leaf, a leaf on the surface is split and keeps its colour in the
        children; equal siblings that a split leaves behind are simplify_nodes' to merge.  Where the tree is finer than
        `depth` under a mode that does not replace it, SvoError is raised and nothing is written.  depth=None: the depth
        declared for this tree.  Returns the new length (node_length)."""
        p, t, ptr = self._heightmap(heights, layers, origin_xz, depth)
        self.gpu.declare_depth(p.depth)
        p.mode_below, p.mode_above = _heightmap_mode(below, "below"), _heightmap_mode(above, "above")
        p.colour_above = int(above_colour) & 0xFFFFFF
        p.n_words = int(self.node_length)
        p.max_words = int(max_words or 0)
        out = C.c_uint64()
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_edit_heightmap(self.gpu._h, C.byref(p), ptr, C.byref(out)))
        self.gpu.sync()  # (the map may be released by the caller)
        self.node_length = out.value
        return out.value

    def height_minmax(self, heights, s, origin_xz=(0, 0), depth=None):
        """Level s (1..depth) of the min/max pyramid that edit_heightmap walks by (svo_heightmap_minmax): an
        int32 device tensor [nx, nz, 2] with one (min, max) pair of the clamped heights per octree-aligned tile of 2^s x
        2^s columns that meets the map's rectangle, tile (origin >> s) + (i, k) at [i, k]; the columns outside the
        rectangle do not count.  heights, origin_xz and depth as in edit_heightmap."""
        p, t, ptr = self._heightmap(heights, (), origin_xz, depth)
        s = int(s)
        fits = 1 <= s <= p.depth <= 21 and t.numel() and all(a + b <= 1 << p.depth for a, b in zip(p.origin_xz, p.size_xz))
        shape = [((a + b - 1) >> s) - (a >> s) + 1 for a, b in zip(p.origin_xz, p.size_xz)] if fits else [0, 0]
        out = torch.empty(shape + [2], dtype=torch.int32, device=self.gpu.torch_device)
        room = out if out.numel() else torch.empty(2, dtype=torch.int32, device=self.gpu.torch_device)  # (nothing is written to it)
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_heightmap_minmax(self.gpu._h, C.byref(p), ptr, min(max(s, 0), 0xFFFFFFFF), room.data_ptr()))
        self.gpu.sync()  # (the map may be released by the caller)
        return out

    @classmethod
    def from_heightmap(cls, gpu, size, heights, depth, layers=((0, 0xFFFFFF),), capacity=None):
        """A Render whose tree is the solid terrain of a height map over the whole `depth` grid's floor, made on the GPU from
        the empty root group (edit_heightmap): its coarse leaves never existed as cells."""
        self = cls(gpu, size, np.full(8, EMPTY_WORD, dtype=np.uint32), capacity)
        self.edit_heightmap(heights, layers, (0, 0), depth)
        return self

    def _source_tree(self, source):
        """a second device tree that a pass only reads, in the three forms combine_nodes and place_nodes take: -> (address,
        length in words, what keeps the words alive until the call returns)"""
        if isinstance(source, Render):
            if source.gpu.device != self.gpu.device:
                raise ValueError(f"the source is on device {source.gpu.device}, the scene on device {self.gpu.device}")
            ptr, room = C.c_void_p(), C.c_size_t()
            source.gpu.check(lib().svo_nodes_device_ptr(source.gpu._h, C.byref(ptr), C.byref(room)))
            source.gpu.sync()  # (its words may still be on their way on its own stream)
            return ptr.value, int(source.node_length), source
        words, length = source if isinstance(source, tuple) else (source, None)
        words = device_u32(words, self.gpu.torch_device, what="source").reshape(-1)
        src_words = int(words.numel() if length is None else length)
        if src_words > words.numel():
            raise ValueError(f"the source holds {words.numel()} words, fewer than its length {src_words}")
        return (words.data_ptr() if words.numel() else None), src_words, words

    def combine_nodes(self, source, op="over", depth=None, at=(0, 0, 0), at_level=0, max_words=None):
        """Combine the tree that is in the node buffer, the scene, with a second device tree, the source, in place
        (svo_nodes_combine).  source: another Render on the same device (its first node_length words), a
        device int32 tensor of words, or a (tensor, length) pair as simplify_nodes(out_of_place=True) returns; it is only
        read.  op, a name of COMBINE_OPS or its number, per cell with a the scene's value and b the source's: "over" b or
        else a (paste), "under" a or else b (fill the empty cells), "paint" b where both hold a voxel, "carve" empty where
        the source holds a voxel, "keep" empty where it holds none, "replace" b.  The source's cube is the scene's cell `at`
        of level at_level (0: the whole scene) and is `depth - at_level` levels deep; the cells outside it stay as they are.
        Coarse leaves stay coarse: a subtree that the source decides as a whole becomes one leaf, a leaf on the source's
        surface is split and keeps its colour in the children.  Where either tree is finer than `depth` and the op has to
        look below, SvoError is raised and nothing is written.  depth=None: the depth declared for this tree.  Returns the
        new length (node_length)."""
        depth = int(self.gpu.tree_depth if depth is None else depth)
        if isinstance(op, str):
            if op not in COMBINE_OPS:
                raise ValueError(f"op must be one of {', '.join(COMBINE_OPS)} (got {op!r})")
            op = COMBINE_OPS.index(op)
        src_ptr, src_words, _held = self._source_tree(source)
        if len(at) != 3:
            raise ValueError(f"at must be three cell coordinates, got {at!r}")
        self.gpu.declare_depth(depth)
        p = CombineParams()
        p.op = max(0, int(op))
        p.depth = max(0, depth)
        p.at_level = max(0, int(at_level))
        p.at[:] = [min(max(0, int(v)), 0xFFFFFFFF) for v in at]
        p.n_words = int(self.node_length)
        p.src_words = src_words
        p.max_words = int(max_words or 0)
        out = C.c_uint64()
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_combine(self.gpu._h, src_ptr, C.byref(p), C.byref(out)))
        self.gpu.sync()  # (the source may be released by the caller)
        self.node_length = out.value
        return out.value

    def place_nodes(self, source, op="over", depth=None, offset=(0, 0, 0), orient=0, src_depth=None, max_words=None):
        """Place a second device tree, the source, into the tree that is in the node buffer, the scene, at any cell offset and
        in any of the cube's 48 orientations, in place (svo_nodes_place): combine_nodes without the condition
        that the source's cube is a cell of the scene's octree.  source and op are combine_nodes'.  The source is a cube of
        2^src_depth cells a side (None: `depth`) whose cells are the scene's; oriented by `orient` (orientation.orientation,
        from_matrix, quarter_turns_y; 0: as it is) about its own cube, its cell (0, 0, 0) then lies on the scene's cell
        `offset`, which may be negative or hang over the scene's edge: the part outside is clipped, the cells outside the
        source's cube stay as they are.  Coarse leaves stay coarse where both trees allow it; equal siblings that a split
        leaves behind are simplify_nodes' to merge.  Where either tree is finer than its depth and the op has to look
        below, SvoError is raised and nothing is written.  depth=None: the depth declared for this tree.  Returns the new
        length (node_length)."""
        depth = int(self.gpu.tree_depth if depth is None else depth)
        if isinstance(op, str):
            if op not in COMBINE_OPS:
                raise ValueError(f"op must be one of {', '.join(COMBINE_OPS)} (got {op!r})")
            op = COMBINE_OPS.index(op)
        src_ptr, src_words, _held = self._source_tree(source)
        if len(offset) != 3:
            raise ValueError(f"offset must be three cell coordinates, got {offset!r}")
        self.gpu.declare_depth(depth)
        p = PlaceParams()
        p.op = max(0, int(op))
        p.depth = max(0, depth)
        p.src_depth = max(0, int(depth if src_depth is None else src_depth))
        p.orient = min(max(0, int(orient)), 0xFFFFFFFF)
        p.offset[:] = [min(max(-0x80000000, int(v)), 0x7FFFFFFF) for v in offset]
        p.n_words = int(self.node_length)
        p.src_words = src_words
        p.max_words = int(max_words or 0)
        out = C.c_uint64()
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_place(self.gpu._h, src_ptr, C.byref(p), C.byref(out)))
        self.gpu.sync()  # (the source may be released by the caller)
        self.node_length = out.value
        return out.value

    def transform_nodes(self, source, op="over", depth=None, matrix=(65536, 0, 0, 0, 65536, 0, 0, 0, 65536), translate=(0, 0, 0), src_depth=None,
                        max_words=None):
        """Place a second device tree, the source, into the tree that is in the node buffer, the scene, under any affine map,
        in place (svo_nodes_transform): place_nodes with free turns, scale and shear, and a source whose cells
        need not be the scene's.  source and op are combine_nodes'.  matrix (9 integers, row-major) and translate (3) are
        Q16 and map SCENE cells to SOURCE cells: the scene cell c samples the source's cell floor(A (c + 1/2) + t), the
        nearest cell to its centre, and stays as it is where that lies outside the source's cube of 2^src_depth cells a side
        (None: `depth`).  transform.fixed makes the numbers from a forward map ("turn the model by F about this point, put
        it there"), transform.from_orientation from place_nodes' arguments, transform.source_cell predicts q.  Coarse
        leaves stay coarse where both trees allow it; equal siblings that a split leaves behind are simplify_nodes' to
        merge.  Point sampling aliases where the map shrinks the source: simplify_nodes(cut_level=...) on the source first.
        Where either tree is finer than its depth and the op has to look below, SvoError is raised and nothing is written.
        depth=None: the depth declared for this tree.  Returns the new length (node_length)."""
        depth = int(self.gpu.tree_depth if depth is None else depth)
        if isinstance(op, str):
            if op not in COMBINE_OPS:
                raise ValueError(f"op must be one of {', '.join(COMBINE_OPS)} (got {op!r})")
            op = COMBINE_OPS.index(op)
        src_ptr, src_words, _held = self._source_tree(source)
        from .transform import whole_numbers
        matrix, translate = whole_numbers(matrix, "matrix"), whole_numbers(translate, "translate")
        if len(matrix) != 9 or len(translate) != 3:
            raise ValueError(f"matrix must hold 9 numbers and translate 3, got {len(matrix)} and {len(translate)}")
        self.gpu.declare_depth(depth)
        p = TransformParams()
        p.op = max(0, int(op))
        p.depth = max(0, depth)
        p.src_depth = max(0, int(depth if src_depth is None else src_depth))
        p.matrix[:] = [min(max(-0x80000000, v), 0x7FFFFFFF) for v in matrix]
        p.translate[:] = [min(max(-(1 << 63), v), (1 << 63) - 1) for v in translate]
        p.n_words = int(self.node_length)
        p.src_words = src_words
        p.max_words = int(max_words or 0)
        out = C.c_uint64()
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_transform(self.gpu._h, src_ptr, C.byref(p), C.byref(out)))
        self.gpu.sync()  # (the source may be released by the caller)
        self.node_length = out.value
        return out.value

    def _morph_step(self, op, conn, colour, depth, open_boundary, max_words):
        """one svo_nodes_morph call"""
        p = MorphParams()
        p.op = op
        p.conn = min(max(0, int(conn)), 0xFFFFFFFF)
        p.depth = max(0, depth)
        p.flags = 1 if open_boundary else 0
        p.colour = colour
        p.n_words = int(self.node_length)
        p.max_words = int(max_words or 0)
        out = C.c_uint64()
        self.gpu.check(lib().svo_nodes_morph(self.gpu._h, C.byref(p), C.byref(out)))
        self.gpu.sync()
        self.node_length = out.value
        return out.value

    def morph_nodes(self, op, steps=1, conn=26, colour=None, depth=None, open_boundary=False, max_words=None):
        """Mathematical morphology on the tree that is in the node buffer, in place (svo_nodes_morph).  op, a
        name of MORPH_OPS: "grow" adds to the voxels every empty cell that has a voxel among its `conn` (6, 18 or 26)
        neighbours, "shrink" empties every voxel that has an empty cell among them; `steps` such steps are the cube (26),
        the 18-cell shape or the octahedron (6) of radius `steps`.  "close" is `steps` grows and then `steps` shrinks (it
        fills holes and gaps narrower than the shape), "open" the reverse (it removes bridges and specks).  A new cell gets
        `colour`; None or 0: the value of its first neighbour in the order faces, edges, corners, each ascending in (dx,
        dy, dz).  The grid's outside never changes a cell, unless open_boundary lets a shrink take it for empty.  Coarse
        leaves stay coarse away from the surface; equal siblings that a split leaves behind are simplify_nodes' to merge,
        and as every step walks the whole tree a merged tree is the cheap input.  Where the tree is finer than `depth`,
        SvoError is raised by the step that meets it and the steps before it stay.  depth=None: the depth declared for
        this tree.  Returns the new length (node_length)."""
        if op not in MORPH_OPS:
            raise ValueError(f"op must be one of {', '.join(MORPH_OPS)} (got {op!r})")
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"steps must not be negative (got {steps})")
        depth = int(self.gpu.tree_depth if depth is None else depth)
        self.gpu.declare_depth(depth)
        colour = 0 if colour is None else int(colour) & 0xFFFFFF
        order = {"grow": (0,), "shrink": (1,), "close": (0, 1), "open": (1, 0)}[op]
        for step_op in order:
            for _ in range(steps):
                self._morph_step(step_op, conn, 0 if step_op else colour, depth, open_boundary, max_words)
        return int(self.node_length)

    def shell_nodes(self, thickness=1, conn=6, depth=None, closed_boundary=False, max_words=None):
        """Hollow the tree that is in the node buffer to a shell, in place and on the device: every voxel that
        `thickness` shrinks under `conn` would keep is emptied, so `thickness` layers of the solid stay.  The grid's
        boundary exposes (closed_boundary: it covers), as in list_surface: with conn=6 and thickness=1 the voxels left are
        exactly the cells of the leaves that list_surface reports.  Made of a snapshot (simplify_nodes out of place), the
        shrinks, a second snapshot, and two combine_nodes: the first snapshot back by "replace", the second carved out of
        it.  Raises as those do; an error leaves the shrunk tree of the steps that ran.  Returns the new length
        (node_length); simplify_nodes merges the interior that the carve emptied."""
        depth = int(self.gpu.tree_depth if depth is None else depth)
        whole = self.simplify_nodes(out_of_place=True)
        self.morph_nodes("shrink", steps=thickness, conn=conn, depth=depth, open_boundary=not closed_boundary, max_words=max_words)
        core = self.simplify_nodes(out_of_place=True)
        self.combine_nodes(whole, "replace", depth=depth, max_words=max_words)
        return self.combine_nodes(core, "carve", depth=depth, max_words=max_words)

    def compact_nodes(self, prune=True, with_perm=False):
        """Compact the first node_length words of the node buffer in place (svo_nodes_compact): unreachable
        groups go, with `prune` also the groups that hold nothing (a word pointing at one becomes the empty word), and
        the rest comes out in the builder's breadth-first order; the freed tail holds the empty word.  Raises SvoError,
        with nothing written, for a malformed tree or with a device adaptive state attached.  Sets node_length to the new
        length and returns it; with_perm: (length, perm) with perm[new word] = old word as a device int32 tensor."""
        p = CompactParams()
        p.flags = 1 if prune else 0
        p.n_words = int(self.node_length)
        perm = torch.empty(max(int(self.node_length), 1), dtype=torch.int32, device=self.gpu.torch_device) if with_perm else None
        out = C.c_uint64()
        if with_perm:
            wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_compact(self.gpu._h, C.byref(p), perm.data_ptr() if with_perm else None, C.byref(out)))
        self.gpu.sync()
        self.node_length = out.value
        return (out.value, perm[: out.value]) if with_perm else out.value

    def simplify_nodes(self, merge=True, cut_level=None, min_level=None, out_of_place=False, with_perm=False):
        """Simplify the tree in the first node_length words of the node buffer on the GPU (svo_nodes_simplify, DESIGN.md
        26).  merge (lossless): an interior word whose whole subtree holds one leaf value becomes that leaf, so eight equal
        sibling leaves are one again, level after level; every cell samples to what it sampled before.  min_level: no
        merged leaf coarser than that level (the root group's words are level 1, so 3 keeps levels 1 and 2 interior).  cut_level (lossy): every interior word of that
        level becomes a leaf of its subtree's mip colour (the average of the non-empty children per channel, bottom-up),
        a level-of-detail copy when out_of_place.  The result is in compact_nodes' canonical breadth-first layout, the same
        bytes for every layout of the same tree.
        In place: sets node_length to the new length and returns it, the freed tail holds the empty word; raises SvoError,
        with nothing written, for a malformed tree or with a device adaptive state attached.  out_of_place: returns (words,
        length), words a device int32 tensor of the new tree; the node buffer is only read and node_length stays.
        with_perm: perm, a device int32 tensor with perm[new word] = old word, comes last in the result.
        The trap: edit_nodes splits a coarse leaf into EMPTY children, as the reference's put_in_voxel does, so voxels put
        into a merged solid by cell list lose the solid's colour around the edit.  edit_region carries the colour down, and
        min_level bounds how coarse the merge goes."""
        dev = self.gpu.torch_device
        p = SimplifyParams()
        p.flags = (1 if merge else 0) | (2 if cut_level is not None else 0)
        p.cut_level = 0 if cut_level is None else max(0, int(cut_level))
        p.min_level = 0 if min_level is None else max(0, int(min_level))
        p.n_words = int(self.node_length)
        room = max(int(self.node_length), 1)
        words = torch.empty(room, dtype=torch.int32, device=dev) if out_of_place else None
        perm = torch.empty(room, dtype=torch.int32, device=dev) if with_perm else None
        p.out_cap = room if out_of_place else 0
        out = C.c_uint64()
        if out_of_place or with_perm:
            wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_simplify(self.gpu._h, C.byref(p), words.data_ptr() if out_of_place else None,
                                                perm.data_ptr() if with_perm else None, C.byref(out)))
        self.gpu.sync()
        n = out.value
        if not out_of_place:
            self.node_length = n
        res = ((words[:n], n) if out_of_place else (n,)) + ((perm[:n],) if with_perm else ())
        return res if len(res) > 1 else n

    def list_voxels(self, depth=None, expand=False, with_levels=False):
        """The voxels of the tree in the first node_length words of the node buffer, listed on the GPU (svo_nodes_list_voxels,
        DESIGN.md 18): the inverse of build_nodes.  Returns (coords, colours), device tensors (N, 3) int32 and N int32 ready
        for build_nodes, edit_nodes, CpuOctree.build and World.build_world: one entry per coloured leaf, coords its minimum
        corner on the `depth` grid, in ascending Morton order, the same for any layout of the same tree.  expand: a leaf above
        `depth` becomes its cells of the `depth` grid.  with_levels: (coords, colours, levels), the level each leaf was
        found at (`depth` for expanded cells).  depth=None: the depth declared for this tree (16 unless a build, an edit
        or from_world raised it).  Raises SvoError for a tree deeper than `depth`, a malformed tree or 2^31 entries or
        more.  The node buffer is only read."""
        dev = self.gpu.torch_device
        p = ListParams()
        p.flags = 1 if expand else 0
        p.depth = max(0, int(self.gpu.tree_depth if depth is None else depth))
        p.n_words = int(self.node_length)
        n = C.c_uint64()
        self.gpu.check(lib().svo_nodes_list_voxels(self.gpu._h, C.byref(p), None, None, None, C.byref(n)))  # the count
        count = n.value
        coords = torch.empty((count, 3), dtype=torch.int32, device=dev)
        colours = torch.empty(count, dtype=torch.int32, device=dev)
        levels = torch.empty(count, dtype=torch.int32, device=dev) if with_levels else None
        if count:
            p.max_voxels = count
            wait_for_torch(self.gpu)
            self.gpu.check(lib().svo_nodes_list_voxels(self.gpu._h, C.byref(p), coords.data_ptr(), colours.data_ptr(),
                                                       levels.data_ptr() if with_levels else None, C.byref(n)))
            self.gpu.sync()
        return (coords, colours, levels) if with_levels else (coords, colours)

    def _surface(self, flags, depth, with_levels):
        """count query, then fill, of svo_nodes_list_surface: (coords, colours, faces, levels or None)"""
        dev = self.gpu.torch_device
        p = SurfaceParams()
        p.flags = flags
        p.depth = max(0, int(self.gpu.tree_depth if depth is None else depth))
        p.n_words = int(self.node_length)
        n = C.c_uint64()
        self.gpu.check(lib().svo_nodes_list_surface(self.gpu._h, C.byref(p), None, None, None, None, C.byref(n)))  # the count
        count = n.value
        coords = torch.empty((count, 3), dtype=torch.int32, device=dev)
        colours, faces = (torch.empty(count, dtype=torch.int32, device=dev) for _ in range(2))
        levels = torch.empty(count, dtype=torch.int32, device=dev) if with_levels else None
        if count:
            p.max_entries = count
            wait_for_torch(self.gpu)
            self.gpu.check(lib().svo_nodes_list_surface(self.gpu._h, C.byref(p), coords.data_ptr(), colours.data_ptr(),
                                                        levels.data_ptr() if with_levels else None, faces.data_ptr(), C.byref(n)))
            self.gpu.sync()
        return coords, colours, faces, levels

    def list_surface(self, depth=None, closed_boundary=False, keep_hidden=False, with_levels=False):
        """The voxels of the tree that show a face, found on the GPU (svo_nodes_list_surface).  Returns device
        int32 tensors (coords, colours, masks[, levels]): list_voxels' entries, in its order, that have at least one exposed
        face, and per entry the 6-bit mask of its exposed faces (bit f: -x, +x, -y, +y, -z, +z).  A face is covered when a
        leaf of the same or a coarser level stands behind it; empty space, finer detail and the grid's boundary expose it
        (closed_boundary: the boundary covers).  keep_hidden: every entry of list_voxels, masks of 0 included.  depth=None:
        the depth declared for this tree, as in list_voxels.  Raises SvoError as list_voxels does.  The node buffer is
        only read."""
        flags = (1 if closed_boundary else 0) | (2 if keep_hidden else 0)
        coords, colours, masks, levels = self._surface(flags, depth, with_levels)
        return (coords, colours, masks, levels) if with_levels else (coords, colours, masks)

    def surface_quads(self, depth=None, closed_boundary=False):
        """The exposed faces of the tree, one entry each, found on the GPU (svo_nodes_list_surface with SVO_SURFACE_QUADS,
        DESIGN.md 23).  Returns device int32 tensors (coords, colours, faces, levels): the leaf's minimum corner on the
        `depth` grid, its colour, the face's number 0..5 (-x, +x, -y, +y, -z, +z) and the leaf's level, the leaves in
        list_voxels' order and a leaf's faces in ascending number: what mesh.quads_to_mesh takes."""
        return self._surface(4 | (1 if closed_boundary else 0), depth, True)

    def surface_rects(self, depth=None, closed_boundary=False, rounds=1, any_value=False):
        """The exposed faces of the tree merged into rectangles on the GPU (svo_nodes_merge_surface).  Returns
        device int32 tensors (rects (N, 6), values (N)): per rectangle face (0..5, as in surface_quads), plane (its
        coordinate along the face's axis a = face >> 1), u0 and v0 (its minimum corner along the axes (a + 1) % 3 and
        (a + 2) % 3), w and h (its extents along them), all on the `depth` grid, and the value its faces share; ascending
        in (face, plane, u0, w, v0): what mesh.rects_to_mesh takes.  A round joins surface_quads' faces of one plane and
        one value along u, then along v; rounds (1..4) beyond the first matter only in a tree of mixed levels.
        any_value: faces join whatever their values, and every value comes back 0.  depth=None: the depth declared for
        this tree, as in list_voxels.  Raises SvoError as surface_quads does.  The node buffer is only read."""
        dev = self.gpu.torch_device
        p = SurfaceMergeParams()
        p.flags = (1 if closed_boundary else 0) | (8 if any_value else 0)
        p.depth = max(0, int(self.gpu.tree_depth if depth is None else depth))
        p.rounds = max(0, int(rounds))
        p.n_words = int(self.node_length)
        n = C.c_uint64()
        self.gpu.check(lib().svo_nodes_merge_surface(self.gpu._h, C.byref(p), None, None, C.byref(n)))  # the count
        count = n.value
        rects = torch.empty((count, 6), dtype=torch.int32, device=dev)
        values = torch.empty(count, dtype=torch.int32, device=dev)
        if count:
            p.max_entries = count
            wait_for_torch(self.gpu)
            self.gpu.check(lib().svo_nodes_merge_surface(self.gpu._h, C.byref(p), rects.data_ptr(), values.data_ptr(), C.byref(n)))
            self.gpu.sync()
        return rects, values

    def label_components(self, depth=None, same_value=False, with_ids=True, with_indices=False, with_sizes=False):
        """The connected components of the tree's voxels, labelled on the GPU (svo_nodes_label_components).
        The entries are list_voxels' (without expand), in its order; two leaves are linked when their cubes share a piece
        of a face (6-connectivity; a coarse leaf is linked to every finer leaf on its faces), with same_value only when
        their colours are equal.  Returns device tensors (labels, ids, n_components[, indices][, sizes]): labels (N)
        int32, the rank of the first entry of the entry's component (labels[i] <= i); ids (N) int32, the component's number
        0..n_components - 1, numbered by ascending first entry (None without with_ids); indices (N) int32, the index of the
        entry's word in the node buffer, what scatter_nodes_device takes; sizes (n_components) int64, the cells of the
        `depth` grid per component.  The same for every layout of the same tree and on every run, indices excepted.
        depth=None: the depth declared for this tree, as in list_voxels.  Raises SvoError as list_voxels does.  The node
        buffer is only read."""
        dev = self.gpu.torch_device
        p = ComponentsParams()
        p.flags = 1 if same_value else 0
        p.depth = self._depth(depth)
        p.n_words = int(self.node_length)
        n, c = C.c_uint64(), C.c_uint64()
        fn = lib().svo_nodes_label_components
        # the count query is the listing's: the entries are its entries, and it stops before the union
        q = ListParams()
        q.depth, q.n_words = p.depth, p.n_words
        self.gpu.check(lib().svo_nodes_list_voxels(self.gpu._h, C.byref(q), None, None, None, C.byref(n)))
        count = n.value
        want_ids = with_ids or with_sizes
        labels = torch.empty(count, dtype=torch.int32, device=dev)
        ids = torch.empty(count, dtype=torch.int32, device=dev) if want_ids else None
        indices = torch.empty(count, dtype=torch.int32, device=dev) if with_indices else None
        if count:
            p.max_entries = count
            wait_for_torch(self.gpu)
            self.gpu.check(fn(self.gpu._h, C.byref(p), labels.data_ptr(), ids.data_ptr() if want_ids else None,
                              indices.data_ptr() if with_indices else None, C.byref(n), C.byref(c)))
            self.gpu.sync()
        out = (labels, ids if with_ids else None, c.value) + ((indices,) if with_indices else ())
        if with_sizes:
            # integer adds commute: exact, and the same on every run
            levels = self.list_voxels(p.depth, with_levels=True)[2].to(torch.int64)
            sizes = torch.zeros(c.value, dtype=torch.int64, device=dev)
            sizes.index_add_(0, ids.to(torch.int64), torch.ones_like(levels) << (3 * (p.depth - levels)))
            out += (sizes,)
        return out

    def scatter_nodes_device(self, indices, words=None, fill=None):
        """words[i], or the one word `fill`, to the node buffer at indices[i] without leaving the device
        (svo_nodes_scatter_device): indices as sample_voxels(with_indices=True) and label_components(with_indices=True)
        give them, device tensors (or numpy, copied there); an index behind node_length, -1 included, is skipped.  Of
        duplicate indices with different words, which one lands is unspecified.  A later frame waits for the write."""
        if (words is None) == (fill is None):
            raise ValueError("give words or fill, not both")
        dev = self.gpu.torch_device
        idx = device_u32(indices, dev, what="indices").reshape(-1)
        n = idx.numel()
        w = device_u32(words, dev, what="words").reshape(-1) if words is not None else None
        if w is not None and w.numel() != n:
            raise ValueError(f"{w.numel()} words for {n} indices")
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_scatter_device(self.gpu._h, idx.data_ptr() if n else None, w.data_ptr() if w is not None and n else None,
                                                      int(fill or 0) & 0xFFFFFFFF, n, int(self.node_length)))
        self.gpu.sync()  # (the inputs may be released by the caller)

    def drop_floating(self, depth=None, anchor=None, same_value=False):
        """Empty the leaves of every component that is not anchored, on the GPU (label_components, then
        scatter_nodes_device).  anchor: a box (lo, hi) in cells of the `depth` grid, hi exclusive; None: the
        floor layer ((0, 0, 0), (2^depth, 1, 2^depth)), y being up as in column_tops.  A component is anchored when the
        cube of at least one of its leaves meets the box; the leaves of every other component get the empty word.
        Returns (n_components, n_dropped_components, n_dropped_leaves).  The groups this leaves empty stay where they
        are: compact_nodes(prune=True) drops them."""
        depth = self._depth(depth)
        side = 1 << min(depth, 31)
        lo, hi = ((0, 0, 0), (side, 1, side)) if anchor is None else ([int(v) for v in anchor[0]], [int(v) for v in anchor[1]])
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError(f"anchor must be two corners of three cells each, got {anchor!r}")
        _, ids, n_components, indices = self.label_components(depth, same_value, with_indices=True)
        if not n_components:
            return 0, 0, 0
        coords, _, levels = self.list_voxels(depth, with_levels=True)
        dev = self.gpu.torch_device
        first = coords.to(torch.int64)
        last = first + (torch.ones_like(levels, dtype=torch.int64) << (depth - levels.to(torch.int64)))[:, None]
        meets = ((first < torch.tensor(hi, device=dev)) & (last > torch.tensor(lo, device=dev))).all(dim=1)
        held = torch.zeros(n_components, dtype=torch.int64, device=dev).index_add_(0, ids.to(torch.int64), meets.to(torch.int64)) > 0
        drop = ~held[ids.to(torch.int64)]
        n_dropped, n_leaves = int((~held).sum()), int(drop.sum())
        if n_leaves:
            self.scatter_nodes_device(indices[drop], fill=EMPTY_WORD)
        return n_components, n_dropped, n_leaves

    def _sample_params(self, depth):
        p = SampleParams()
        p.depth = max(0, int(self.gpu.tree_depth if depth is None else depth))
        p.n_words = int(self.node_length)
        return p

    def sample_voxels(self, coords, depth=None, with_levels=False, with_indices=False):
        """What the tree in the first node_length words of the node buffer holds at cells of the `depth` grid, looked up on
        the GPU (svo_nodes_sample).  coords as build_nodes takes them, in any order.  Returns an int32 device
        tensor of N values: the leaf's value (its 24-bit colour in built and edited trees, 0 for empty), SAMPLE_FINER where
        the tree is refined below `depth`, SAMPLE_OUTSIDE for a coordinate outside [0, 2^depth) (a negative one included),
        SAMPLE_BROKEN where the path met a bad pointer.  with_levels: also the level the walk stopped on; with_indices: also
        the index of the word it stopped on (as in a hit record; -1 for OUTSIDE); in that order.  depth=None: the depth
        declared for this tree, as in list_voxels.  The node buffer is only read."""
        dev = self.gpu.torch_device
        xyz, _, n, xyz_ptr, _ = voxel_list(self.gpu, coords)
        p = self._sample_params(depth)
        values = torch.empty(n, dtype=torch.int32, device=dev)
        levels = torch.empty(n, dtype=torch.int32, device=dev) if with_levels else None
        indices = torch.empty(n, dtype=torch.int32, device=dev) if with_indices else None
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_sample(self.gpu._h, C.byref(p), xyz_ptr, n, values.data_ptr() if n else None,
                                              levels.data_ptr() if with_levels and n else None,
                                              indices.data_ptr() if with_indices and n else None))
        self.gpu.sync()  # (the inputs may be released by the caller)
        out = (values,) + ((levels,) if with_levels else ()) + ((indices,) if with_indices else ())
        return out if len(out) > 1 else values

    def sample_dense(self, origin, size, depth=None):
        """The cells [origin, origin + size) of the `depth` grid as a dense int32 device tensor of shape `size`, indexed
        [x, y, z] like build_nodes_dense's grid, read from the tree on the GPU (svo_nodes_sample_dense):
        values and marks as sample_voxels gives them.  The whole grid of a dense-built tree comes back as grid & 0xFFFFFF.
        Raises SvoError for a box that leaves the grid or has 2^31 cells or more.  The node buffer is only read."""
        dev = self.gpu.torch_device
        o, s = [int(v) for v in origin], [int(v) for v in size]
        if len(o) != 3 or len(s) != 3 or min(o + s) < 0 or max(o + s) >= 1 << 32:
            raise ValueError(f"origin and size must be 3 values in [0, 2^32) each, got {o} and {s}")
        p = self._sample_params(depth)
        # a box the call will refuse gets no memory first: the library decides and words the refusal
        fits = 1 <= p.depth <= 21 and all(a + b <= 1 << p.depth for a, b in zip(o, s)) and s[0] * s[1] * s[2] < 1 << 31
        grid = torch.empty(s if fits else (0,), dtype=torch.int32, device=dev)
        room = grid if grid.numel() else torch.empty(1, dtype=torch.int32, device=dev)  # (nothing is written to it)
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_sample_dense(self.gpu._h, C.byref(p), (C.c_uint32 * 3)(*o), (C.c_uint32 * 3)(*s), room.data_ptr()))
        self.gpu.sync()
        return grid

    def distance_dense(self, origin, size, max_distance, depth=None, mode="voxels", with_sites=False):
        """The exact squared Euclidean distance of every cell of the box [origin, origin + size) of the `depth` grid to its
        nearest site within max_distance (1..127) cells, computed from the tree on the GPU (svo_nodes_distance, DESIGN.md
        35), as an int32 device tensor of shape `size`, indexed [x, y, z] like sample_dense's.  mode, a name of
        distance.MODES: "voxels" the sites are the occupied cells (every cell that sample_dense gives a value other than
        0), "empty" the empty cells, those outside the grid included, "signed" the voxels for an empty cell and the empty
        cells for an occupied one, which gets the negated value.  distance.FAR (-FAR) where no site is that near.  Sites
        outside the box count.  with_sites: (d2, sites), sites the offset to the nearest site, the lowest (x, y, z) among
        equally near ones, packed as distance.unpack_sites and distance.site_cells take it.  Raises SvoError for a box that
        leaves the grid, has 2^31 cells or more or needs more workspace than the library allows.  The node buffer is
        only read."""
        from .distance import MODES
        dev = self.gpu.torch_device
        o, s = [int(v) for v in origin], [int(v) for v in size]
        if len(o) != 3 or len(s) != 3 or min(o + s) < 0 or max(o + s) >= 1 << 32:
            raise ValueError(f"origin and size must be 3 values in [0, 2^32) each, got {o} and {s}")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {', '.join(MODES)} (got {mode!r})")
        p = DistanceParams()
        p.mode, p.depth, p.n_words = MODES.index(mode), self._depth(depth), int(self.node_length)
        p.max_distance = min(max(0, int(max_distance)), 0xFFFFFFFF)
        # a box the call will refuse gets no memory first: the library decides and words the refusal
        r = p.max_distance
        fits = (1 <= p.depth <= 21 and 1 <= r <= 127 and all(a + b <= 1 << p.depth for a, b in zip(o, s)) and s[0] * s[1] * s[2] < 1 << 31
                and self._distance_workspace(o, s, r, mode == "signed") <= 1 << 30)
        d2 = torch.empty(s if fits else (0,), dtype=torch.int32, device=dev)
        sites = torch.empty(s if fits else (0,), dtype=torch.int32, device=dev) if with_sites else None
        room = d2 if d2.numel() else torch.empty(1, dtype=torch.int32, device=dev)  # (nothing is written to it)
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_distance(self.gpu._h, C.byref(p), (C.c_uint32 * 3)(*o), (C.c_uint32 * 3)(*s), room.data_ptr(),
                                                sites.data_ptr() if with_sites and sites.numel() else None))
        self.gpu.sync()
        return (d2, sites) if with_sites else d2

    @staticmethod
    def _distance_workspace(o, s, r, signed):
        """the bytes of workspace that svo_nodes_distance takes for a box (svo_hip.h's formula)"""
        if not s[0] * s[1] * s[2]:
            return 0
        gx, gy = s[0] + 2 * r, s[1] + 2 * r
        z0 = (o[2] - r) // 64 * 64
        words = (o[2] + s[2] + r - 1 - z0) // 64 + 1
        slab = max(1, min(s[1], (1 << 21) // (gx * s[2])))
        return gx * gy * words * 8 + (2 if signed else 1) * gx * slab * s[2] * 4

    def morph_ball(self, op, radius, origin, size, colour=None, depth=None, max_words=None):
        """Grow or shrink the tree that is in the node buffer by a ball of `radius` (1..127) cells inside the box [origin,
        origin + size) of the `depth` grid, in place and on the device: morph_nodes with a round shape, and
        one pass whatever the radius.  op "grow": every empty cell of the box with a voxel within `radius` (Euclidean,
        voxels outside the box count) becomes a voxel of `colour`; None or 0: the value of its nearest voxel, the lowest
        (x, y, z) among equally near ones.  op "shrink": every occupied cell of the box with an empty cell within `radius`
        is emptied; the grid's outside is empty.  Every other cell of the grid samples exactly as before, the cells of a
        coarse leaf included, which keeps its colour where it is split.
        Made of distance_dense over the box (with the sites for a grow that takes its colours from them), sample_voxels at
        the sites, a dense cube of the changed cells built by build_nodes_dense on a context of its own, and one
        place_nodes of that cube: "under" for a grow, "carve" for a shrink.  The cube covers the changed cells' bounding
        box alone (its corner moved down to a multiple of 8 cells), with the side 2^k >= that box's longest side, and k <= 9: A BOX SIDE ABOVE 512 CELLS IS REFUSED with
        ValueError, as is a radius outside 1..127.  A grow whose colours would
        come from a cell that samples to a mark (SAMPLE_FINER, SAMPLE_BROKEN) raises SvoError before anything is written;
        otherwise raises as distance_dense and place_nodes do, nothing written.  "close" and "open" are two calls with a
        box grown by the radius.  depth=None: the depth declared for this tree.  Returns the new length (node_length);
        equal siblings that a split leaves behind are simplify_nodes' to merge."""
        from .distance import FAR, site_cells
        from .gpu import Gpu
        if op not in ("grow", "shrink"):
            raise ValueError(f"op must be grow or shrink (got {op!r})")
        o, s = [int(v) for v in origin], [int(v) for v in size]
        if len(o) != 3 or len(s) != 3 or min(o + s) < 0:
            raise ValueError(f"origin and size must be 3 values, none negative, got {o} and {s}")
        if max(s) > 512:
            raise ValueError(f"the box's sides must be at most 512 cells: the changed cells are placed as a dense cube (got {s})")
        radius = int(radius)
        if not 1 <= radius <= 127:
            raise ValueError(f"radius must be 1..127 (got {radius})")
        depth = self._depth(depth)
        colour = 0 if colour is None else int(colour) & 0xFFFFFF
        grow = op == "grow"
        from_sites = grow and not colour
        got = self.distance_dense(o, s, radius, depth, "voxels" if grow else "empty", with_sites=from_sites)
        d2 = got[0] if from_sites else got
        changed = (d2 > 0) & (d2 != FAR)
        n = int(changed.sum())
        if not n:
            return int(self.node_length)
        if from_sites:
            cells, _ = site_cells(got[1], o)
            values = self.sample_voxels(cells[changed], depth)
            if int(values.max()) >= SAMPLE_FINER:
                raise SvoError(f"morph_ball: a nearest voxel samples to a mark (SAMPLE_FINER or SAMPLE_BROKEN) at depth {depth}: "
                                   "it has no colour to give")
        at = changed.nonzero()
        lo, hi = at.min(dim=0).values.tolist(), (at.max(dim=0).values + 1).tolist()  # the changed cells' bounding box
        low = [((a + v) & ~7) - a for a, v in zip(o, lo)]  # from a cell of level depth - 3 on: the cube's groups then lie on the scene's
        if max(b - a for a, b in zip(low, hi)) <= 512:
            lo = low
        k = max(1, (max(b - a for a, b in zip(lo, hi)) - 1).bit_length())
        cube = torch.zeros((1 << k,) * 3, dtype=torch.int32, device=self.gpu.torch_device)
        at = at - at.new_tensor(lo)
        cube[at[:, 0], at[:, 1], at[:, 2]] = values if from_sites else (colour if grow else 1)
        words = min(8 * (n * k + 1), (8 << 3 * k) // 7 + 8)
        own = Gpu(self.gpu.device)
        try:
            source = Render(own, (8, 8), np.full(8, EMPTY_WORD, dtype=np.uint32), capacity=max(1024, -(-words // 8) * 8))
            source.build_nodes_dense(cube)
            return self.place_nodes(source, "under" if grow else "carve", depth, offset=[a + b for a, b in zip(o, lo)], src_depth=k,
                                    max_words=max_words)
        finally:
            own.close()

    def _depth(self, depth):
        return max(0, int(self.gpu.tree_depth if depth is None else depth))

    def column_tops(self, origin_xz, size_xz, depth=None, y_range=None, with_values=False):
        """The highest occupied cell of each column of a rectangle of the `depth` grid, found on the GPU (svo_nodes_column_tops,
        DESIGN.md 22): an int32 device tensor of shape size_xz, indexed [x, z], holding the y of the first cell from
        y_range[1] - 1 down to y_range[0] whose sample_voxels value is not 0, or TOP_NONE (-1).  with_values: (tops, values),
        values that cell's value: a colour, SAMPLE_FINER where the tree is refined below `depth` (occupied, and said so),
        SAMPLE_BROKEN, 0 under TOP_NONE.  y_range=None: the whole height; depth=None: the depth declared for this tree.
        Raises SvoError for a rectangle that leaves the grid or a bad y range.  The node buffer is only read."""
        dev = self.gpu.torch_device
        o, s = [int(v) for v in origin_xz], [int(v) for v in size_xz]
        if len(o) != 2 or len(s) != 2 or min(o + s) < 0 or max(o + s) >= 1 << 32:
            raise ValueError(f"origin_xz and size_xz must be 2 values in [0, 2^32) each, got {o} and {s}")
        p = TopsParams()
        p.depth, p.n_words = self._depth(depth), int(self.node_length)
        lo, hi = (0, 1 << min(p.depth, 31)) if y_range is None else (int(v) for v in y_range)
        if min(lo, hi) < 0 or max(lo, hi) >= 1 << 32:
            raise ValueError(f"y_range must be 2 values in [0, 2^32), got {(lo, hi)}")
        p.y_lo, p.y_hi = lo, hi
        # a rectangle the call will refuse gets no memory first: the library decides and words the refusal
        fits = 1 <= p.depth <= 21 and all(a + b <= 1 << p.depth for a, b in zip(o, s)) and s[0] * s[1] < 1 << 31
        tops = torch.empty(s if fits else (0, 0), dtype=torch.int32, device=dev)
        values = torch.empty_like(tops) if with_values else None
        room = tops if tops.numel() else torch.empty(1, dtype=torch.int32, device=dev)  # (nothing is written to it)
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_column_tops(self.gpu._h, C.byref(p), (C.c_uint32 * 2)(*o), (C.c_uint32 * 2)(*s), room.data_ptr(),
                                                   values.data_ptr() if with_values and values.numel() else None))
        self.gpu.sync()
        return (tops, values) if with_values else tops

    def structure_sites(self, tops, values, origin_xz, one_in, seed=0, on_value=0, lift=1, rotate=True):
        """The columns of a rectangle that get a structure, picked on the GPU (svo_structures_sites) from what
        column_tops(origin_xz, tops.shape, ..., with_values=True) returned (values may be None when on_value is 0): the
        column (x, z) is a site when it has a top whose value is a plain value (not FINER, not BROKEN) and, with on_value,
        that value, and when lowbias32(lowbias32(x + seed) ^ z) % one_in == 0.  Returns (origins (N, 3) int32 = (x, top +
        lift, z), rots (N) int32 in 0..3, all 0 without `rotate`), device tensors in the arrays' order, ready for
        stamp_structures."""
        dev = self.gpu.torch_device
        top = device_u32(tops, dev, what="tops")
        val = device_u32(values, dev, what="values") if values is not None else None
        if top.dim() != 2 or (val is not None and val.shape != top.shape):
            raise ValueError(f"tops and values must be (size_x, size_z), got {tuple(top.shape)} and {None if val is None else tuple(val.shape)}")
        o = [int(v) for v in origin_xz]
        if len(o) != 2 or min(o) < 0 or max(o) >= 1 << 32:
            raise ValueError(f"origin_xz must be 2 values in [0, 2^32), got {o}")
        p = SitesParams()
        p.flags, p.seed, p.one_in = 1 if rotate else 0, int(seed) & 0xFFFFFFFF, max(0, int(one_in))
        p.on_value, p.lift = int(on_value) & 0xFFFFFFFF, int(lift)
        args = (top.data_ptr() if top.numel() else None, val.data_ptr() if val is not None and val.numel() else None,
                (C.c_uint32 * 2)(*o), (C.c_uint32 * 2)(*top.shape))
        n = C.c_uint64(top.numel())
        wait_for_torch(self.gpu)
        if n.value > ONE_CALL_ENTRIES:
            self.gpu.check(lib().svo_structures_sites(self.gpu._h, C.byref(p), *args, None, None, C.byref(n)))  # the count
        room = n.value
        origins = torch.empty((room, 3), dtype=torch.int32, device=dev)
        rots = torch.empty(room, dtype=torch.int32, device=dev)
        if room:
            p.max_sites = room
            wait_for_torch(self.gpu)
            self.gpu.check(lib().svo_structures_sites(self.gpu._h, C.byref(p), *args, origins.data_ptr(), rots.data_ptr(), C.byref(n)))
        self.gpu.sync()  # (the inputs may be released by the caller)
        return origins[:n.value], rots[:n.value]

    def stamp_structures(self, structure, origins, depth=None, rots=None, with_placement=False):
        """The voxel list of `structure` (structure.Structure) placed at every origin, made on the GPU (svo_structures_stamp,
        DESIGN.md 22).  origins: (K, 3) integers, the cell the structure's offset (0, 0, 0) lands on, each in [-2^22, 2^22);
        rots: K quarter turns about +y in 0..3 (None: none), turning an offset (dx, dy, dz) into (dz, dy, -dx) each.
        Returns device tensors (coords (N, 3) int32, colours (N) int32[, placements (N) int32]): placement by placement, the
        structure's voxels in their order, those outside the `depth` grid clipped.  The list is what edit_nodes and
        build_nodes take: a later placement wins a shared cell, a colour of 0 removes the cell."""
        dev = self.gpu.torch_device
        offsets, colours = structure.on(dev)
        org = device_u32(origins, dev, what="origins", signed=True)
        if org.dim() != 2 or org.shape[1] != 3:
            raise ValueError(f"origins must be (K, 3), got {tuple(org.shape)}")
        k, m = org.shape[0], offsets.shape[0]
        rot = device_u32(rots, dev, what="rots", clamp=True).reshape(-1) if rots is not None else None
        if rot is not None and rot.numel() != k:
            raise ValueError(f"{rot.numel()} rotations for {k} placements")
        p = StampParams()
        p.depth = self._depth(depth)
        args = (offsets.data_ptr() if m else None, colours.data_ptr() if m else None, m, org.data_ptr() if k else None,
                rot.data_ptr() if rot is not None and k else None, k)
        n = C.c_uint64(k * m)
        wait_for_torch(self.gpu)
        if n.value > ONE_CALL_ENTRIES:
            self.gpu.check(lib().svo_structures_stamp(self.gpu._h, C.byref(p), *args, None, None, None, C.byref(n)))  # the count
        room = n.value
        coords = torch.empty((room, 3), dtype=torch.int32, device=dev)
        out_colours = torch.empty(room, dtype=torch.int32, device=dev)
        placements = torch.empty(room, dtype=torch.int32, device=dev) if with_placement else None
        if room:
            p.max_voxels = room
            wait_for_torch(self.gpu)
            self.gpu.check(lib().svo_structures_stamp(self.gpu._h, C.byref(p), *args, coords.data_ptr(), out_colours.data_ptr(),
                                                      placements.data_ptr() if with_placement else None, C.byref(n)))
        self.gpu.sync()  # (the inputs may be released by the caller)
        out = (coords[:n.value], out_colours[:n.value]) + ((placements[:n.value],) if with_placement else ())
        return out

    def place_structures(self, structure, origins, depth=None, rots=None, max_words=None):
        """stamp_structures, then edit_nodes with the list: the structure put into the tree at every origin, in place.
        Returns the new length (node_length)."""
        depth = self._depth(depth)
        coords, colours = self.stamp_structures(structure, origins, depth, rots)
        return self.edit_nodes(coords, depth, colours, max_words=max_words)

    def scatter_structures(self, structure, origin_xz, size_xz, one_in, seed=0, depth=None, y_range=None, on_value=0, lift=1,
                           rotate=True, max_words=None):
        """A structure scattered over the ground of a rectangle without the tree leaving the device: column_tops, then
        structure_sites, then place_structures.  Returns the sites (origins, rots) and leaves node_length as edit_nodes
        does."""
        depth = self._depth(depth)
        tops, values = self.column_tops(origin_xz, size_xz, depth, y_range, with_values=True)
        origins, rots = self.structure_sites(tops, values, origin_xz, one_in, seed, on_value, lift, rotate)
        self.place_structures(structure, origins, depth, rots, max_words)
        return origins, rots

    def build_nodes_dense(self, grid, max_words=None):
        """Build the tree of a dense (side, side, side) colour grid indexed [x, y, z] (non-zero = voxel, low 24 bits the
        colour; side = 2^depth, depth 1..10) on the GPU (svo_nodes_build_dense).  Returns the word count."""
        g = device_u32(grid, self.gpu.torch_device, cells=True)
        side = g.shape[0] if g.dim() == 3 else 0
        depth = side.bit_length() - 1
        if g.dim() != 3 or tuple(g.shape) != (side,) * 3 or side != 1 << depth:
            raise ValueError(f"grid must be (side, side, side) with side a power of two, got {tuple(g.shape)}")
        p = self._build_params(depth, 0, max_words)
        out = C.c_uint64()
        wait_for_torch(self.gpu)
        self.gpu.check(lib().svo_nodes_build_dense(self.gpu._h, g.data_ptr(), C.byref(p), C.byref(out)))
        self.gpu.sync()
        self.node_length = out.value
        return out.value

    def _build_params(self, depth, colour, max_words):
        depth = int(depth)
        self.gpu.declare_depth(depth)
        p = BuildParams()
        p.depth = max(0, depth)
        p.default_colour = int(colour) & 0xFFFFFF
        p.max_words = int(max_words or 0)
        return p

    def scatter_nodes(self, indices, words, node_length=None):
        """Incremental upload: words[i] -> node buffer [indices[i]] (svo_nodes_scatter)."""
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        self.gpu.check(lib().svo_nodes_scatter(self.gpu._h, indices.ctypes.data, words.ctypes.data, indices.size))
        self.gpu.sync()  # the host arrays may be released by the caller
        if indices.size:
            self.node_length = max(self.node_length, int(indices.max()) + 1)
        if node_length is not None:
            self.node_length = max(self.node_length, node_length)

    def read_nodes(self, n=None, offset=0):
        n = self.node_length if n is None else n
        out = np.empty(n, dtype=np.uint32)
        self.gpu.check(lib().svo_nodes_read(self.gpu._h, offset, out.ctypes.data, n))
        return out

    def resize(self, new_size):
        if new_size[0] > 0 and new_size[1] > 0:  # render.rs:183
            self.size = (int(new_size[0]), int(new_size[1]))

    def set_flags(self, pause_adaptive=None, show_steps=None, show_hits=None, shadows=None, misc_bool=None):
        f = self.uniforms.flags
        for bit, v in ((F_PAUSE_ADAPTIVE, pause_adaptive), (F_SHOW_STEPS, show_steps), (F_SHOW_HITS, show_hits),
                       (F_SHADOWS, shadows), (F_MISC_BOOL, misc_bool)):
            if v is not None:
                f = (f | bit) if v else (f & ~bit)
        self.uniforms.flags = f

    def update(self, settings, character):
        """render.rs:191-215: camera = proj * look_at_rh; upload the uniforms."""
        w, h = self.size
        # Settings.octree_depth (app.rs:24) is the depth the adaptive loop refines to: a tree may reach it, so it is declared to the
        # library when it exceeds what the context holds (a deeper scene used to fail only at svo_sync); any depth,
        # the library words the refusal of one the option does not take
        depth = int(getattr(settings, "octree_depth", 0) or 0)
        self.gpu.declare_depth(depth, most=depth)
        cam, inv = camera_matrices(character.pos, character.look, settings.fov, w, h)
        self.uniforms.camera[:] = cam.tolist()
        self.uniforms.camera_inverse[:] = inv.tolist()
        self.uniforms.dimensions[:] = [float(w), float(h), 0.0, 0.0]
        self.upload_uniforms()

    def upload_uniforms(self):
        self.gpu.check(lib().svo_set_uniforms(self.gpu._h, C.byref(self.uniforms)))

    def alloc_hits(self, n_pixels, device=None):
        dev = device if device is not None else f"cuda:{self.gpu.device}"
        return torch.empty((n_pixels, 4), dtype=torch.int32, device=dev)

    def _rect(self, tile):
        """(frame w, h, x0, y0, w, h) of `tile`; None: the whole frame"""
        return self.size + (tuple(tile) if tile is not None else (0, 0) + self.size)

    def render(self, hits=None, tile=None, rgba=None):
        """Trace every pixel of the frame (or of tile=(x0, y0, w, h)); asynchronous.  Returns the
        device tensor of hit records (n_pixels x 4 int32 = svo_hit)."""
        w, h, x0, y0, tw, th = self._rect(tile)
        if hits is None:
            hits = self.alloc_hits(tw * th)
        self.gpu.check(lib().svo_render(self.gpu._h, w, h, x0, y0, tw, th, hits.data_ptr(),
                                        rgba.data_ptr() if rgba is not None else None))
        return hits

    def render_tiles(self, tile_w, tile_h, first_tile, tile_stride, hits=None, rgba=None):
        """This rank's tiles (first_tile, first_tile + tile_stride, ...), contiguous in that order."""
        w, h = self.size
        n_mine = sharding.local_tile_count(w, h, tile_w, tile_h, first_tile, tile_stride)
        if hits is None:
            hits = self.alloc_hits(n_mine * tile_w * tile_h)
        self.gpu.check(lib().svo_render_tiles(self.gpu._h, w, h, tile_w, tile_h, first_tile, tile_stride,
                                              hits.data_ptr(), rgba.data_ptr() if rgba is not None else None))
        return hits

    def render_secondary(self, n_secondary, tile=None, hits=None, secondary=None):
        """Primary rays plus n_secondary rays per hit pixel (svo_render_secondary): returns (primary records,
        secondary records [n_secondary * n_pixels, ray-major]) as device tensors; asynchronous."""
        w, h, x0, y0, tw, th = self._rect(tile)
        if hits is None:
            hits = self.alloc_hits(tw * th)
        if secondary is None:
            secondary = self.alloc_hits(n_secondary * tw * th)
        self.gpu.check(lib().svo_render_secondary(self.gpu._h, w, h, x0, y0, tw, th, n_secondary, hits.data_ptr(),
                                                  secondary.data_ptr()))
        return hits, secondary

    def render_tiles_secondary(self, tile_w, tile_h, first_tile, tile_stride, n_secondary, hits=None, secondary=None):
        """render_tiles with secondary rays: this rank's tiles, contiguous; secondary ray-major over them."""
        w, h = self.size
        n_mine = sharding.local_tile_count(w, h, tile_w, tile_h, first_tile, tile_stride)
        if hits is None:
            hits = self.alloc_hits(n_mine * tile_w * tile_h)
        if secondary is None:
            secondary = self.alloc_hits(n_secondary * n_mine * tile_w * tile_h)
        self.gpu.check(lib().svo_render_tiles_secondary(self.gpu._h, w, h, tile_w, tile_h, first_tile, tile_stride,
                                                        n_secondary, hits.data_ptr(), secondary.data_ptr()))
        return hits, secondary

    def assemble_tiles(self, gathered, tile_w, tile_h, out=None):
        """Rank 0: un-permute a gathered frame ([world, n_pad, tile_h * tile_w, 4] int32, device; last dimension 3 for wire
        records) into the row-major frame
        ([H, W, 4]) with one kernel on this context's stream (svo_assemble_tiles)."""
        w, h = self.size
        world, n_pad = int(gathered.shape[0]), int(gathered.shape[1])
        if out is None:
            out = torch.empty((h, w, 4), dtype=torch.int32, device=gathered.device)
        fn = lib().svo_assemble_tiles_packed if gathered.shape[-1] == 3 else lib().svo_assemble_tiles
        self.gpu.check(fn(self.gpu._h, gathered.data_ptr(), world, n_pad, w, h, tile_w, tile_h, out.data_ptr()))
        return out

    def assemble_tiles_rgba(self, gathered, tile_w, tile_h, out=None):
        """Rank 0: un-permute a gathered COLOUR frame ([world, n_pad, tile_h * tile_w] int32 RGBA8, device) into [H, W]
        (svo_assemble_tiles_rgba)."""
        w, h = self.size
        world, n_pad = int(gathered.shape[0]), int(gathered.shape[1])
        if out is None:
            out = torch.empty((h, w), dtype=torch.int32, device=gathered.device)
        self.gpu.check(lib().svo_assemble_tiles_rgba(self.gpu._h, gathered.data_ptr(), world, n_pad, w, h, tile_w, tile_h, out.data_ptr()))
        return out

    def pack_records(self, records, wire):
        """[..., 4] int32 hit records -> [..., 3] int32 wire records (svo_pack_records), on this context's stream."""
        n = records.numel() // 4
        self.gpu.check(lib().svo_pack_records(self.gpu._h, records.data_ptr(), n, wire.data_ptr()))
        return wire

    def render_host(self, tile=None, rgba=False):
        """Blocking variant with host results: hit records (numpy structured array, tile-local row-major)
        and, with rgba=True, also the shaded RGBA8 image of fs_main (uint8 [h, w, 4])."""
        w, h, x0, y0, tw, th = self._rect(tile)
        out = np.empty((th, tw), dtype=HIT_DTYPE)
        img = np.empty((th, tw), dtype=np.uint32) if rgba else None
        self.gpu.check(lib().svo_render_host(self.gpu._h, w, h, x0, y0, tw, th, out.ctypes.data,
                                             img.ctypes.data if rgba else None))
        return (out, img.view(np.uint8).reshape(th, tw, 4)) if rgba else out

    def alloc_rgba(self, n_pixels, device=None):
        dev = device if device is not None else f"cuda:{self.gpu.device}"
        return torch.empty((n_pixels,), dtype=torch.int32, device=dev)

    def trace_rays(self, rays, hits=None):
        """octree_ray over explicit rays (device float32 tensor n x 6)."""
        n = rays.shape[0]
        if hits is None:
            hits = self.alloc_hits(n, rays.device)
        self.gpu.check(lib().svo_trace_rays(self.gpu._h, rays.data_ptr(), n, hits.data_ptr()))
        return hits


def hits_to_numpy(hits):
    """device hit tensor -> numpy structured array (value, t, info, normal_bits)"""
    return hits.cpu().numpy().view(np.uint32).reshape(-1, 4).copy().view(HIT_DTYPE).reshape(-1)
