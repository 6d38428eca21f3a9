"""ctypes loader for libsvo_hip.so (the C-ABI drop-in, include/svo_hip.h + include/svo_host.h).

There is no CPU fallback: if the library is missing this module raises, and every device
call goes through the HIP kernels in csrc/.
"""
import ctypes as C
import os

# torch first: it ships its own libamdhip64.so.7; loading it before our library makes both share
# one HIP runtime (same SONAME), so torch tensors/streams and our kernels live in one context.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVO_HIP_LIB") or os.path.join(_HERE, "libsvo_hip.so")  # override: A/B builds in experiments


class Uniforms(C.Structure):
    """svo_uniforms: the reference's Uniforms (render.rs:287-322) with explicit u32 flags."""
    _fields_ = [
        ("camera", C.c_float * 16),
        ("camera_inverse", C.c_float * 16),
        ("dimensions", C.c_float * 4),
        ("sun_dir", C.c_float * 4),
        ("flags", C.c_uint32),
        ("misc_value", C.c_float),
    ]


class TerrainParams(C.Structure):
    _fields_ = [
        ("seed", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("cam", C.c_float * 3),
        ("lod_c", C.c_float),
        ("min_depth", C.c_uint32),
        ("max_words", C.c_uint64),
    ]


class ProcParams(C.Structure):
    """svo_proc_params: one procedural chunk (include/svo_hip.h)."""
    _fields_ = [
        ("pos", C.c_float * 3),
        ("base_depth", C.c_uint32),
        ("chunk_depth", C.c_uint32),
        ("max_nodes", C.c_uint64),
    ]


class BuildParams(C.Structure):
    """svo_build_params: a tree built on the GPU (include/svo_hip.h)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("default_colour", C.c_uint32),
        ("max_words", C.c_uint64),
    ]


class EditParams(C.Structure):
    """svo_edit_params: voxels put into a tree that is in the node buffer (include/svo_hip.h)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("default_colour", C.c_uint32),
        ("n_words", C.c_uint64),
        ("max_words", C.c_uint64),
    ]


class RegionShape(C.Structure):
    """svo_region_shape: one box or ball of a shape edit, 32 bytes (include/svo_hip.h)."""
    _fields_ = [
        ("kind", C.c_uint16),
        ("mode", C.c_uint16),
        ("colour", C.c_uint32),
        ("a", C.c_uint32 * 3),
        ("b", C.c_uint32 * 3),
    ]


class RegionParams(C.Structure):
    """svo_region_params: the tree in the node buffer edited by shapes (include/svo_hip.h)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n_words", C.c_uint64),
        ("max_words", C.c_uint64),
    ]


class CombineParams(C.Structure):
    """svo_combine_params: the tree in the node buffer combined with a second tree (include/svo_hip.h)."""
    _fields_ = [
        ("op", C.c_uint32),
        ("depth", C.c_uint32),
        ("at_level", C.c_uint32),
        ("at", C.c_uint32 * 3),
        ("n_words", C.c_uint64),
        ("src_words", C.c_uint64),
        ("max_words", C.c_uint64),
    ]


class PlaceParams(C.Structure):
    """svo_place_params: a second tree placed into the tree in the node buffer at a cell offset and orientation (include/svo_hip.h)."""
    _fields_ = [
        ("op", C.c_uint32),
        ("depth", C.c_uint32),
        ("src_depth", C.c_uint32),
        ("orient", C.c_uint32),
        ("offset", C.c_int32 * 3),
        ("reserved", C.c_uint32),
        ("n_words", C.c_uint64),
        ("src_words", C.c_uint64),
        ("max_words", C.c_uint64),
    ]


class TransformParams(C.Structure):
    """svo_transform_params: a second tree placed into the tree in the node buffer under an affine map (include/svo_hip.h)."""
    _fields_ = [
        ("op", C.c_uint32),
        ("depth", C.c_uint32),
        ("src_depth", C.c_uint32),
        ("matrix", C.c_int32 * 9),
        ("translate", C.c_int64 * 3),
        ("n_words", C.c_uint64),
        ("src_words", C.c_uint64),
        ("max_words", C.c_uint64),
    ]


class MorphParams(C.Structure):
    """svo_morph_params: one step of morphology on the tree in the node buffer (include/svo_hip.h)."""
    _fields_ = [
        ("op", C.c_uint32),
        ("conn", C.c_uint32),
        ("depth", C.c_uint32),
        ("flags", C.c_uint32),
        ("colour", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n_words", C.c_uint64),
        ("max_words", C.c_uint64),
    ]


class HeightmapLayer(C.Structure):
    """svo_heightmap_layer: one band of ground below a height map's surface (include/svo_hip.h)."""
    _fields_ = [
        ("thickness", C.c_uint32),
        ("colour", C.c_uint32),
    ]


class HeightmapParams(C.Structure):
    """svo_heightmap_params: the tree in the node buffer shaped by a height map (include/svo_hip.h)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("n_layers", C.c_uint32),
        ("n_words", C.c_uint64),
        ("max_words", C.c_uint64),
        ("origin_xz", C.c_uint32 * 2),
        ("size_xz", C.c_uint32 * 2),
        ("mode_below", C.c_uint32),
        ("mode_above", C.c_uint32),
        ("colour_above", C.c_uint32),
        ("reserved", C.c_uint32),
        ("layers", HeightmapLayer * 8),
    ]


class CompactParams(C.Structure):
    """svo_compact_params: the tree in the node buffer compacted in place (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n_words", C.c_uint64),
    ]


class SimplifyParams(C.Structure):
    """svo_simplify_params: the tree in the node buffer simplified, in place or into a copy (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("cut_level", C.c_uint32),
        ("min_level", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n_words", C.c_uint64),
        ("out_cap", C.c_uint64),
    ]


class ListParams(C.Structure):
    """svo_list_params: the voxels of the tree in the node buffer listed on the device (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("depth", C.c_uint32),
        ("n_words", C.c_uint64),
        ("max_voxels", C.c_uint64),
    ]


class SurfaceParams(C.Structure):
    """svo_surface_params: the visible surface of the tree in the node buffer (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("depth", C.c_uint32),
        ("n_words", C.c_uint64),
        ("max_entries", C.c_uint64),
    ]


class SurfaceMergeParams(C.Structure):
    """svo_surface_merge_params: the visible surface merged into rectangles (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("depth", C.c_uint32),
        ("rounds", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n_words", C.c_uint64),
        ("max_entries", C.c_uint64),
    ]


class ComponentsParams(C.Structure):
    """svo_components_params: the connected components of the tree in the node buffer (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("depth", C.c_uint32),
        ("n_words", C.c_uint64),
        ("max_entries", C.c_uint64),
    ]


class SampleParams(C.Structure):
    """svo_sample_params: the tree in the node buffer sampled on the device (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("depth", C.c_uint32),
        ("n_words", C.c_uint64),
    ]


class DistanceParams(C.Structure):
    """svo_distance_params: the exact distance field of the tree in the node buffer (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("mode", C.c_uint32),
        ("depth", C.c_uint32),
        ("max_distance", C.c_uint32),
        ("n_words", C.c_uint64),
    ]


class VoxelizeParams(C.Structure):
    """svo_voxelize_params: a triangle mesh voxelised on the device (include/svo_hip.h)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("flags", C.c_uint32),
        ("default_colour", C.c_uint32),
        ("n_vertices", C.c_uint32),
        ("max_voxels", C.c_uint64),
    ]


class SolidParams(C.Structure):
    """svo_solid_params: a closed triangle mesh voxelised solid on the device (include/svo_hip.h)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("flags", C.c_uint32),
        ("n_vertices", C.c_uint32),
        ("reserved", C.c_uint32),
        ("max_out", C.c_uint64),
        ("max_pairs", C.c_uint64),
    ]


class TopsParams(C.Structure):
    """svo_tops_params: the highest occupied cell of each column of the tree in the node buffer (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("depth", C.c_uint32),
        ("n_words", C.c_uint64),
        ("y_lo", C.c_uint32),
        ("y_hi", C.c_uint32),
    ]


class SitesParams(C.Structure):
    """svo_sites_params: the columns that get a structure (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("seed", C.c_uint32),
        ("one_in", C.c_uint32),
        ("on_value", C.c_uint32),
        ("lift", C.c_int32),
        ("reserved", C.c_uint32),
        ("max_sites", C.c_uint64),
    ]


class StampParams(C.Structure):
    """svo_stamp_params: placements x structure -> a voxel list (include/svo_hip.h)."""
    _fields_ = [
        ("flags", C.c_uint32),
        ("depth", C.c_uint32),
        ("max_voxels", C.c_uint64),
    ]


class ChunkBuildParams(C.Structure):
    """svo_chunk_build_params: a mip-coloured tree or a chunked world built on the GPU (include/svo_hip.h)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("world_depth", C.c_uint32),
        ("default_colour", C.c_uint32),
        ("max_nodes", C.c_uint64),
    ]


class AdaptiveResult(C.Structure):
    """svo_adaptive_result: one device adaptive step (include/svo_hip.h)."""
    _fields_ = [
        ("n_sub", C.c_uint32),
        ("n_unsub", C.c_uint32),
        ("chunks_loaded", C.c_uint64),
        ("length", C.c_uint64),
        ("n_removed", C.c_uint32),
        ("removed", C.POINTER(C.c_uint32)),
    ]


vp, sz, u32, u64, i64, f32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int64, C.c_float
cp = C.c_char_p
fp = C.POINTER(C.c_float)

# the device boundary (include/svo_hip.h): name -> (result, argument types)
DEVICE_SIGNATURES = {
    "svo_device_count": (C.c_int, ()),
    "svo_buffer_alloc": (C.c_int, (vp, sz, C.POINTER(vp))),
    "svo_buffer_free": (C.c_int, (vp, vp)),
    "svo_buffer_read": (C.c_int, (vp, vp, vp, sz)),
    "svo_ctx_create": (C.c_int, (C.c_int, C.POINTER(vp))),
    "svo_ctx_destroy": (C.c_int, (vp,)),
    "svo_ctx_set_stream": (C.c_int, (vp, vp, C.c_int)),
    "svo_set_option": (C.c_int, (vp, C.c_int, i64)),
    "svo_last_error": (cp, (vp,)),
    "svo_sync": (C.c_int, (vp,)),
    "svo_nodes_alloc": (C.c_int, (vp, sz)),
    "svo_nodes_bind_device": (C.c_int, (vp, vp, sz)),
    "svo_nodes_write": (C.c_int, (vp, sz, vp, sz)),
    "svo_nodes_scatter": (C.c_int, (vp, vp, vp, sz)),
    "svo_nodes_read": (C.c_int, (vp, sz, vp, sz)),
    "svo_nodes_device_ptr": (C.c_int, (vp, C.POINTER(vp), C.POINTER(sz))),
    "svo_nodes_share": (C.c_int, (vp, vp)),
    "svo_nodes_invalidate": (C.c_int, (vp,)),
    "svo_comm_unique_id": (C.c_int, (vp,)),
    "svo_comm_init_rank": (C.c_int, (vp, vp, C.c_int, C.c_int)),
    "svo_comm_init_all": (C.c_int, (C.c_int, C.POINTER(vp))),
    "svo_comm_destroy": (C.c_int, (vp,)),
    "svo_gather_frame": (C.c_int, (vp, vp, sz, vp, C.c_int)),
    "svo_gather_wait": (C.c_int, (vp,)),
    "svo_gather_frame_all": (C.c_int, (C.c_int, C.POINTER(vp), C.POINTER(vp), sz, vp, C.c_int)),
    "svo_set_uniforms": (C.c_int, (vp, C.POINTER(Uniforms))),
    "svo_render": (C.c_int, (vp, u32, u32, u32, u32, u32, u32, vp, vp)),
    "svo_render_host": (C.c_int, (vp, u32, u32, u32, u32, u32, u32, vp, vp)),
    "svo_render_tiles": (C.c_int, (vp, u32, u32, u32, u32, u32, u32, vp, vp)),
    "svo_render_secondary": (C.c_int, (vp, u32, u32, u32, u32, u32, u32, u32, vp, vp)),
    "svo_render_tiles_secondary": (C.c_int, (vp, u32, u32, u32, u32, u32, u32, u32, vp, vp)),
    "svo_assemble_tiles": (C.c_int, (vp, vp, u32, u32, u32, u32, u32, u32, vp)),
    "svo_assemble_tiles_packed": (C.c_int, (vp, vp, u32, u32, u32, u32, u32, u32, vp)),
    "svo_assemble_tiles_rgba": (C.c_int, (vp, vp, u32, u32, u32, u32, u32, u32, vp)),
    "svo_pack_records": (C.c_int, (vp, vp, sz, vp)),
    "svo_trace_rays": (C.c_int, (vp, vp, sz, vp)),
    "svo_last_render_ms": (C.c_int, (vp, fp)),
    "svo_timing_collect": (C.c_int, (vp, fp, sz, C.POINTER(sz))),
    "svo_diag_gather": (C.c_int, (vp, u32, u32)),
    "svo_diag_strip_classes": (C.c_int, (vp, vp, sz)),
    "svo_diag_deal": (C.c_int, (vp, vp, vp, sz, vp, sz)),
    "svo_diag_schedule": (C.c_int, (vp, C.c_int, vp, vp, sz, vp, vp, sz, vp)),
    "svo_scan_dispatch": (C.c_int, (vp, u32)),
    "svo_scan_read": (C.c_int, (vp, vp, C.POINTER(u32), vp, C.POINTER(u32), sz)),
    "svo_proc_generate_chunk": (C.c_int, (vp, C.POINTER(ProcParams), C.POINTER(vp))),
    "svo_world_generate": (C.c_int, (vp, vp, u32, u32)),
    "svo_proc_sdf": (C.c_int, (vp, vp, sz, vp)),
    "svo_proc_classify": (C.c_int, (vp, C.POINTER(ProcParams), vp)),
    "svo_proc_timing": (C.c_int, (vp, fp)),
    "svo_nodes_build": (C.c_int, (vp, vp, vp, sz, C.POINTER(BuildParams), C.POINTER(u64))),
    "svo_nodes_build_dense": (C.c_int, (vp, vp, C.POINTER(BuildParams), C.POINTER(u64))),
    "svo_buffer_write": (C.c_int, (vp, vp, vp, sz)),
    "svo_build_timing": (C.c_int, (vp, fp)),
    "svo_cpu_octree_build": (C.c_int, (vp, vp, vp, sz, C.POINTER(ChunkBuildParams), C.POINTER(vp))),
    "svo_world_build": (C.c_int, (vp, vp, vp, vp, sz, C.POINTER(ChunkBuildParams))),
    "svo_world_build_timing": (C.c_int, (vp, fp)),
    "svo_nodes_edit": (C.c_int, (vp, vp, vp, sz, C.POINTER(EditParams), C.POINTER(u64))),
    "svo_edit_timing": (C.c_int, (vp, fp)),
    "svo_nodes_edit_region": (C.c_int, (vp, C.POINTER(RegionShape), sz, C.POINTER(RegionParams), C.POINTER(u64))),
    "svo_region_timing": (C.c_int, (vp, fp)),
    "svo_nodes_combine": (C.c_int, (vp, vp, C.POINTER(CombineParams), C.POINTER(u64))),
    "svo_combine_timing": (C.c_int, (vp, fp)),
    "svo_nodes_place": (C.c_int, (vp, vp, C.POINTER(PlaceParams), C.POINTER(u64))),
    "svo_place_timing": (C.c_int, (vp, fp)),
    "svo_nodes_transform": (C.c_int, (vp, vp, C.POINTER(TransformParams), C.POINTER(u64))),
    "svo_transform_timing": (C.c_int, (vp, fp)),
    "svo_nodes_morph": (C.c_int, (vp, C.POINTER(MorphParams), C.POINTER(u64))),
    "svo_morph_timing": (C.c_int, (vp, fp)),
    "svo_nodes_edit_heightmap": (C.c_int, (vp, C.POINTER(HeightmapParams), vp, C.POINTER(u64))),
    "svo_heightmap_minmax": (C.c_int, (vp, C.POINTER(HeightmapParams), vp, u32, vp)),
    "svo_heightmap_timing": (C.c_int, (vp, fp)),
    "svo_nodes_compact": (C.c_int, (vp, C.POINTER(CompactParams), vp, C.POINTER(u64))),
    "svo_compact_timing": (C.c_int, (vp, fp)),
    "svo_nodes_simplify": (C.c_int, (vp, C.POINTER(SimplifyParams), vp, vp, C.POINTER(u64))),
    "svo_simplify_timing": (C.c_int, (vp, fp)),
    "svo_nodes_list_voxels": (C.c_int, (vp, C.POINTER(ListParams), vp, vp, vp, C.POINTER(u64))),
    "svo_list_timing": (C.c_int, (vp, fp)),
    "svo_nodes_list_surface": (C.c_int, (vp, C.POINTER(SurfaceParams), vp, vp, vp, vp, C.POINTER(u64))),
    "svo_surface_timing": (C.c_int, (vp, fp)),
    "svo_nodes_merge_surface": (C.c_int, (vp, C.POINTER(SurfaceMergeParams), vp, vp, C.POINTER(u64))),
    "svo_surface_merge_timing": (C.c_int, (vp, fp)),
    "svo_nodes_label_components": (C.c_int, (vp, C.POINTER(ComponentsParams), vp, vp, vp, C.POINTER(u64), C.POINTER(u64))),
    "svo_components_timing": (C.c_int, (vp, fp, C.POINTER(u32))),
    "svo_nodes_scatter_device": (C.c_int, (vp, vp, vp, u32, sz, u64)),
    "svo_nodes_sample": (C.c_int, (vp, C.POINTER(SampleParams), vp, sz, vp, vp, vp)),
    "svo_nodes_sample_dense": (C.c_int, (vp, C.POINTER(SampleParams), C.POINTER(u32), C.POINTER(u32), vp)),
    "svo_sample_timing": (C.c_int, (vp, fp)),
    "svo_nodes_distance": (C.c_int, (vp, C.POINTER(DistanceParams), C.POINTER(u32), C.POINTER(u32), vp, vp)),
    "svo_distance_timing": (C.c_int, (vp, fp)),
    "svo_mesh_voxelize": (C.c_int, (vp, C.POINTER(VoxelizeParams), vp, vp, vp, sz, vp, vp, vp, C.POINTER(u64))),
    "svo_voxelize_timing": (C.c_int, (vp, fp)),
    "svo_mesh_voxelize_solid": (C.c_int, (vp, C.POINTER(SolidParams), vp, vp, sz, vp, C.POINTER(u64), C.POINTER(u64))),
    "svo_solid_timing": (C.c_int, (vp, fp)),
    "svo_nodes_column_tops": (C.c_int, (vp, C.POINTER(TopsParams), C.POINTER(u32), C.POINTER(u32), vp, vp)),
    "svo_structures_sites": (C.c_int, (vp, C.POINTER(SitesParams), vp, vp, C.POINTER(u32), C.POINTER(u32), vp, vp, C.POINTER(u64))),
    "svo_structures_stamp": (C.c_int, (vp, C.POINTER(StampParams), vp, vp, sz, vp, vp, sz, vp, vp, vp, C.POINTER(u64))),
    "svo_structure_timing": (C.c_int, (vp, fp)),
    "svo_adaptive_attach": (C.c_int, (vp, vp, vp)),
    "svo_adaptive_step": (C.c_int, (vp, vp, u32, vp, u32, C.POINTER(AdaptiveResult))),
    "svo_adaptive_download": (C.c_int, (vp, vp)),
    "svo_adaptive_length": (C.c_int, (vp, C.POINTER(u64))),
    "svo_adaptive_timing": (C.c_int, (vp, fp)),
    "svo_adaptive_expand": (C.c_int, (vp, u32, fp, f32, u64, C.POINTER(AdaptiveResult))),
    "svo_adaptive_expand_timing": (C.c_int, (vp, fp)),
}
# the host data model (include/svo_host.h): name -> (result, argument types)
HOST_SIGNATURES = {
    "svo_cpu_octree_new": (vp, (C.c_uint8,)),
    "svo_cpu_octree_free": (None, (vp,)),
    "svo_cpu_octree_len": (sz, (vp,)),
    "svo_cpu_octree_load_file": (vp, (cp, u32, cp, sz)),
    "svo_cpu_octree_load_vox": (vp, (cp, sz, cp, sz)),
    "svo_cpu_octree_load_rsvo": (vp, (cp, sz, u32, cp, sz)),
    "svo_cpu_octree_from_voxels": (vp, (u32, vp, sz, vp, cp, sz)),
    "svo_cpu_octree_put_in_voxel": (None, (vp, fp, C.POINTER(C.c_uint8), u32)),
    "svo_cpu_octree_put_in_block": (None, (vp, fp, u32, u32)),
    "svo_cpu_octree_find_voxel": (None, (vp, fp, i64, C.POINTER(u64), C.POINTER(u32), fp)),
    "svo_cpu_octree_get_node_mask": (None, (vp, sz, C.POINTER(C.c_uint8))),
    "svo_cpu_octree_to_octree": (None, (vp, vp)),
    "svo_cpu_octree_raw": (None, (vp, vp, vp)),
    "svo_cpu_octree_generate_mips": (None, (vp, C.POINTER(C.c_uint8))),
    "svo_vox_parse": (i64, (cp, sz, C.POINTER(u32), vp, sz, vp, cp, sz)),
    "svo_vox_write": (sz, (u32, vp, sz, vp, vp, sz)),
    "svo_vox_write_box": (sz, (C.POINTER(u32), vp, sz, vp, vp, sz)),
    "svo_structure_load": (i64, (cp, cp, sz, vp, vp, vp, sz, cp, sz)),
    "svo_rsvo_write": (sz, (vp, vp, sz)),
    "svo_octree_new": (vp, (C.POINTER(C.c_uint8),)),
    "svo_octree_from_words": (vp, (vp, sz)),
    "svo_octree_free": (None, (vp,)),
    "svo_octree_len": (sz, (vp,)),
    "svo_octree_raw_data": (vp, (vp,)),
    "svo_octree_get_node": (u32, (vp, sz)),
    "svo_octree_subdivide": (C.c_int, (vp, sz, C.POINTER(C.c_uint8), u32)),
    "svo_octree_unsubdivide": (C.c_int, (vp, sz)),
    "svo_octree_find_voxel": (None, (vp, fp, i64, C.POINTER(u64), C.POINTER(u32), fp)),
    "svo_octree_expanded": (C.c_int, (vp, sz, vp)),
    "svo_octree_pos_offset": (None, (u32, u32, fp)),
    "svo_octree_holes": (sz, (vp,)),
    "svo_octree_set_node": (None, (vp, sz, u32)),
    "svo_octree_position": (None, (vp, sz, fp)),
    "svo_octree_hole_stack": (sz, (vp, vp, sz)),
    "svo_octree_positions": (sz, (vp, vp, sz)),
    "svo_octree_take_dirty": (sz, (vp, vp, vp, sz)),
    "svo_world_new": (vp, (cp,)),
    "svo_world_free": (None, (vp,)),
    "svo_world_last_error": (cp, (vp,)),
    "svo_world_insert": (C.c_int, (vp, u32, vp)),
    "svo_world_remove": (C.c_int, (vp, u32)),
    "svo_world_chunk": (vp, (vp, u32)),
    "svo_world_chunk_ids": (sz, (vp, vp, sz)),
    "svo_world_find_voxel": (C.c_int, (vp, fp, i64, C.POINTER(u32), C.POINTER(u64), C.POINTER(u32), fp)),
    "svo_world_generate_mip_tree": (C.c_int, (vp, u32, C.POINTER(C.c_uint8))),
    "svo_world_save_chunk": (C.c_int, (vp, u32)),
    "svo_world_load_chunk": (C.c_int, (vp, u32)),
    "svo_world_load": (vp, (cp, cp, sz)),
    "svo_cpu_octree_bin": (sz, (vp, vp, sz)),
    "svo_cpu_octree_from_bin": (vp, (cp, sz, cp, sz)),
    "svo_adaptive_subdivide": (i64, (vp, vp, vp, sz, C.POINTER(u64))),
    "svo_adaptive_unsubdivide": (i64, (vp, vp, vp, sz)),
    "svo_world_expand": (u64, (vp, vp, u32, fp, f32, u64)),
    "svo_camera_matrices": (None, (fp, fp, f32, f32, f32, fp, fp)),
    "svo_gen_terrain": (u64, (C.POINTER(TerrainParams), vp, u64)),
    "svo_gen_terrain_height": (C.c_int32, (u32, u32, u32, u32)),
    "svo_gen_fractal": (u64, (C.POINTER(TerrainParams), vp, u64)),
    "svo_gen_random": (u64, (u32, u32, f32, f32, u64, vp, u64)),
    "svo_nodes_max_depth": (u32, (vp, u64)),
    "svo_nodes_relayout": (u64, (vp, u64, u32, vp, vp)),
}
DEVICE_SYMBOLS, HOST_SYMBOLS = list(DEVICE_SIGNATURES), list(HOST_SIGNATURES)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C octree-tracer_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    for table in (DEVICE_SIGNATURES, HOST_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = list(args)
    _lib = L
    return L


class SvoError(RuntimeError):
    pass
