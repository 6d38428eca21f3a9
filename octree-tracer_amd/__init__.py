"""octree-tracer_amd: MI355X-native drop-in for the GPU path of ria8651/octree-tracer.

Host-side mirror of the reference's dispatch API (same names and argument meaning) over the
C ABI of libsvo_hip.so:
    gpu.Gpu            <- src/gpu.rs      Gpu
    render.Render      <- src/render.rs   Render {new, update, render, resize}, Uniforms
    compute.Compute    <- src/compute.rs  Compute {new, update}
    octree.Octree      <- src/octree.rs   Octree, Voxel, VOXEL_OFFSET
    cpu_octree.CpuOctree <- src/cpu_octree.rs CpuOctree
    camera.{Character, Settings} <- src/main.rs
    world.World        <- src/world.rs    World {chunks, find_voxel, generate_mip_tree, save/load_chunk, load_world, generate_world}
    procedural.Procedural <- src/procedural.rs Procedural {generate_chunk} (deterministic: DESIGN.md 11)
    adaptive           <- src/adaptive.rs  process_subdivision / process_unsubdivision
    scenes             deterministic benchmark scene generators (no reference counterpart)
    mesh               triangle meshes voxelised on the GPU into voxel lists, a tree's visible surface as a triangle mesh, a Wavefront
                       reader and writer, mesh generators (no reference counterpart)
    region             boxes and balls for Render.edit_region: fill, carve and paint a device tree by shapes (no reference counterpart)
    orientation        the cube's 48 symmetries as Render.place_nodes numbers them (no reference counterpart)
    distance           what Render.distance_dense returns, taken apart: FAR, NO_SITE, the packed sites, radius masks (no reference counterpart)
    transform          affine maps in Q16 as Render.transform_nodes takes them: turns, scale, shear (no reference counterpart)
    structure.Structure <- src/cpu_octree.rs CpuOctree::load_structure: a .vox model as offsets, block indices and colours
The package directory name contains a hyphen; import it through __graft_entry__.load_package(),
which registers it as module `octree_tracer_amd`.
"""
from . import _lib
from ._lib import SvoError, Uniforms
from .octree import VOXEL_OFFSET, Octree, Voxel, create_node
from .cpu_octree import CHUNK_OFFSET, CpuOctree
from .camera import Character, Settings, camera_matrices
from .gpu import Gpu
from .render import Render, HIT_DTYPE, F_PAUSE_ADAPTIVE, F_SHOW_STEPS, F_SHOW_HITS, F_SHADOWS, F_MISC_BOOL
from .render import SAMPLE_FINER, SAMPLE_OUTSIDE, SAMPLE_BROKEN, TOP_NONE, MORPH_OPS, HEIGHTMAP_MODES
from .structure import Structure, load_structure
from .compute import Compute
from .world import World
from .procedural import Procedural
from . import procedural
from . import scenes
from . import mesh
from . import region
from . import orientation
from . import transform
from . import distance
from . import structure
from . import sharding
from . import adaptive

__all__ = ["Gpu", "Render", "Compute", "Octree", "CpuOctree", "Voxel", "World", "Procedural", "Uniforms", "Character", "Settings",
           "SvoError", "SAMPLE_FINER", "SAMPLE_OUTSIDE", "SAMPLE_BROKEN", "TOP_NONE", "MORPH_OPS", "HEIGHTMAP_MODES", "Structure", "load_structure", "VOXEL_OFFSET", "CHUNK_OFFSET", "HIT_DTYPE", "create_node", "camera_matrices", "scenes", "mesh", "region", "orientation", "transform", "distance", "structure", "sharding", "adaptive", "procedural"]
