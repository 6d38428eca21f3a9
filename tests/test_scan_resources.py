"""The shared tile kernels of csrc/svo_scan.h as the builder, the generator and the adaptive expand instantiate them,
checked at build time with the method of test_list_resources.py (no GPU needed: hipcc cross-compiles gfx950): every
instantiation that the file launches exists in its device code and no kernel of the file uses scratch.  A thread's state
(16 keys in the builder) lives in registers only while the functors' loops unroll; DESIGN.md 12 has the table."""
import shutil

import pytest

from test_list_resources import HIPCC, _instances, _resources

# file -> (kernel, the functor types of the instantiation, how many instantiations)
FILES = {
    "svo_build.hip": (("tile_count_kernel", "Level", 4), ("tile_emit_kernel", "Level", "LevelEmit", 4), ("tile_count_kernel", "ScanInPlace", 1),
                      ("tile_emit_kernel", "ScanInPlace", 1), ("tile_offsets_kernel", 1)),
    "svo_proc.hip": (("tile_count_kernel", "LevelMasks", 1), ("tile_emit_kernel", "LevelMasks", "WriteRanks", 1), ("tile_offsets_kernel", 1)),
    "svo_adapt.hip": (("tile_count_kernel", "Compaction", "LeafWord", "EmitLeaf", 1), ("tile_emit_kernel", "Compaction", "LeafWord", "EmitLeaf", 1),
                      ("tile_count_kernel", "Compaction", "ViewRefines", "EmitCandidate", 1),
                      ("tile_emit_kernel", "Compaction", "ViewRefines", "EmitCandidate", 1),
                      ("tile_count_kernel", "ScanInPlace", 1), ("tile_emit_kernel", "ScanInPlace", 1), ("tile_offsets_kernel", 1)),
}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
@pytest.mark.parametrize("name", sorted(FILES))
def test_tile_kernels_exist_without_scratch(name):
    res = _resources(name)
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for *want, count in FILES[name]:
        assert len(_instances(kernels, *want)) == count, (want, sorted(kernels))
    for k, r in kernels.items():
        assert r["scratch"] == 0, f"{k} uses {r['scratch']} bytes of scratch per lane"
