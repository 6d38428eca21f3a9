"""The solid voxeliser's kernels' resources, checked at build time with the method of test_voxelize_resources.py (no GPU
needed: hipcc cross-compiles gfx950): every kernel that csrc/svo_solid.hip launches exists in its device code, the shared
tile kernels of svo_scan.h as the instantiations with this file's functors, and runs without scratch, the 128-bit
bisection of the heights included (DESIGN.md 24 has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _instances, _resources

# (kernel, the functor types of the instantiation)
KERNELS = (("solid_setup_kernel",), ("min_of_blocks_kernel",), ("solid_test_kernel",), ("solid_total_kernel",), ("tile_offsets_kernel",),
           ("tile_count_kernel", "Squares"), ("tile_scatter_kernel", "Squares", "Children"),
           ("tile_count_kernel", "Heads"), ("tile_emit_kernel", "Heads"), ("tile_count_kernel", "OpenColumns"),
           ("tile_count_kernel", "Intervals"), ("tile_emit_kernel", "Intervals"), ("tile_count_kernel", "Runs"), ("tile_emit_kernel", "Runs"),
           ("tile_count_kernel", "ScanInPlace"), ("tile_emit_kernel", "ScanInPlace"),
           ("solid_lengths_kernel",), ("solid_cells_kernel",))
TILE = 256 * 16


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_solid_kernel_uses_scratch():
    res = _resources("svo_solid.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert _instances(kernels, *want), (want, sorted(kernels))
    assert len(_instances(kernels, "solid_test_kernel")) == 2  # the overlap levels' and the covering level's
    assert len(_instances(kernels, "solid_total_kernel")) == 2  # over a level's tile sums (u32) and the spans' block sums (u64)
    scatters = _instances(kernels, "tile_scatter_kernel", "Squares", "Children")
    assert len(scatters) == 2  # the levels' and the crossings'
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    for name, r in scatters.items():
        assert r["lds"] == (TILE + TILE // 32) * 4 + 1024 == 17920, name
    (cells,) = _instances(kernels, "solid_cells_kernel").values()
    assert cells["lds"] == TILE * 4 + 8, cells  # a tile's offsets and the two searches' results
