"""The voxeliser's kernels' resources, checked at build time with the method of test_list_resources.py (no GPU needed:
hipcc cross-compiles gfx950): every kernel that csrc/svo_voxelize.hip launches exists in its device code, the shared tile
kernels of svo_scan.h as the instantiations with this file's functors, and runs without scratch, the 128-bit plane test
included; the two row-wise emits keep the tile's ranks in LDS, padded by one word per 32, beside the block scan's 1 KiB
(DESIGN.md 12 and 20 have the tables)."""
import shutil

import pytest

from test_list_resources import HIPCC, _instances, _resources

# (kernel, the functor types of the instantiation)
KERNELS = (("vox_setup_kernel",), ("min_of_blocks_kernel",), ("vox_test_kernel",), ("tile_count_kernel", "Pairs"), ("vox_total_kernel",),
           ("tile_scatter_kernel", "Pairs", "Children"), ("tile_offsets_kernel",))
TILE = 256 * 16


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_voxeliser_kernel_uses_scratch():
    res = _resources("svo_voxelize.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert _instances(kernels, *want), (want, sorted(kernels))
    scatters = _instances(kernels, "tile_scatter_kernel", "Pairs", "Children")
    assert len(scatters) == 2  # the levels' and the emit's
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    for name, r in scatters.items():
        assert r["lds"] == (TILE + TILE // 32) * 4 + 1024 == 17920, name
