"""The structure kernels' resources, checked at build time with the method of test_list_resources.py (no GPU needed: hipcc
cross-compiles gfx950): every kernel that csrc/svo_structure.hip launches exists in its device code, the shared tile
kernels of svo_scan.h as the instantiations with this file's functors, and runs without scratch; the column walk keeps
its path in LDS, 21 levels x 256 lanes x 4 bytes, and the stamp's row-wise emit the tile's ranks, padded by one word per
32, beside the block scan's 1 KiB (DESIGN.md 12 and 22 have the tables)."""
import shutil

import pytest

from test_list_resources import HIPCC, _instances, _resources

# (kernel, the functor types of the instantiation)
KERNELS = (("column_tops_kernel",), ("tile_count_kernel", "Sites"), ("tile_emit_kernel", "Sites", "SitesOut"), ("stamp_check_kernel",),
           ("min_of_blocks_kernel",), ("tile_count_kernel", "Stamp"), ("tile_scatter_kernel", "Stamp", "StampOut"),
           ("tile_offsets_kernel",))
TILE = 256 * 16


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_structure_kernel_uses_scratch():
    res = _resources("svo_structure.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert len(_instances(kernels, *want)) == 1, (want, sorted(kernels))
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    tops = next(r for k, r in kernels.items() if "column_tops_kernel" in k)
    assert tops["lds"] == 21 * 256 * 4
    (scatter,) = _instances(kernels, "tile_scatter_kernel", "Stamp", "StampOut").values()
    assert scatter["lds"] == (TILE + TILE // 32) * 4 + 1024 == 17920
