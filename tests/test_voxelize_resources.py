"""The voxeliser's kernels' resources, checked at build time with the method of test_list_resources.py (no GPU needed:
hipcc cross-compiles gfx950): every kernel of csrc/svo_voxelize.hip exists in its device code and runs without scratch,
the 128-bit plane test included (DESIGN.md 20 has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("vox_setup_kernel", "vox_bad_kernel", "vox_test_kernel", "vox_sum_kernel", "vox_total_kernel", "vox_scatter_kernel",
           "tile_offsets_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_voxeliser_kernel_uses_scratch():
    res = _resources("svo_voxelize.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    assert sum("vox_scatter_kernel" in k for k in kernels) == 2  # the levels' and the emit's
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
