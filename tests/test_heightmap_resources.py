"""The height-map edit's kernels' resources, checked at build time with the method of test_sample_resources.py (no GPU needed:
hipcc cross-compiles gfx950): every kernel of csrc/svo_heightmap.hip exists in its device code and runs without scratch;
the pyramid kernel's three instantiations keep the registers and the LDS that DESIGN.md 32 states, so every one of them
runs eight waves per SIMD."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("heightmap_pyramid_kernel", "heightmap_plan_kernel", "heightmap_emit_kernel", "region_mark_kernel", "region_check_kernel",
           "region_fill_kernel", "region_write_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_heightmap_kernel_uses_scratch():
    res = _resources("svo_heightmap.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    pyramid = {k: r for k, r in kernels.items() if "heightmap_pyramid_kernel" in k}
    assert len(pyramid) == 3, sorted(pyramid)  # the map by single heights, by four along z, a level's pairs
    for name, r in pyramid.items():
        assert r["vgpr"] <= 64 and r["lds"] == 128 and r["occupancy"] == 8, (name, r)
