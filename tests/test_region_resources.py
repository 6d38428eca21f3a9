"""The shape edit's kernels' resources, checked at build time with the method of test_sample_resources.py (no GPU needed:
hipcc cross-compiles gfx950): every kernel of csrc/svo_region.hip exists in its device code and runs without scratch
(DESIGN.md 25 has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("region_plan_kernel", "region_emit_kernel", "region_mark_kernel", "region_check_kernel", "region_fill_kernel",
           "region_write_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_region_kernel_uses_scratch():
    res = _resources("svo_region.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
