"""The sampling kernels' resources, checked at build time with the method of test_list_resources.py (no GPU needed: hipcc
cross-compiles gfx950): both kernels of csrc/svo_sample.hip exist in its device code and run without scratch (DESIGN.md 19
has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("sample_cells_kernel", "sample_dense_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_sampling_kernel_uses_scratch():
    res = _resources("svo_sample.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
