"""The structure kernels' resources, checked at build time with the method of test_list_resources.py (no GPU needed: hipcc
cross-compiles gfx950): every kernel of csrc/svo_structure.hip exists in its device code and runs without scratch, and
the column walk keeps its path in LDS, 21 levels x 256 lanes x 4 bytes (DESIGN.md 22 has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("column_tops_kernel", "sites_sum_kernel", "sites_emit_kernel", "stamp_check_kernel", "stamp_bad_kernel", "stamp_sum_kernel",
           "stamp_emit_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_structure_kernel_uses_scratch():
    res = _resources("svo_structure.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    tops = next(r for k, r in kernels.items() if "column_tops_kernel" in k)
    assert tops["lds"] == 21 * 256 * 4
