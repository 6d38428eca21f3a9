"""The combine's kernels' resources, checked at build time with the method of test_sample_resources.py (no GPU needed:
hipcc cross-compiles gfx950): every kernel that csrc/svo_combine.hip launches exists in its device code -- its own plan and
emit, and the shape edit's check and commit kernels, which it shares through csrc/svo_frontier.h -- and runs without scratch
(DESIGN.md 27 has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("combine_plan_kernel", "combine_emit_kernel", "region_mark_kernel", "region_check_kernel", "region_fill_kernel",
           "region_write_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_combine_kernel_uses_scratch():
    res = _resources("svo_combine.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    assert not any("region_plan_kernel" in k or "region_emit_kernel" in k for k in kernels)  # (the shape edit's own stay in its file)
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
