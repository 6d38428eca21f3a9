"""The simplification kernels' resources, checked at build time with the method of test_list_resources.py (no GPU needed:
hipcc cross-compiles gfx950): every kernel of csrc/svo_simplify.hip exists in the gfx950 code object, runs without
scratch and without LDS, and leaves room for 8 waves per SIMD (DESIGN.md 26 has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("simplify_reduce_kernel", "simplify_total_kernel", "simplify_emit_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_simplify_kernel_uses_scratch():
    res = _resources("svo_simplify.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        if any(want in name for want in KERNELS):  # (the shared discovery and scan kernels are their own files' business)
            assert r["lds"] == 0 and r["occupancy"] == 8, (name, r)
