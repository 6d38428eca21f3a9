"""The simplification kernels' resources, checked at build time with the method of test_list_resources.py (no GPU needed:
hipcc cross-compiles gfx950): the reduce of csrc/svo_simplify.hip and the total and emit kernels of the canonical rewrite
that it shares with the compaction (csrc/svo_compact.hip) exist in the gfx950 code object, run without scratch and without
LDS, and leave room for 8 waves per SIMD (DESIGN.md 17 and 26 have the tables)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = {"svo_simplify.hip": ("simplify_reduce_kernel",), "svo_compact.hip": ("rewrite_total_kernel", "rewrite_emit_kernel")}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_simplify_kernel_uses_scratch():
    for source, wanted in KERNELS.items():
        res = _resources(source)
        kernels = {k: r for k, r in res.items() if "kernel" in k}
        for want in wanted:
            assert any(want in k for k in kernels), (want, sorted(kernels))
        for name, r in kernels.items():
            assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
            if any(want in name for want in wanted):  # (the shared discovery and scan kernels are their own files' business)
                assert r["lds"] == 0 and r["occupancy"] == 8, (name, r)
