"""The affine placement's kernels' resources, checked at build time with the method of test_place_resources.py (no GPU needed:
hipcc cross-compiles gfx950): every kernel that csrc/svo_transform.hip launches exists in its device code -- its own root, plan
and emit, the check and commit kernels it shares with the other top-down edits through csrc/svo_frontier.h, and the scans' and
the status' kernels of csrc/svo_scan.h -- and runs without scratch: a lane folds its up to eight items into five counters as it
finds them and keeps none of them in an array.  The plan and the emit stay at 64 VGPRs or fewer, eight waves per SIMD, the bound
the placement is held to (DESIGN.md 34 has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("transform_root_kernel", "transform_plan_kernel", "transform_emit_kernel", "region_mark_kernel", "region_check_kernel",
           "region_fill_kernel", "region_write_kernel", "tile_count_kernel", "tile_offsets_kernel", "tile_emit_kernel", "min_of_blocks_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_transform_kernel_uses_scratch():
    res = _resources("svo_transform.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    assert not any("place_plan_kernel" in k or "combine_plan_kernel" in k for k in kernels)  # (the other passes' own stay in their files)
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    for want in ("transform_plan_kernel", "transform_emit_kernel"):
        assert all(r["vgpr"] <= 64 and r["occupancy"] == 8 for k, r in kernels.items() if want in k)
