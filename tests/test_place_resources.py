"""The placement's kernels' resources, checked at build time with the method of test_combine_resources.py (no GPU needed: hipcc
cross-compiles gfx950): every kernel that csrc/svo_place.hip launches exists in its device code -- its own root, plan and emit,
the check and commit kernels it shares with the shape edit and the combine through csrc/svo_frontier.h, and the scans' and the
status' kernels of csrc/svo_scan.h -- and runs without scratch: a lane reads its parent's eight items from the group's record by
a computed index and keeps none of them in an array (DESIGN.md 30 has the table)."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("place_root_kernel", "place_plan_kernel", "place_emit_kernel", "region_mark_kernel", "region_check_kernel", "region_fill_kernel",
           "region_write_kernel", "tile_count_kernel", "tile_offsets_kernel", "tile_emit_kernel", "min_of_blocks_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_place_kernel_uses_scratch():
    res = _resources("svo_place.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    assert not any("combine_plan_kernel" in k or "combine_emit_kernel" in k for k in kernels)  # (the combine's own stay in its file)
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    # the plan and the emit hold eight items' worth of state in a handful of registers, not in eight
    for want in ("place_plan_kernel", "place_emit_kernel"):
        assert all(r["vgpr"] <= 64 for k, r in kernels.items() if want in k)
