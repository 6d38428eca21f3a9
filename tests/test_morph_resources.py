"""The morphology's kernels' resources, checked at build time with the method of test_place_resources.py (no GPU needed: hipcc
cross-compiles gfx950): every kernel that csrc/svo_morph.hip launches exists in its device code -- its own root, plan and emit,
the check and commit kernels it shares with the shape edit, the combine and the placement through csrc/svo_frontier.h, and the
scans' and the status' kernels of csrc/svo_scan.h -- and runs without scratch: a lane derives each of its up to 26 items from
the group's record by a computed index and folds it into three counters, keeping none in an array (DESIGN.md 31 has the table).
Eight waves per SIMD need at most 64 registers a lane (512 / 8): the build reaches that for both kernels, so it is asserted."""
import shutil

import pytest

from test_list_resources import HIPCC, _resources

KERNELS = ("morph_root_kernel", "morph_plan_kernel", "morph_emit_kernel", "region_mark_kernel", "region_check_kernel", "region_fill_kernel",
           "region_write_kernel", "tile_count_kernel", "tile_offsets_kernel", "tile_emit_kernel", "min_of_blocks_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_morph_kernel_uses_scratch():
    res = _resources("svo_morph.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    assert not any("place_plan_kernel" in k or "place_emit_kernel" in k for k in kernels)  # (the placement's own stay in its file)
    for name, r in kernels.items():
        print(name, r)
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    # 26 items' worth of state in a handful of registers: eight waves per SIMD
    for want in ("morph_plan_kernel", "morph_emit_kernel"):
        assert all(r["vgpr"] <= 64 for k, r in kernels.items() if want in k)
