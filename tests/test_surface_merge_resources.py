"""The merge kernels' resources, checked at build time with the method of test_surface_resources.py (no GPU needed: hipcc
cross-compiles gfx950): every kernel that csrc/svo_surface_merge.hip launches exists in its device code, the shared tile
kernels of svo_scan.h as the instantiations with this file's functors, and runs without scratch; the pass's own kernels
use no LDS, the tile kernels the block scan's 256 words (DESIGN.md 28 has the table)."""
import os
import re
import shutil

import pytest

from test_list_resources import HIPCC, ROOT, _instances, _resources

# the row's name in DESIGN.md 28 -> (the kernel and the functor types of the instantiation, or its template argument as
# the mangled name spells it; LDS bytes)
KERNELS = {
    "merge_keys_kernel<true>": (("merge_keys_kernel", "ILb1EE"), 0),
    "merge_keys_kernel<false>": (("merge_keys_kernel", "ILb0EE"), 0),
    "merge_gather_kernel": (("merge_gather_kernel",), 0),
    "merge_flag_kernel": (("merge_flag_kernel",), 0),
    "tile_count_kernel<Runs>": (("tile_count_kernel", "Runs"), 256 * 4),
    "tile_emit_kernel<Runs, RunsOut>": (("tile_emit_kernel", "Runs", "RunsOut"), 256 * 4),
    "merge_out_kernel": (("merge_out_kernel",), 0),
}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_merge_kernel_uses_scratch():
    res = _resources("svo_surface_merge.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for row_name, (parts, lds) in KERNELS.items():
        found = {k: r for k, r in _instances(kernels, parts[0]).items() if parts[1] in k} if parts[1:] and parts[1].startswith("ILb") \
            else _instances(kernels, *parts)
        assert len(found) == 1, (row_name, sorted(kernels))
        (r,) = found.values()
        assert r["lds"] == lds, row_name
        # the figures DESIGN.md 28 states in its kernel table
        row = re.search(rf"^\| `{re.escape(row_name)}` \|(.*)\|$", design, re.M)
        assert row, f"DESIGN.md 28 has no row for {row_name}"
        stated = [int(x) for x in re.findall(r"\d+", row.group(1))[2:4]]  # (behind the VGPRs and SGPRs)
        assert stated == [lds, 0], row_name
