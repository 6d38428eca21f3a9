"""The component kernels' resources, checked at build time with the method of test_surface_resources.py (no GPU needed: hipcc
cross-compiles gfx950): every kernel that csrc/svo_components.hip launches exists in its device code, the shared tile
kernels of svo_scan.h as the instantiations with this file's functors, and runs without scratch; the link kernel keeps one
path per wave in LDS, 21 levels x 4 waves x 4 bytes (DESIGN.md 29 has the table)."""
import os
import re
import shutil

import pytest

from test_list_resources import HIPCC, ROOT, _instances, _resources

# (kernel, the functor types of the instantiation)
KERNELS = (("components_link_kernel",), ("components_init_kernel",), ("components_hook_kernel",), ("components_compress_kernel",),
           ("components_id_kernel",), ("scatter_device_kernel",), ("tile_count_kernel", "Roots"), ("tile_offsets_kernel",),
           ("tile_emit_kernel", "Roots", "RootNumbers"))


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_components_kernel_uses_scratch():
    res = _resources("svo_components.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert len(_instances(kernels, *want)) == 1, (want, sorted(kernels))
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
    (link,) = _instances(kernels, "components_link_kernel").values()
    assert link["lds"] == 21 * 4 * 4 == 336
    # the figure DESIGN.md 29 states in its kernel table
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    row = re.search(r"^\| `components_link_kernel` \|(.*)\|$", design, re.M)
    assert row, "DESIGN.md 29 has no row for components_link_kernel"
    lds, scratch = (int(x) for x in re.findall(r"\d+", row.group(1))[2:4])  # (behind the VGPRs and SGPRs)
    assert (lds, scratch) == (link["lds"], 0)
