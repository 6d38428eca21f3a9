"""The distance kernels' resources, checked at build time with the method of test_list_resources.py (no GPU needed: hipcc
cross-compiles gfx950): every kernel that DESIGN.md 35 names exists in the device code of csrc/svo_distance.hip, the table's
kernels are the file's, and none runs with scratch."""
import os
import re
import shutil

import pytest

from test_list_resources import HIPCC, ROOT, _resources

KERNELS = ("distance_bits_kernel", "distance_zy_kernel", "distance_x_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_distance_kernel_uses_scratch():
    res = _resources("svo_distance.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    assert len(kernels) == 4  # the x pass in two instantiations
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        assert r["lds"] == 0 and r["occupancy"] == 8, (name, r)


def test_the_design_names_the_files_kernels():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 35."):]
    named = set(re.findall(r"distance_\w+_kernel", section))
    assert named == set(KERNELS), named
    source = open(os.path.join(ROOT, "octree-tracer_amd", "csrc", "svo_distance.hip")).read()
    assert set(re.findall(r"void (distance_\w+_kernel)\(", source)) == set(KERNELS)
