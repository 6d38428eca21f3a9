"""The listing kernels' resources, checked at build time with the method of test_kernel_resources.py (no GPU needed: hipcc
cross-compiles gfx950): every kernel of csrc/svo_list.hip runs without scratch (DESIGN.md 18 has the table)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("list_count_kernel", "list_root_kernel", "list_offsets_kernel", "list_emit_kernel", "list_expand_kernel")


def _resources(name):
    src = os.path.join(ROOT, "octree-tracer_amd", "csrc", name)
    mk = open(os.path.join(ROOT, "octree-tracer_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("-I../../include", "-I" + os.path.join(ROOT, "include"))
    cmd = [HIPCC] + [f for f in flags.split() if f not in ("-fPIC", "-Wall")] + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", "/dev/null"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return out


def _instances(kernels, kernel, *functors):
    """The entries of `kernels` (mangled name -> figures) that are `kernel`, instantiated with the functor types `functors`:
    a type's name stands in the mangled symbol behind its length."""
    parts = [f"{len(p)}{p}" for p in (kernel,) + functors]
    return {k: r for k, r in kernels.items() if all(p in k for p in parts)}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_no_listing_kernel_uses_scratch():
    res = _resources("svo_list.hip")
    kernels = {k: r for k, r in res.items() if "kernel" in k}
    for want in KERNELS:
        assert any(want in k for k in kernels), (want, sorted(kernels))
    for name, r in kernels.items():
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
