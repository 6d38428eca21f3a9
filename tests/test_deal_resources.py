"""The replay twin of the default trace kernel (trace_stack_replay_kernel) lives within the same register budget as
the kernel whose claims it replaces: it is launched on the same grid, seven waves per SIMD, and a spilled register inside the round
would cost it more than the claims it saves.  The compiler's own resource report, as in test_kernel_resources.py."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_replay_kernel_fits_seven_waves_without_spilling():
    res = _resources()
    for ge in ("0", "1"):
        name = f"_ZN3svo25trace_stack_replay_kernelILi256ELi12ELi3ELb{ge}EEEvNS_9TraceArgsEjPj"
        assert name in res, sorted(k for k in res if "replay" in k)
        r = res[name]
        assert r["scratch"] == 0, f"{name} spills {r['scratch']} bytes per lane"
        assert r["vgpr"] <= 72 and r["occupancy"] >= 7, r
        # it drops the claim code's scalar state: no more scalar registers than the claiming kernel
        claiming = res[f"_ZN3svo18trace_stack_kernelILi256ELi12ELi3ELb{ge}ELb0ELb0ELb0EEEvNS_9TraceArgsEjPjS2_"]
        assert r["sgpr"] <= claiming["sgpr"], (r, claiming)
