"""Register budgets of the kernels whose occupancy depends on them (CPU: hipcc's resource-usage remarks of the
gfx950 code objects).  A 1024-lane workgroup needs <= 128 VGPRs to launch at all and <= 64 for two of them per CU;
a cold path inlined into a hot kernel has pushed one over that line before (round 4: the pipelined chain sum in
the shared-portal path took k_canopy_ladder<15> from 51 to 77 VGPRs and ml.tree from 2.85e10 to 1.92e10 pairs/s)."""
import os

import pytest

from kernel_resources import HIPCC, resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_register_budgets_of_the_canopy_kernels():
    v = resources("launch_canopy.hip")
    for k, n in v.items():
        assert n["vgpr_spill"] == 0, (k, "spills")

    def of(fragment):
        hits = {k: n for k, n in v.items() if fragment in k}
        assert hits, fragment
        return hits

    # two 1024-lane workgroups per CU (canopy / ladder images of at most 80 KiB) are 8 waves per SIMD: at most 64
    # VGPRs and at most 80 SGPRs (the hardware admits floor(800 / (sgprs rounded up to 16 + 16)) waves per SIMD)
    for frag in ("k_canopy_ilpILi7ELi1E", "k_canopy_ilpILi3ELi1E", "k_canopy_ilpILi1ELi1E", "k_canopy_ladderILi15E"):
        for k, n in of(frag).items():
            assert n["vgpr"] <= 64 and n["sgpr"] <= 80, (k, n)
    # every kernel of the family is launched with 1024 lanes: at most 128 VGPRs
    for k, n in v.items():
        if "k_canopy" in k or "k_mrca_ranks" in k:
            assert n["vgpr"] <= 128, (k, n)
