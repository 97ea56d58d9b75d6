"""Resources of the linkage kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the two grid passes
and the chain with its cache in LDS and in global memory keep nothing in scratch memory, spill no register, and their
static LDS -- the partial minima of the workgroup reductions -- with the largest dynamic request, 16 bytes per slot up
to kLinkageLdsMaxObjects, fits the 160 KiB of a CU.  The chain is one workgroup of 1024 threads, four waves a SIMD: 128
VGPRs at the most."""
import os
import re

import pytest

from conftest import ROOT
from kernel_resources import HIPCC, resources

# (k_linkage_chain<Lds>: <true> keeps the cache in LDS)
KERNELS = ("k_linkage_expand", "k_linkage_nearest", "k_linkage_chainILb1E", "k_linkage_chainILb0E")
# a candidate is 24 bytes: one per wave of the workgroup, twice in the chain (the pick, row a's entry)
STATIC_LDS = {"k_linkage_expand": 0, "k_linkage_nearest": 4 * 24, "k_linkage_chainILb1E": 2 * 16 * 24, "k_linkage_chainILb0E": 2 * 16 * 24}
LDS_BYTES = 160 * 1024


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_linkage_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_linkage" in k}
    assert len(mine) == len(KERNELS), sorted(mine)
    plan = open(os.path.join(ROOT, "suchtree_amd", "csrc", "linkage_plan.h")).read()
    lds_max = int(re.search(r"kLinkageLdsMaxObjects = (\d+);", plan).group(1))
    for kernel in KERNELS:
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["lds"] == STATIC_LDS[kernel], (k, v)
        assert v["vgpr"] <= 128, (k, v)
        dynamic = 16 * lds_max if kernel == "k_linkage_chainILb1E" else 0
        assert v["lds"] + dynamic <= LDS_BYTES, (k, v, dynamic)
