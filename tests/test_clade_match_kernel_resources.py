"""Resources of the clade matching kernel (CPU: hipcc's resource-usage remarks of the gfx950 code object): k_clade_match
keeps nothing in scratch memory, spills no register and declares no static LDS (its bitmap, counts and the words in which
the waves meet are all in the dynamic region, whose base is then 16-byte aligned).  The VGPR count is the one DESIGN.md
section 20 records."""
import os

import pytest

from kernel_resources import HIPCC, resources

VGPRS = {"k_clade_match": 58}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_clade_match_kernel_uses_no_scratch_and_spills_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_clade_match" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0 and v["lds"] == 0, (k, v)
        assert v["vgpr"] == vgprs and v["occupancy"] == 8, (k, v)
