"""Resources of the UniFrac kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the table and widen
kernels and the two pair forms (one pair per lane, one pair per wave) keep nothing in scratch memory and spill no
register.  The VGPR counts are those DESIGN.md section 19 records."""
import os

import pytest

from kernel_resources import HIPCC, resources

VGPRS = {"k_unifrac_table": 10, "k_unifrac_widen": 6, "k_unifrac_lane": 26, "k_unifrac_wave": 32}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_unifrac_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_unifrac" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
