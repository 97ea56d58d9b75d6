"""Resources of the kernels of the UniFrac null (CPU: hipcc's resource-usage remarks of the gfx950 code object): the set
kernel (one wave per task, a 2 KiB bitmap in LDS) and the two pair forms over the relabelled table (one task per lane, one
per wave) keep nothing in scratch memory and spill no register.  The VGPR counts are those DESIGN.md section 22 records.
(The kernels are named k_null_unifrac_*: tests/test_unifrac_kernel_resources.py counts every kernel whose name holds
"k_unifrac".)"""
import os

import pytest

from kernel_resources import HIPCC, resources

VGPRS = {"k_null_unifrac_sets": 32, "k_null_unifrac_lane": 26, "k_null_unifrac_wave": 34}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_unifrac_null_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_null_unifrac" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
    assert [v["lds"] for k, v in mine.items() if "k_null_unifrac_sets" in k] == [2048]
