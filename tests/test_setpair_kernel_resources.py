"""Resources of the between-set dispersion kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the
three task forms (packed, one wave, one workgroup) keep nothing in scratch memory and spill no register.  The VGPR counts
are those DESIGN.md section 21 records."""
import os

import pytest

from kernel_resources import HIPCC, resources

VGPRS = {"k_setpair_tasks_packed": 42, "k_setpair_tasks_wave": 30, "k_setpair_tasks_group": 37}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_setpair_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_setpair" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
