"""Resources of the partner-dispersion kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the three
task forms (packed, one wave, one workgroup) and the two instantiations of the sigma kernel (256 and 1024 lanes) keep
nothing in scratch memory and spill no register.  The VGPR counts are those DESIGN.md section 18 records."""
import os

import pytest

from kernel_resources import HIPCC, resources

VGPRS = {"k_dispersion_tasks_packed": 32, "k_dispersion_tasks_wave": 30, "k_dispersion_tasks_group": 27,
         "k_dispersion_sigmaILi256E": 16, "k_dispersion_sigmaILi1024E": 16}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_dispersion_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_dispersion" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
