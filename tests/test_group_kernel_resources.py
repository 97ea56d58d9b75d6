"""Resources of the group-sum kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the relabel, the
wave form, the row form and the fold keep nothing in scratch memory and spill no register.  The VGPR counts are those
DESIGN.md section 24 records, of the first build that met the tests."""
import os

import pytest

from kernel_resources import HIPCC, resources

VGPRS = {"k_group_relabel": 6, "k_group_wave": 11, "k_group_rows": 66, "k_group_fold": 9}
STATIC_LDS = {"k_group_relabel": 0, "k_group_wave": 16640, "k_group_rows": 0, "k_group_fold": 2048}      # (the fold: 256 int64 accumulators)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_group_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_group_" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
        assert v["lds"] == STATIC_LDS[kernel], (k, v)      # (the row form's row is dynamic: 4 n bytes on top)
