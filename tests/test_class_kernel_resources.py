"""Resources of the class-sum kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the expand, the
wave form, the row form -- with its LDS accumulators and in the compare form it was measured against -- and the fold keep
nothing in scratch memory and spill no register.  The VGPR counts are those DESIGN.md section 26 records, of the first
build that met the tests."""
import os

import pytest

from kernel_resources import HIPCC, resources

# (k_class_rows<Compare>: <true> is the measurement form without the LDS accumulators)
VGPRS = {"k_class_expand": 10, "k_class_wave": 12, "k_class_rowsILb0E": 55, "k_class_rowsILb1E": 55, "k_class_fold": 12}
# the wave form: y (64 x 65 words), the class square (64 x 68 bytes) and four waves' accumulators (64 classes x 4 copies x 8 bytes)
STATIC_LDS = {"k_class_expand": 0, "k_class_wave": 16640 + 4352 + 8192, "k_class_rowsILb0E": 8192, "k_class_rowsILb1E": 0, "k_class_fold": 2048}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_class_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_class" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
        assert v["lds"] == STATIC_LDS[kernel], (k, v)      # (the row form's row pair and its waves' class rows are dynamic: 8 n + 16 bytes on top)
