"""Resources of the Mantel kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the wave form, the row
form -- each in its simple and partial instance -- and the fold keep nothing in scratch memory and spill no register.
The VGPR counts are those DESIGN.md section 23 records, of the first build that met the tests."""
import os

import pytest

from kernel_resources import HIPCC, resources

# (k_mantel_rows<Z, Gather>: <.., true> is the measurement form without the LDS row)
VGPRS = {"k_mantel_waveILb0E": 51, "k_mantel_waveILb1E": 51, "k_mantel_rowsILb0ELb0E": 65, "k_mantel_rowsILb1ELb0E": 72,
         "k_mantel_rowsILb0ELb1E": 30, "k_mantel_rowsILb1ELb1E": 47, "k_mantel_fold": 22}
STATIC_LDS = {k: 16640 if "wave" in k else 128 if "rows" in k else 0 for k in VGPRS}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mantel_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_mantel" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
        assert v["lds"] == STATIC_LDS[kernel], (k, v)      # (the row form's row is dynamic: 4 n bytes on top)
