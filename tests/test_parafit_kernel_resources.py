"""Resources of the ParaFit kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the expansion, the
three relabel forms, the row form, the wave form and the fold keep nothing in scratch memory and spill no register.
The VGPR counts are those DESIGN.md section 25 records, of the first build that met the tests."""
import os

import pytest

from kernel_resources import HIPCC, resources

# (k_parafit_relabel<T>: T = 256 the small sort class, 1024 the large one)
VGPRS = {"k_parafit_expand": 6, "k_parafit_relabel_wave": 21, "k_parafit_relabelILi256E": 15, "k_parafit_relabelILi1024E": 15, "k_parafit_rows": 52,
         "k_parafit_wave": 52, "k_parafit_fold": 12}
STATIC_LDS = {k: 33280 if k == "k_parafit_wave" else 80 if k == "k_parafit_rows" else 0 for k in VGPRS}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_parafit_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_parafit" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
        assert v["lds"] == STATIC_LDS[kernel], (k, v)      # (the row form's row and the sorts' keys are dynamic, on top)
