"""Resources of the per-clade Hommola kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the
relabelling kernels (one wave, 256 lanes, 1024 lanes) and k_hommola_blocks keep nothing in scratch memory and spill no
register -- the 1024-lane form has 128 VGPRs per lane at the most."""
import os

import pytest

from kernel_resources import HIPCC, resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_hommola_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_hommola_relabel" in k or "k_hommola_blocks" in k}
    assert len(mine) == 4, sorted(mine)      # (relabel: one wave, 256 lanes, 1024 lanes; blocks)
    for k, v in mine.items():
        assert v["vgpr"] <= 128 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
