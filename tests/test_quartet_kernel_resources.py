"""Resources of the quartet kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): k_quartet_draw
(both modes) and k_quartet_agree keep nothing in scratch memory -- the draw's sorted positions and the sixteen running
counts are indexed by constants only, so they stay in registers -- and stay at or below 64 VGPRs, so that eight waves
per SIMD hide the latency of their loads."""
import os

import pytest

from kernel_resources import HIPCC, resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_quartet_kernels_use_no_scratch_and_at_most_64_vgprs():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_quartet_draw" in k or "k_quartet_agree" in k}
    assert len(mine) == 3, sorted(mine)      # (draw: ST_QUARTET_ALL and ST_QUARTET_SAMPLE; agree)
    for k, v in mine.items():
        assert v["vgpr"] <= 64 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
