"""Resources of k_canopy_ilp_heap (CPU: hipcc's resource-usage remarks of the gfx950 code object): a 1024-lane workgroup needs
at most 128 VGPRs, and the kernel must keep nothing in scratch memory -- its line values are picked out of 16-byte loads by
selects, and a select chain over the components of one vector has been turned into an extract at a variable index before,
which lives in scratch: 2.8 ms per 1e8 pairs became 4.9."""
import os

import pytest

from kernel_resources import HIPCC, resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_heap_kernel_keeps_its_registers_and_uses_no_scratch():
    # (the part of launch_canopy.hip that holds the explicit pair sources: the only ones the kernel is instantiated for)
    res = resources("launch_canopy.hip", ("-DST_CANOPY_PART=0",))
    heap = {k: v for k, v in res.items() if "k_canopy_ilp_heap" in k}
    assert len(heap) == 2, sorted(heap)      # (SrcContig and SrcContig32)
    for k, v in heap.items():
        assert v["vgpr"] <= 128 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
