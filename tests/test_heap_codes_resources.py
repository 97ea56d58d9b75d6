"""Resources of k_canopy_ilp_codes (CPU: hipcc's resource-usage remarks of the gfx950 code object of launch_canopy_codes.hip):
a 1024-lane workgroup needs at most 128 VGPRs, and the kernel must keep nothing in scratch memory -- its 20-bit fields are cut
out of the loaded dwords by funnel shifts on fixed register pairs and selects, and a dword picked at a variable position would
live in scratch.  The kernel has a unit of its own so that part 0 of launch_canopy.hip stays what it was: still exactly the two
instantiations of k_canopy_ilp_heap there, and none of the new kernel."""
import os

import pytest

from kernel_resources import HIPCC, resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_codes_kernel_keeps_its_registers_and_uses_no_scratch():
    res = resources("launch_canopy_codes.hip")
    codes = {k: v for k, v in res.items() if "k_canopy_ilp_codes" in k}
    assert len(codes) == 2 and len(res) == 2, sorted(res)      # (SrcContig and SrcContig32, and nothing else in the unit)
    for k, v in codes.items():
        assert "k_canopy_ilp" in k and "k_canopy_ilp_heap" not in k, k
        assert v["vgpr"] <= 128 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_part_0_of_the_canopy_unit_still_holds_the_two_heap_line_kernels():
    res = resources("launch_canopy.hip", ("-DST_CANOPY_PART=0",))
    heap = {k: v for k, v in res.items() if "k_canopy_ilp_heap" in k}
    assert len(heap) == 2, sorted(heap)
    assert not [k for k in res if "k_canopy_ilp_codes" in k]
    for k, v in heap.items():
        assert v["vgpr"] <= 128 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
