"""Resources of k_canopy_ilp_codes (CPU: hipcc's resource-usage remarks of the gfx950 code object of launch_canopy_codes.hip):
a 1024-lane workgroup needs at most 128 VGPRs, and the kernel must keep nothing in scratch memory -- its 20-bit fields are cut
out of the loaded dwords by funnel shifts on fixed register pairs and selects, and a dword picked at a variable position would
live in scratch.  The kernel has a unit of its own so that part 0 of launch_canopy.hip stays what it was: still exactly the two
instantiations of k_canopy_ilp_heap there, and none of the new kernel."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _resources(tmp_path, source, extra=()):
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *extra,
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "unit.o"), os.path.join(ROOT, "suchtree_amd", "csrc", source)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key, pattern in (("vgpr", r"\bVGPRs: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                             ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pattern, line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_codes_kernel_keeps_its_registers_and_uses_no_scratch(tmp_path):
    res = _resources(tmp_path, "launch_canopy_codes.hip")
    codes = {k: v for k, v in res.items() if "k_canopy_ilp_codes" in k}
    assert len(codes) == 2 and len(res) == 2, sorted(res)      # (SrcContig and SrcContig32, and nothing else in the unit)
    for k, v in codes.items():
        assert "k_canopy_ilp" in k and "k_canopy_ilp_heap" not in k, k
        assert v["vgpr"] <= 128 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_part_0_of_the_canopy_unit_still_holds_the_two_heap_line_kernels(tmp_path):
    res = _resources(tmp_path, "launch_canopy.hip", ("-DST_CANOPY_PART=0",))
    heap = {k: v for k, v in res.items() if "k_canopy_ilp_heap" in k}
    assert len(heap) == 2, sorted(heap)
    assert not [k for k in res if "k_canopy_ilp_codes" in k]
    for k, v in heap.items():
        assert v["vgpr"] <= 128 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
