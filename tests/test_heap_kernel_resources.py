"""Resources of k_canopy_ilp_heap (CPU: hipcc's resource-usage remarks of the gfx950 code object): a 1024-lane workgroup needs
at most 128 VGPRs, and the kernel must keep nothing in scratch memory -- its line values are picked out of 16-byte loads by
selects, and a select chain over the components of one vector has been turned into an extract at a variable index before,
which lives in scratch: 2.8 ms per 1e8 pairs became 4.9."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_heap_kernel_keeps_its_registers_and_uses_no_scratch(tmp_path):
    # (the part of launch_canopy.hip that holds the explicit pair sources: the only ones the kernel is instantiated for)
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-DST_CANOPY_PART=0",
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "unit.o"), os.path.join(ROOT, "suchtree_amd", "csrc", "launch_canopy.hip")],
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
    heap = {k: v for k, v in res.items() if "k_canopy_ilp_heap" in k}
    assert len(heap) == 2, sorted(heap)      # (SrcContig and SrcContig32)
    for k, v in heap.items():
        assert v["vgpr"] <= 128 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
