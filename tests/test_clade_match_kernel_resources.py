"""Resources of the clade matching kernel (CPU: hipcc's resource-usage remarks of the gfx950 code object): k_clade_match
keeps nothing in scratch memory, spills no register and declares no static LDS (its bitmap, counts and the words in which
the waves meet are all in the dynamic region, whose base is then 16-byte aligned).  The VGPR count is the one DESIGN.md
section 20 records."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

VGPRS = {"k_clade_match": 58}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_clade_match_kernel_uses_no_scratch_and_spills_nothing(tmp_path):
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "unit.o"), os.path.join(ROOT, "suchtree_amd", "csrc", "suchtree_hip.hip")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key, pattern in (("vgpr", r"\bVGPRs: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                             ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                             ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pattern, line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    mine = {k: v for k, v in res.items() if "k_clade_match" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0 and v["lds"] == 0, (k, v)
        assert v["vgpr"] == vgprs and v["occupancy"] == 8, (k, v)
