"""Resources of the UniFrac kernels (CPU: hipcc's resource-usage remarks of the gfx950 code object): the table and widen
kernels and the two pair forms (one pair per lane, one pair per wave) keep nothing in scratch memory and spill no
register.  The VGPR counts are those DESIGN.md section 19 records."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

VGPRS = {"k_unifrac_table": 10, "k_unifrac_widen": 6, "k_unifrac_lane": 26, "k_unifrac_wave": 32}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_unifrac_kernels_use_no_scratch_and_spill_nothing(tmp_path):
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
                             ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pattern, line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    mine = {k: v for k, v in res.items() if "k_unifrac" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
