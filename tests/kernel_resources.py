"""hipcc's resource-usage remarks of a gfx950 code object, for the test_*resources*.py files: one compile per
(unit, flags) and process, one parser."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

_FIELDS = (("vgpr", r"\bVGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
           ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
           ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"))


@functools.lru_cache(maxsize=None)
def resources(unit, flags=()):
    """{mangled kernel name: {vgpr, sgpr, vgpr_spill, sgpr_spill, scratch, lds, occupancy}} of suchtree_amd/csrc/<unit>,
    compiled for the device with the product's flags and `flags` (a tuple).  The dictionary is shared: read it only."""
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *flags,
                              "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                              "-o", os.path.join(tmp, "unit.o"), os.path.join(ROOT, "suchtree_amd", "csrc", unit)],
                             capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key, pattern in _FIELDS:
            m = re.search(pattern, line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    return res
