"""Resources of the tree-set kernel (CPU: hipcc's resource-usage remarks of the gfx950 code object): k_rf_tasks keeps
nothing in scratch memory, spills no register, has no static LDS -- the two int32 where the waves meet, the sparse table
and q are all in the dynamic region -- and its largest dynamic request, rf_lds_bytes at the cap of 16384 leaves, fits
the 160 KiB of a CU (it is 42,000 bytes: three workgroups a CU at the cap)."""
import os
import re

import pytest

from conftest import ROOT
from kernel_resources import HIPCC, resources

KERNELS = ("k_rf_tasks",)
LDS_BYTES = 160 * 1024


def _lds_bytes(m):
    """rf_lds_bytes of rf_plan.h, written out once more"""
    nb = (m + 63) >> 6
    stride, levels = (nb + 7) & ~7, nb.bit_length()
    return 16 + 2 * levels * stride * 2 + ((m + 7) & ~7) * 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_rf_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_rf_" in k}
    assert len(mine) == len(KERNELS), sorted(mine)
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    cap = int(re.search(r"#define ST_RF_MAX_LEAVES (\d+)", header).group(1))
    assert cap == 16384 and _lds_bytes(cap) == 42000 and _lds_bytes(4) == 64
    for kernel in KERNELS:
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["lds"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)
        assert v["lds"] + _lds_bytes(cap) <= LDS_BYTES, (k, v)
    # the kernel's name is in no other family's filter
    for k in mine:
        assert not any(s in k for s in ("k_clade_match", "k_rank_", "k_pair", "k_class", "k_group_", "k_swap", "k_linkage", "k_mantel", "k_parafit",
                                        "k_unifrac", "k_setpair", "k_dispersion", "k_kendall_", "k_quartet", "k_hommola", "k_canopy", "k_mrca_ranks")), k
