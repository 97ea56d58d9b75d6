"""The host side of the per-clade Hommola test (no GPU): st_hommola_permutation on the host against the numpy
restatement of its definition (tests/hommola_clade_reference.py), the uniformity of the permutations, their prefix
property and independence, and -- in a stand-alone program under AddressSanitizer + UBSan -- the plan (laminar check,
maximal ranges, block tables, chunk cuts), the fold of pieces and every argument error."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import hommola_clade_reference as ref
from suchtree_amd import _capi, compare

SIZES = (1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 16383, 16384)
KEYS = ((0, 0, 1, 0), (0, 0, 1, 1), (2024, 7, 1, 0), (2024, 7, 999, 1), ((1 << 64) - 1, 123456, 3, 0), ((1 << 64) - 1, 2 ** 31 - 2, 2 ** 40, 1))


@pytest.mark.parametrize("n", SIZES)
def test_host_permutation_equals_the_restatement(n):
    for seed, node, p, side in KEYS:
        got = compare.hommola_permutation(seed, node, p, side, n)
        assert got.dtype == np.int32 and got.shape == (n,)
        assert np.array_equal(np.sort(got), np.arange(n)), (seed, node, p, side)
        assert np.array_equal(got, ref.permutation(seed, node, p, side, n)), (seed, node, p, side)
    assert np.array_equal(compare.hommola_permutation(5, 3, 0, 1, n), np.arange(n))      # p = 0: the identity


def test_permutation_argument_errors():
    assert _capi.HOMMOLA_MAX_UNIVERSE == 16384
    for n in (0, 16385, -1):
        with pytest.raises(ValueError):
            compare.hommola_permutation(1, 1, 1, 0, n)
    for kw in ({"p": -1}, {"side": 2}, {"side": -1}, {"node": -1}):
        with pytest.raises(ValueError):
            compare.hommola_permutation(**{"seed": 1, "node": 1, "p": 1, "side": 0, "n": 4, **kw})


@pytest.mark.parametrize("seed, node, side", [(2024, 7, 0), (2024, 7, 1), (0, 0, 0)])
def test_permutations_of_four_are_uniform(seed, node, side):
    """The 24 permutations of n = 4 over p = 1..24000: chi-squared below 49.73, the 0.999 quantile at 23 degrees of freedom
    (the restatement gave 17.8, 19.9 and 25.1 for these three streams)."""
    index = {perm: i for i, perm in enumerate(itertools.permutations(range(4)))}
    counts = np.zeros(24)
    for p in range(1, 24001):
        counts[index[tuple(int(v) for v in compare.hommola_permutation(seed, node, p, side, 4))]] += 1
    chi2 = float(((counts - 1000.0) ** 2 / 1000.0).sum())
    print("chi2", seed, node, side, chi2)
    assert chi2 < 49.73


def test_prefix_property_and_independence():
    n, seed = 300, 99
    base = compare.hommola_permutation(seed, 11, 5, 0, n)
    assert np.array_equal(base, compare.hommola_permutation(seed, 11, 5, 0, n))      # a function of its arguments alone
    for other in ((seed, 11, 5, 1), (seed, 12, 5, 0), (seed, 11, 6, 0), (seed + 1, 11, 5, 0)):
        assert not np.array_equal(base, compare.hommola_permutation(*other, n)), other
    # the streams of consecutive p and of the two sides do not collide: (2p + s) is distinct for every (p, s)
    seen = {tuple(compare.hommola_permutation(seed, 11, p, s, 8)) for p in range(1, 200) for s in (0, 1)}
    assert len(seen) > 390


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_hommola_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_hommola")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_hommola.cpp"), os.path.join(csrc, "hommola_plan.cpp"),
                           os.path.join(csrc, "compare_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize hommola ok" in out.stdout


def test_facade_errors_raised_before_any_upload():
    """hommola_by_clade checks its arguments before either tree goes to a device."""
    import pandas as pd
    from suchtree_amd import SuchLinkedTrees, SuchTree, synth
    ta = SuchTree(synth.random_binary_tree(6, seed=1) + (["a%d" % i for i in range(6)],))
    tb = SuchTree(synth.random_binary_tree(9, seed=2) + (["b%d" % i for i in range(9)],))
    links = pd.DataFrame(np.eye(6, 9, dtype=int), index=list(ta.leaves.keys()), columns=list(tb.leaves.keys()))
    slt = SuchLinkedTrees(ta, tb, links)
    for kw in ({"tree": "C"}, {"permutations": -1}, {"permutations": 2.5}, {"permutations": True}, {"max_leaves": 16385}, {"seed": -1},
               {"seed": 1 << 64}):
        with pytest.raises(ValueError):
            slt.hommola_by_clade(**kw)
    assert ta._dev_tree is None and tb._dev_tree is None
