"""Seeded sessions of tests/fuzz_compare.py on the device layer: the two-tree compare entries -- moments and histogram, the
exact rank sums, the exact Kendall counts, the row reduction, quartets, every clade at once, Hommola's test for every clade
-- on drawn trees, numberings, special lengths, strategies,
handle options, pair inputs, ranges and chunk values together, against the float64 and integer references on the per-pair
distances of the same two handles.  Each session asserts the census of what it reached (fuzz_compare.REQUIRED); the seeds
were chosen on the CPU so that it holds.  By hand, longer: python tests/fuzz_compare.py ranks 2000 1 device"""
import pytest

import fuzz_compare

pytestmark = pytest.mark.gpu

CASES = 48
SEEDS = {"moments": (1, 2), "ranks": (1, 2), "kendall2": (3, 5), "rows": (1, 2), "quartets": (1, 2), "clades": (1, 2), "hommola": (1, 2), "linked": (1, 2)}


@pytest.mark.parametrize("family,seed", [(f, s) for f in SEEDS for s in SEEDS[f]])
def test_compare_entries_against_the_references(family, seed):
    reached = fuzz_compare.run(family, seed, CASES, "device")
    print("%s seed %d: %d cases; %s" % (family, seed, CASES, dict(sorted(reached.items()))))
