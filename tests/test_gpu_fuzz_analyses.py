"""Seeded sessions of tests/fuzz_analyses.py on the device layer: every kernel form of the set passes, Mantel, clade
matching, Kendall and the keyed permutation against the host restatement on the same arguments, records by bytes and
integers with ==, with universes up to 8,300 (16,384 where no matrix is held), chunk values, ranges and the form-switching
environment variables drawn together.  Each session asserts the census of what it reached (fuzz_analyses.REQUIRED); the
seeds were chosen on the CPU so that it holds.  By hand, longer: python tests/fuzz_analyses.py null 2000 1 device"""
import pytest

import fuzz_analyses

pytestmark = pytest.mark.gpu

CASES = 48
SEEDS = {"dispersion": (1, 2), "beta": (1, 2), "unifrac": (1, 2), "null": (1, 2), "mantel": (1, 2), "clade": (1, 2), "kendall": (1, 2),
         "permutation": (1, 2)}


@pytest.mark.parametrize("family,seed", [(f, s) for f in fuzz_analyses.FAMILIES for s in SEEDS[f]])
def test_kernels_against_the_host_restatement(family, seed, monkeypatch):
    setenv = lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)      # noqa: E731
    reached = fuzz_analyses.run(family, seed, CASES, "device", setenv)
    print("%s seed %d: %d cases; %s" % (family, seed, CASES, dict(sorted(reached.items()))))
