"""Seeded sessions of tests/fuzz_analyses.py on the host layer (no GPU): the library's host forms -- the restatements that
the GPU tests take as their yardstick -- against the independent references under tests/, at random small sizes, with set
sizes, ranges, chunk values, permutations and options drawn together.  Integers are compared with ==, float records within
the bounds the contract states; each session asserts the census of what it reached (fuzz_analyses.REQUIRED).
By hand, longer: python tests/fuzz_analyses.py dispersion 100000 1 host"""
import pytest

import fuzz_analyses
from suchtree_amd import build as st_build

CASES = 1500
SEEDS = {"dispersion": (1, 2), "beta": (1, 2), "unifrac": (1, 2), "null": (1, 2), "mantel": (1, 2), "clade": (1, 2), "kendall": (1, 2),
         "permutation": (1, 2)}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    st_build.build()


@pytest.mark.parametrize("family,seed", [(f, s) for f in fuzz_analyses.FAMILIES for s in SEEDS[f]])
def test_host_forms_against_the_references(family, seed, monkeypatch):
    setenv = lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)      # noqa: E731
    reached = fuzz_analyses.run(family, seed, CASES, "host", setenv)
    print("%s seed %d: %d cases; %s" % (family, seed, CASES, dict(sorted(reached.items()))))


@pytest.mark.parametrize("family", fuzz_analyses.FAMILIES)
def test_census_of_the_device_sessions_holds(family):
    """The sessions of tests/test_gpu_fuzz_analyses.py reach what they must: the census needs the draws alone, so a
    generator edited here fails here, before a GPU sees it."""
    import test_gpu_fuzz_analyses as gpu
    for seed in gpu.SEEDS[family]:
        assert fuzz_analyses.missing(family, fuzz_analyses.census(family, seed, gpu.CASES, "device"), "device") == [], seed
