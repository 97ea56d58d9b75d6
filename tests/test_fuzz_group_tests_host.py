"""Seeded fuzz of st_group_sums_codes without a GPU (tests/fuzz_group_tests.py draws the cases): the host restatement,
under each case's chunk and slice, equals the pair loop of tests/group_reference.py."""
import pytest

import fuzz_group_tests as fuzz
import group_reference as ref


@pytest.mark.parametrize("k", range(fuzz.N_CASES))
def test_host_equals_the_reference(k, monkeypatch):
    c = fuzz.case(k)
    got = fuzz.run(c, -1, monkeypatch)
    assert got.tolist() == ref.group_sums(c["y"], c["group"], c["n_groups"], c["permutations"], c["seed"], c["stream"])
    assert got.tobytes() == fuzz.run(c, -1, monkeypatch, plain=True).tobytes()
