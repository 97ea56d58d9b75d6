"""Seeded fuzz of st_group_sums_codes on the device (tests/fuzz_group_tests.py draws the cases, whose host sums
tests/test_fuzz_group_tests_host.py checks against the definition): the kernels, under each case's chunk and slice,
give the bytes of the host restatement."""
import pytest

import fuzz_group_tests as fuzz

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(fuzz.N_CASES))
def test_device_equals_host(k, monkeypatch):
    c = fuzz.case(k)
    assert fuzz.run(c, 0, monkeypatch).tobytes() == fuzz.run(c, -1, monkeypatch, plain=True).tobytes()
