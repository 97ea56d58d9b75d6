"""scripts/l2_lru_model.py: the LRU model of one XCD's L2 behind the streaming hint (LAB_NOTES.md 9), at a scaled-down
size -- the model depends on the ratio of table and cache only."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("l2_lru_model", os.path.join(ROOT, "scripts", "l2_lru_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_uniform_reads_hit_cache_over_table(model):
    """No streams: C / T = 0.50, as a bypass and as streams of no bytes."""
    for kw in ({"bypass": True}, {"stream_in": 0.0, "stream_out": 0.0}):
        r = model.simulate(4096, 2048, pairs=100_000, **kw)
        assert abs(r["line_hit_rate"] - 0.50) <= 0.01, r


def test_headline_streams_cost_six_points(model):
    """16 B of pairs in and 12 B of results out per pair, allocating: 0.437, i.e. 1.251 fabric reads per pair."""
    r = model.simulate(4096, 2048, stream_in=16.0, stream_out=12.0, pairs=100_000)
    assert abs(r["line_hit_rate"] - 0.437) <= 0.01, r
    assert abs(r["fabric_reads_per_pair"] - (2 * (1 - r["line_hit_rate"]) + 0.125)) < 1e-12


def test_resident_table_and_cli(model, capsys):
    """A table the size of the cache stays resident only when the streams bypass it; the command line prints both."""
    rows = model.main(["--table-bytes", str(4 << 20), "--scale", "32", "--pairs", "50000"])
    assert [r["streams_allocate"] for r in rows] == [True, False]
    assert abs(rows[0]["line_hit_rate"] - 0.815) <= 0.01 and rows[1]["line_hit_rate"] > 0.9999, rows      # (a cold miss or two after the warm-up)
    assert "bypass L2" in capsys.readouterr().out
