"""bench.py prints exactly one JSON line with the contract's fields (small batch, GPU box)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_bench_line_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                          "--pairs", "4000000", "--cpu-seconds", "1", "--full"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "pairs/s" and d["scaling"] == "strong" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    # HBM is the bound; the primary figure is what the kernel moves (counter bytes of the committed PMC
    # passes x this run's kernel rate), the algorithmic 28 + 8h bytes ride along flagged as exceeding the peak, the
    # fabric's random-sector rate (measured in this process at the kernel's footprint) is the secondary ceiling
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] < 1, r
    assert r["traffic"] and abs(r["achieved"] - r["traffic_bytes_per_pair"] * r["pairs_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["traffic_source"].startswith("profiles/traffic_r") and r["rocprof"]["kernel_avg_ms"] > 0 and 0 < r["rocprof"]["frac"] < 1
    a = r["algorithmic"]
    assert a["bytes_per_pair"] > 300 and abs(a["frac_of_hbm_peak"] - a["GBps"] / 8000.0) < 1e-12 and a["exceeds_peak"] == (a["frac_of_hbm_peak"] > 1)
    assert r["algorithmic_bytes_per_pair"] == a["bytes_per_pair"] and r["algorithmic_frac_of_hbm_peak"] == a["frac_of_hbm_peak"]
    sc = r["secondary_ceiling"]
    assert sc["name"] == "fabric_random_sector" and sc["unit"] == "Greads/s" and 30 < sc["peak"] < 400
    assert abs(sc["frac"] - sc["achieved"] / sc["peak"]) < 1e-12 and 0 < sc["frac"] <= 1.02 and r["request_rate"]["frac"] == sc["frac"]
    assert 0 < r["counter_traffic"]["frac_of_hbm_peak"] < 1
    assert abs(sc["gather_footprint_MiB"] - d["hardware_measured"]["table"]["MiB"]) < 1e-6
    assert [t["leaves"] for t in r["hbm_regime"]["trees"]] == [1 << 20, 1 << 22, 1 << 24]
    assert not r["hbm_regime"]["trees"][2]["fits_infinity_cache"] and 0 < r["hbm_regime"]["trees"][2]["frac_of_hbm_peak"] < 1
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "pairs/s" and c["sample"]
    assert d["parity"]["distances_bit_exact"] and d["parity"]["mrca_bit_exact"]
    assert d["end_to_end_host_path"]["matches_device_results"]
    assert d["value"] > 1e9
    assert r["required_bytes_per_pair"] == 156 and 0 < r["required_frac"] < 1
    assert d["hardware_measured"]["table"]["Greads_per_s"] > 1 and d["hardware_measured"]["stream_copy_GBps"] > 100
    e = d["end_to_end_host_path"]
    assert e["pairs_per_s"] > 1e8 and e["pairs_per_s_fresh_arrays"] > 1e8 and e["pairs_per_s_call_and_drop_loop"] > 1e8
    assert e["cpu_passes_pairs_per_s"] > e["pairs_per_s"] * 0.5 and e["link_side_pairs_per_s"] > e["pairs_per_s"] * 0.5
    assert e["link_bytes_per_pair"] == {"in": 6, "out": 7} and e["one_process_many_gpus_ceiling"]["x_one_gpu"] > 0.5
    assert d["mrca_ids_only"]["matches_the_fused_launch"] and d["mrca_ids_only"]["ids_per_s"] > 1e9
    # ceilings are the best of a sweep of launch shapes, and the shape is reported
    hw = d["hardware_measured"]
    assert hw["table"]["shapes_swept"] >= 9 and hw["table"]["best_shape"]["unroll"] in (4, 8, 16)
    assert hw["stream_copy_shapes_swept"] >= 8 and hw["stream_copy_GBps"] > 3000
    # the other BASELINE configs ride in the same line (driver-observed numbers for configs 2, 4, 5)
    oc = d["other_configs"]
    for key in ("config2_ml_tree", "config2_nj_tree", "config4_triangle_100k", "config5_fish_worm"):
        assert "error" not in oc[key], oc[key]
    for key in ("config2_ml_tree", "config2_nj_tree"):
        c = oc[key]
        assert c["default"]["bit_exact_on_sample"] and c["walk"]["bit_exact_on_sample"] and c["host_path"]["bit_exact_on_sample"]
        assert c["default"]["pairs_per_s"] > 1e9 and c["walk"]["pairs_per_s"] > 1e9 and c["algorithmic_bytes_per_pair"] > 500
    # every leg is measured to the headline's standard (round 6): the CPU column -- the oracle on the leg's own pairs, one thread
    # and all host cores -- and a roofline block whose frac is counter bytes / kernel time / 8 TB/s wherever a committed PMC summary
    # of THIS kernel at THIS batch size exists (SURVEY 8d's algorithmic bytes ride along, flagged where they exceed the peak)
    def leg_blocks(where, cpu, roofs):
        assert cpu["kind"] in ("port", "reference") and cpu["unit"] == "pairs/s" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"], (where, cpu)
        for r in roofs:
            assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12, (where, r)
            a = r["algorithmic"]
            assert a["exceeds_peak"] == (a["frac_of_hbm_peak"] > 1) and a["why"], (where, a)
            if r["traffic"] is not None:
                assert 0 < r["frac"] < 1 and r["traffic_source"].startswith("profiles/traffic_") and r["counters_kernel"], (where, r)
                assert abs(r["traffic"] - r["traffic_bytes_per_pair"] * r["pairs_per_launch"]) < 1e-6 * r["traffic"], (where, r)
    for key in ("config2_ml_tree", "config2_nj_tree"):
        c = oc[key]
        assert c["cpu_baseline"]["single_thread_value"] > 0 and c["default"]["x_cpu_all_cores"] > 10 and c["default"]["x_cpu_one_thread"] > 100, c
        leg_blocks(key, c["cpu_baseline"], [c["default"]["roofline"], c["walk"]["roofline"]])
        assert c["default"]["roofline"]["traffic"] is not None, c["default"]["roofline"]      # (the round's profiles cover the kernel the handle picks)
    t = oc["config4_triangle_100k"]
    leg_blocks("config4", t["cpu_baseline"], [t["canopy"]["roofline"], t["walk"]["roofline"]])
    for key in ("walk_only_tree", "deep_long_record_tree"):
        leg_blocks(key, oc[key]["cpu_baseline"], [oc[key]["roofline"]])
    leg_blocks("config5", oc["config5_fish_worm"]["cpu_baseline"], [])
    assert t["pairs"] == 4_999_950_000 and t["bit_exact_on_sample"] and t["canopy"]["pairs_per_s"] > 1e10
    assert t["streamed_to_host"]["pairs"] == 1 << 30 and t["streamed_to_host"]["pairs_per_s"] > 1e9
    for key in ("walk_only_tree", "deep_long_record_tree"):
        assert "error" not in oc[key], oc[key]
        assert oc[key]["bit_exact_on_sample"] and oc[key]["pairs_per_s"] > 1e9, oc[key]
    # the tree beyond 512-byte records: 1 KB records read by the scalar ladder kernel, the walk family timed beside it
    w = oc["walk_only_tree"]
    assert w["record_bytes"] == 1024 and w["kernel"] == "canopy_ladder" and w["walk"]["bit_exact_on_sample"] and w["walk"]["pairs_per_s"] > 1e9, w
    assert oc["deep_long_record_tree"]["record_bytes"] == 512
    f = oc["config5_fish_worm"]
    assert f["distances_bit_exact"] and f["laplacian_bit_exact"] and f["pairs"] == 2 * 18145 and f["laplacian_shape"] == [422, 422]


def test_bench_under_torchrun_one_rank():
    """The N > 1 code path (process group, sharded step, barriers) with world size 1 -- all a
    1-GPU box can run of it; the slicing / gather itself is covered by the gloo tests."""
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
                          "--gpus", "1", "--steps", "2", "--warmup", "1", "--pairs", "2000000", "--cpu-seconds", "1",
                          "--no-host-path", "--no-microbench", "--no-other-configs", "--full"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["value"] > 1e8
    # the CPU baseline and the parity block are produced under the process group too (every N)
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] in ("port", "reference")
    assert d["parity"]["distances_bit_exact"] and d["parity"]["mrca_bit_exact"]


def test_plain_bench_run_and_dumped_outputs(tmp_path):
    """Without --full: the headline fields only, and --dump-outputs holds the last timed step's results at a seeded
    sample of positions (the batch is larger than DUMP_PAIRS), bit for bit what the oracle computes for those pairs."""
    import numpy as np
    from oracle.oracle import OracleTree
    from suchtree_amd import synth
    import bench
    n, out_dir = 4_000_000, tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--pairs", str(n),
                          "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["ms_per_step"] - n / d["value"] * 1e3) < 1e-6 * d["ms_per_step"] and d["value"] > 1e9
    for key in ("cpu_baseline", "parity", "hardware_measured", "end_to_end_host_path", "mrca_ids_only", "other_configs"):
        assert key not in d, key
    idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, n, bench.DUMP_PAIRS))
    pairs = synth.random_leaf_pairs(1 << 20, n, seed=3)[idx]
    dd, mm = np.load(out_dir / "distances.npy"), np.load(out_dir / "mrca_ids.npy")
    assert dd.dtype == mm.dtype == np.float64 and len(dd) == len(mm) == len(idx)
    parent, dist = synth.balanced_tree(20)
    O = OracleTree(parent, dist)
    assert np.array_equal(dd.view(np.int64), O.distances_mt(pairs, 16).view(np.int64)) and np.array_equal(mm, O.mrca_bulk(pairs))
