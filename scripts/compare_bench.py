"""Measure the compare path (SuchTree.compare_distances) on all pairs of ml.tree vs nj.tree (54,327 shared taxa,
1,475,684,301 pairs) and print one JSON line:

  moments_s / moments_pairs_per_s     moments only (one pass)
  hist64_s / hist64_pairs_per_s       moments + a 64 x 64 histogram with given edges (one pass)
  kernels                             from a second run of this script under `rocprofv3 --kernel-trace --stats`:
                                      summed kernel time of the two trees' float32 triangle launches and of the reduction
                                      kernels (k_pair_*), each for the moments-only and the histogram pass, and the
                                      reduction's share of the summed kernel time

    python scripts/compare_bench.py [--reps 3] [--no-profile]

Reads the committed fixtures under tests/golden only.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load():
    from suchtree_amd import SuchTree
    g = os.path.join(ROOT, "tests", "golden")
    z1, z2 = np.load(os.path.join(g, "ml_tree.npz")), np.load(os.path.join(g, "nj_tree.npz"))
    nj_of = np.load(os.path.join(g, "ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    T1 = SuchTree((z1["parent"], z1["distance"])).to_device()
    T2 = SuchTree((z2["parent"], z2["distance"])).to_device()
    return T1._device_tree(), T2._device_tree(), z1["leaf_ids"].astype(np.int64), nj_of


def run(reps):
    from suchtree_amd.compare import histogram_edges
    dx, dy, ids_x, ids_y = load()
    n = len(ids_x) * (len(ids_x) - 1) // 2
    dx.compare_triangle_host(dy, ids_x[:3000], ids_y[:3000])          # warm-up (kernels loaded, pipes built)
    best_m, m = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        m, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
        t = time.perf_counter() - t0
        best_m = t if best_m is None else min(best_m, t)
    edges = histogram_edges(64, None, (m.min_x, m.max_x, m.min_y, m.max_y))
    best_h, h = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        _, h = dx.compare_triangle_host(dy, ids_x, ids_y, edges=edges)
        t = time.perf_counter() - t0
        best_h = t if best_h is None else min(best_h, t)
    from suchtree_amd.compare import DistanceComparison
    r = DistanceComparison.from_moments(m).pearson_r
    return {"pairs": n, "pearson_r": r, "hist_total": int(h.sum()), "moments_s": best_m, "moments_pairs_per_s": n / best_m,
            "hist64_s": best_h, "hist64_pairs_per_s": n / best_h, "reps": reps}


def profile():
    """Run this script once more (one rep) under rocprofv3 and sum the kernel time by kind."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="compare_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "cmp", "--", sys.executable,
               os.path.abspath(__file__), "--child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written", "files": sorted(os.path.relpath(f, out) for f in
                                                                   glob.glob(os.path.join(out, "**", "*"), recursive=True))[:20]}
        rows = list(csv.DictReader(open(traces[0])))
        # the child's phases are told apart by the reduction kernel each uses: moments-only or histogram form
        phases = {"moments": {"triangle_ns": 0, "reduction_ns": 0}, "hist64": {"triangle_ns": 0, "reduction_ns": 0}}
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        pending = 0
        for r in rows:
            name, ns = r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            if "k_pair_moments<true>" in name or "k_pair_momentsILb1E" in name:
                phases["hist64"]["reduction_ns"] += ns
                phases["hist64"]["triangle_ns"] += pending
                pending = 0
            elif "k_pair_moments<false>" in name or "k_pair_momentsILb0E" in name:
                phases["moments"]["reduction_ns"] += ns
                phases["moments"]["triangle_ns"] += pending
                pending = 0
            elif "k_pair_shift" in name or "k_pair_moments_final" in name:
                pass      # (a few microseconds per call)
            elif "k_canopy" in name or "k_walk" in name:
                pending += ns
        for ph in phases.values():
            tot = ph["triangle_ns"] + ph["reduction_ns"]
            ph["reduction_share"] = ph["reduction_ns"] / tot if tot else None
        return phases
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:       # (under rocprofv3: one rep of each phase, the warm-up's small triangle included)
        run(1)
        return
    res = run(a.reps)
    res["kernels"] = None if a.no_profile else profile()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
