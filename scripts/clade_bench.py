"""Measure SuchLinkedTrees.linked_distances_by_clade at the scale of the reference's per-clade notebook loop and print
one JSON line.  Seeded synthetic system: TreeB = synth.random_binary_tree(100_000), TreeA = a balanced tree of 256
leaves, one or two links per TreeB leaf.

  capped / uncapped / root_summary   best and median wall time of >= 5 runs after a warm-up: the notebook's filters
                                     (min_leaves=10, min_links=10, max_links=2500), no cap, and linked_distances_summary()
                                     at the root (the same pairs as the uncapped run); pairs evaluated, pairs/s, clades/s
  ratio_uncapped_vs_root             uncapped pairs/s over root_summary pairs/s
  loop                               subset_b + linked_distances_summary on 200 seeded clades, extrapolated to all
  kernels                            from a second run under `rocprofv3 --kernel-trace --stats`: summed kernel time of
                                     the distance kernels and of k_clade_pieces in one uncapped call

    python scripts/clade_bench.py [--reps 5] [--no-profile]
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


def system():
    import pandas as pd
    from suchtree_amd import SuchTree, synth
    from suchtree_amd.linked import SuchLinkedTrees
    pa, da = synth.balanced_tree(8)
    pb, db = synth.random_binary_tree(100_000, seed=1)
    A = SuchTree((pa, da, ["a%d" % i for i in range(256)]))
    B = SuchTree((pb, db, ["b%d" % i for i in range(100_000)]))
    rng = np.random.default_rng(2)
    mat = np.zeros((256, 100_000), dtype=np.uint8)
    mat[rng.integers(0, 256, 100_000), np.arange(100_000)] = 1
    second = rng.random(100_000) < 0.5
    mat[rng.integers(0, 256, int(second.sum())), np.flatnonzero(second)] = 1
    df = pd.DataFrame(mat.astype(bool), index=list(A.leaves), columns=list(B.leaves))
    S = SuchLinkedTrees(A.to_device(), B.to_device(), df)
    return S


def timed(fn, reps):
    fn()
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, min(ts), float(np.median(ts))


def run(reps):
    S = system()
    L = S.subset_n_links
    all_pairs = L * (L - 1) // 2
    res = {"n_links": L, "reps": reps}
    n_internal = len(S.TreeB.get_internal_nodes())
    # pairs evaluated with a cap: the segments of the nodes within it
    from suchtree_amd import _capi
    B = S.TreeB
    col_of = np.full(B.size, -1, dtype=np.int64)
    col_of[S._col_ids] = np.arange(len(S._col_ids))
    _, ids_b = S._links_in_order(col_of[S._leaf_order(B, B.root_node)], S._subset_a_leafs)
    capped_pairs = _capi.clade_plan(B._flat.parent, ids_b, max_links=2500)["total_pairs"]
    for key, kw, pairs in (("capped", dict(min_leaves=10, min_links=10, max_links=2500), capped_pairs),
                           ("uncapped", dict(), all_pairs)):
        C, best, med = timed(lambda: S.linked_distances_by_clade(**kw), reps)
        res[key] = {"best_s": best, "median_s": med, "pairs": pairs, "rows": len(C), "pairs_per_s": pairs / best,
                    "clades_per_s": n_internal / best}
    s, best, med = timed(lambda: S.linked_distances_summary(), reps)
    res["root_summary"] = {"best_s": best, "median_s": med, "pairs": all_pairs, "pairs_per_s": all_pairs / best,
                           "pearson_r": s.pearson_r}
    res["ratio_uncapped_vs_root"] = res["uncapped"]["pairs_per_s"] / res["root_summary"]["pairs_per_s"]
    # the loop of the notebook on 200 seeded clades
    nodes = np.random.default_rng(3).choice(B.get_internal_nodes(), 200, replace=False)
    R = S
    t0 = time.perf_counter()
    for v in nodes:
        R.subset_b(int(v))
        if R.subset_n_links >= 2:
            R.linked_distances_summary()
    t = time.perf_counter() - t0
    R.subset_b(B.root_node)
    res["loop"] = {"clades": 200, "s": t, "extrapolated_all_s": t / 200 * n_internal,
                   "speedup_vs_uncapped": t / 200 * n_internal / res["uncapped"]["best_s"]}
    return res


def profile():
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="clade_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "cl", "--", sys.executable,
               os.path.abspath(__file__), "--child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        sums = {}
        for r in csv.DictReader(open(traces[0])):
            name = r["Kernel_Name"]
            kind = ("k_clade_pieces" if "k_clade_pieces" in name else "distance" if ("k_canopy" in name or "k_walk" in name)
                    else "k_pair_moments" if "k_pair_moments" in name else "other")
            sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        tot = sum(sums.values())
        return {"ns": sums, "clade_reduction_share": sums.get("k_clade_pieces", 0) / tot if tot else None,
                "note": "one uncapped by-clade call and one root linked_distances_summary()"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        S = system()
        S.linked_distances_by_clade()
        S.linked_distances_summary()
        return
    res = run(max(a.reps, 5))
    res["kernels"] = None if a.no_profile else profile()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
