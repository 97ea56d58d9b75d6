"""Measure SuchLinkedTrees.hommola_cospeciation and print one JSON line.  Workloads: gopher_louse (99,999 permutations)
and fish_worm (9,999) from tests/golden, and the seeded system of scripts/clade_bench.py (9 permutations).

Per workload:
  best_s / median_s            wall time of >= 5 runs after a warm-up
  pairs / padding_pairs        pairs evaluated (rows x P) and padding pairs evaluated besides (rows x (S - P))
  pairs_per_s                  pairs over best_s
  draw_share                   time to draw the permutations on the host (compare.hommola_rows alone) over best_s
  summary_pairs_per_s          linked_distances_summary() on the same links; ratio_vs_summary = pairs_per_s over it
  loop                         compare_triangle_host per relabelled row on min(200, permutations) rows, extrapolated
  numpy_s                      (small sets) the numpy restatement of scikit-bio's test on precomputed distance matrices
kernels: from a second run under `rocprofv3 --kernel-trace --stats`, summed kernel time of the distance kernels and of
k_row_blocks in one call per workload (the fold runs on the host, overlapped with the device).

    python scripts/hommola_bench.py [--reps 5] [--no-profile]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

WORKLOADS = (("gopher_louse", 99_999), ("fish_worm", 9_999), ("clade_bench_system", 9))


def system(which):
    import pandas as pd
    from suchtree_amd import SuchTree
    from suchtree_amd.linked import SuchLinkedTrees
    if which == "clade_bench_system":
        import clade_bench
        return clade_bench.system()
    d = os.path.join(ROOT, "tests", "golden", which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]).to_device(), SuchTree(d + "/" + names[1]).to_device(), links)


def universes(S):
    u_a, u_b = np.asarray(S.subset_a_leafs, np.int64), np.asarray(S.subset_b_leafs, np.int64)
    wa = np.full(S.TreeA.size, -1, np.int64)
    wa[u_a] = np.arange(len(u_a))
    wb = np.full(S.TreeB.size, -1, np.int64)
    wb[u_b] = np.arange(len(u_b))
    ll = S.linklist
    return u_a, u_b, wa[ll[:, 1]], wb[ll[:, 0]]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def numpy_restatement(S, permutations, seed):
    """scikit-bio's algorithm in numpy on distance matrices over the universes (the matrices from the GPU, not timed)."""
    u_a, u_b, pos_a, pos_b = universes(S)
    mats = []
    for T, u in ((S.TreeA, u_a), (S.TreeB, u_b)):
        i, j = np.meshgrid(u, u, indexing="ij")
        mats.append(T.distances_bulk(np.stack([i.ravel(), j.ravel()], axis=1)).reshape(len(u), len(u)))
    DA, DB = mats
    rows, cols = np.tril_indices(len(pos_a), -1)
    t0 = time.perf_counter()
    rng = np.random.default_rng(seed)
    r = np.corrcoef(DA[pos_a[cols], pos_a[rows]], DB[pos_b[cols], pos_b[rows]])[0, 1]
    for _ in range(permutations):
        mp = rng.permutation(len(u_b))
        mh = rng.permutation(len(u_a))
        pa, pb = mh[pos_a], mp[pos_b]
        np.corrcoef(DA[pa[cols], pa[rows]], DB[pb[cols], pb[rows]])
    return time.perf_counter() - t0, r


def run_one(which, permutations, reps):
    from suchtree_amd import compare
    S = system(which)
    L = S.subset_n_links
    P = L * (L - 1) // 2
    rows = permutations + 1
    C = 1 << 25
    S_row = P if P <= C // 2 else -(-P // 8192) * 8192
    res = {"n_links": L, "permutations": permutations, "pairs": rows * P, "padding_pairs": rows * (S_row - P)}
    out = {}

    def call():
        out["r"] = S.hommola_cospeciation(permutations, seed=1)

    best, med = timed(call, reps)
    res.update(best_s=best, median_s=med, pairs_per_s=rows * P / best, corr_coeff=out["r"].corr_coeff, p_value=out["r"].p_value)
    u = universes(S)
    t0 = time.perf_counter()
    for _ in compare.hommola_rows(*u, permutations, 1, max(1, (1 << 23) // L)):
        pass
    res["draw_s"] = time.perf_counter() - t0
    res["draw_share"] = res["draw_s"] / best
    sbest, _ = timed(lambda: S.linked_distances_summary(), reps)
    res["summary_pairs_per_s"] = P / sbest
    res["ratio_vs_summary"] = res["pairs_per_s"] / res["summary_pairs_per_s"]
    k = min(200, permutations)
    dev_a, dev_b = S.TreeA._device_tree(), S.TreeB._device_tree()
    gen = compare.hommola_rows(*u, k, 2, max(1, (1 << 23) // L))
    batches = list(gen)
    t0 = time.perf_counter()
    n = 0
    for ids_a, ids_b in batches:
        for i in range(len(ids_a)):
            dev_a.compare_triangle_host(dev_b, ids_a[i], ids_b[i])
            n += 1
    t = time.perf_counter() - t0
    res["loop"] = {"rows": n, "s": t, "extrapolated_s": t / n * rows, "speedup": t / n * rows / best}
    if which != "clade_bench_system":
        ns, r = numpy_restatement(S, permutations, 1)
        res["numpy_s"] = ns
        res["numpy_vs_gpu"] = ns / best
        res["numpy_r_minus_gpu_r"] = r - res["corr_coeff"]
    return res


def profile():
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="hommola_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "hb", "--", sys.executable,
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
            kind = ("k_row_blocks" if "k_row_blocks" in name else "distance" if ("k_canopy" in name or "k_walk" in name)
                    else "other")
            sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        tot = sum(sums.values())
        return {"ns": sums, "row_reduction_share": sums.get("k_row_blocks", 0) / tot if tot else None,
                "note": "one hommola_cospeciation call per workload"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        for which, perms in WORKLOADS:
            system(which).hommola_cospeciation(perms, seed=1)
        return
    res = {"reps": max(a.reps, 5)}
    for which, perms in WORKLOADS:
        res[which] = run_one(which, perms, res["reps"])
    res["kernels"] = None if a.no_profile else profile()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
