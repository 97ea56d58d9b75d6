"""Measure SuchLinkedTrees.hommola_by_clade against the per-clade loop it replaces and print one JSON line.  The seeded
system of scripts/clade_bench.py (TreeB = 100,000 leaves, 149,685 links), the notebook's filters (min_leaves=10,
min_links=10, max_links=2500), permutations=999.

  sample   >= 200 kept clades spread over the link-count deciles.  `loop`: subset_b(c); hommola_cospeciation(999) for
           each of them -- the only route before hommola_by_clade; `by_clade`: the same clades with nodes=.  Both after
           a warm-up, alternating, `reps` times each: median, min and max wall time.  `speedup` = loop median over
           by_clade median; `loop_all_extrapolated_s` scales the loop's time to every kept clade by pair count (an
           extrapolation, not a measurement).
  full     the whole call over every kept clade: median / min / max wall time, clades/s, pairs/s (pairs of one
           permutation x 1000 rows), bytes of the distance matrices.
  kernels  from a second run under `rocprofv3 --kernel-trace --stats` of one by_clade call on the sample: summed kernel
           time of the distance kernels (the matrices), the relabelling sorts and k_hommola_blocks; `host_and_copies_s`
           is that call's wall time less their sum (the fold of pieces runs on the host beside the device).

    python scripts/hommola_clade_bench.py [--reps 5] [--no-full] [--full-budget-s 240] [--no-profile]
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

FILTERS = dict(min_leaves=10, min_links=10, max_links=2500)
PERMUTATIONS = 999


def kept_clades(S):
    """(nodes, n_links, n_leaves) of the clades the filters keep and the default max_leaves evaluates."""
    C = S.hommola_by_clade(permutations=0, seed=1, **FILTERS)
    return C.nodes, C.n_links, C.n_leaves


def sample(nodes, n_links, size=200):
    """`size` clades spread over the link-count deciles (seeded)."""
    rng = np.random.default_rng(4)
    edges = np.quantile(n_links, np.linspace(0, 1, 11))
    picked = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        pool = np.flatnonzero((n_links >= lo) & (n_links <= hi))
        picked.extend(rng.choice(pool, min(len(pool), size // 10), replace=False).tolist())
    picked = sorted(set(picked))
    return nodes[picked], n_links[picked]


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def loop(S, nodes):
    root = S.TreeB.root_node
    t0 = time.perf_counter()
    for v in nodes:
        S.subset_b(int(v))
        S.hommola_cospeciation(PERMUTATIONS, seed=5)
    t = time.perf_counter() - t0
    S.subset_b(root)
    return t


def by_clade(S, nodes=None):
    t0 = time.perf_counter()
    C = S.hommola_by_clade(permutations=PERMUTATIONS, seed=5, nodes=nodes, **FILTERS)
    return time.perf_counter() - t0, C


def run(reps, full, full_budget_s):
    import clade_bench
    S = clade_bench.system()
    nodes, n_links, n_leaves = kept_clades(S)
    pairs = n_links * (n_links - 1) // 2
    s_nodes, s_links = sample(nodes, n_links)
    s_pairs = int((s_links * (s_links - 1) // 2).sum())
    res = {"n_links": int(S.subset_n_links), "kept_clades": len(nodes), "kept_pairs_per_permutation": int(pairs.sum()),
           "permutations": PERMUTATIONS, "sample_clades": len(s_nodes), "sample_pairs_per_permutation": s_pairs}
    print("kept %d clades, sample %d" % (len(nodes), len(s_nodes)), file=sys.stderr, flush=True)
    loop(S, s_nodes[:5])      # warm-up of both routes
    by_clade(S, s_nodes)
    t_loop, t_new = [], []
    for _ in range(reps):      # alternating
        t_loop.append(loop(S, s_nodes))
        t_new.append(by_clade(S, s_nodes)[0])
        print("sample: loop %.3f s, by_clade %.3f s" % (t_loop[-1], t_new[-1]), file=sys.stderr, flush=True)
    res["sample"] = {"loop": spread(t_loop), "by_clade": spread(t_new),
                     "speedup": float(np.median(t_loop) / np.median(t_new)),
                     "loop_all_extrapolated_s": float(np.median(t_loop) * int(pairs.sum()) / s_pairs)}
    res["sample"]["beats_loop_beyond_spread"] = bool(max(t_new) < min(t_loop))
    if full:
        ts = []
        for _ in range(reps):
            t, C = by_clade(S)
            ts.append(t)
            print("full: %.3f s" % t, file=sys.stderr, flush=True)
            if sum(ts) > full_budget_s:      # (a slow machine: fewer repeats, reported as such)
                break
        med = float(np.median(ts))
        parent = np.asarray(S.TreeB._flat.parent)
        leaves = S._leaf_counts(S.TreeB)
        top = np.flatnonzero((leaves <= 4096) & ((parent < 0) | (leaves[np.maximum(parent, 0)] > 4096)))
        res["full"] = dict(spread(ts), rows=len(C), clades_per_s=len(C) / med,
                           pairs_per_s=float(pairs.sum()) * (PERMUTATIONS + 1) / med,
                           matrix_bytes_all_groups=int(4 * (256 * 256 + int((leaves[top].astype(np.int64) ** 2).sum()))),
                           n_significant_at_0_05=int(np.count_nonzero(C.p_value <= 0.05)))
    return res


def profile():
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="hommola_clade_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "hc", "--", sys.executable,
               os.path.abspath(__file__), "--child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        wall = json.loads(p.stdout.strip().splitlines()[-1])
        sums = {}
        for r in csv.DictReader(open(traces[0])):
            name = r["Kernel_Name"]
            kind = ("relabel" if "k_hommola_relabel" in name else "blocks" if "k_hommola_blocks" in name
                    else "distance" if ("k_canopy" in name or "k_walk" in name) else "other")
            sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        # (the trace covers the warm-up call as well: halve)
        secs = {k: v / 2e9 for k, v in sums.items()}
        return {"kernel_s": secs, "call_wall_s": wall["wall_s"], "host_and_copies_s": wall["wall_s"] - sum(secs.values()),
                "note": "one by_clade call on the sample (the trace holds two identical calls; halved)"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-full", action="store_true")
    ap.add_argument("--full-budget-s", type=float, default=240.0, help="stop repeating the whole call once this much time has gone into it")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        import clade_bench
        S = clade_bench.system()
        nodes, n_links, _ = kept_clades(S)
        s_nodes, _ = sample(nodes, n_links)
        by_clade(S, s_nodes)
        print(json.dumps({"wall_s": by_clade(S, s_nodes)[0]}))
        return
    res = run(max(a.reps, 5), not a.no_full, a.full_budget_s)
    res["kernels"] = None if a.no_profile else profile()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
