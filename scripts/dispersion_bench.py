"""Measure SuchTree.dispersion against the per-row, per-permutation loop it replaces and print one JSON line.  A seeded
synthetic system from suchtree_amd.synth: a random binary partner tree of 4096 leaves, `--rows` rows (default 4096)
whose partner counts are spread log-uniformly over 2 .. 512, permutations=999.

  sample   ten rows, one per partner-count decile.  `loop`: for each row and each of the 1000 relabellings (the same
           sigma, computed beforehand and not timed), pairwise_distances on the relabelled partners and MPD / MNTD
           with numpy on the host -- the only route before dispersion; `dispersion`: the same rows in one call.  Both
           after a warm-up, alternating, `reps` times each: median, min and max wall time.  `speedup` = loop median
           over dispersion median; `loop_all_extrapolated_s` scales the loop's time to every row by k^2 (an
           extrapolation, not a measurement).
  full     the whole call over every row: median / min / max wall time, rows/s, matrix gathers per second over the
           wall time (k (k - 1) gathers per row and relabelling).
  kernels  from a second run under `rocprofv3 --kernel-trace --stats` of one whole call: summed kernel time of the
           distance kernels (the matrix), k_dispersion_sigma and the three k_dispersion_tasks forms, the gather rate
           over the task kernels' time; `host_and_copies_s` is that call's wall time less their sum.

    python scripts/dispersion_bench.py [--reps 5] [--rows 4096] [--no-profile]
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

LEAVES, PERMUTATIONS, SEED = 4096, 999, 5


def system(rows):
    """(tree, sets of leaf ids): seeded."""
    from suchtree_amd import SuchTree, synth
    tree = SuchTree(synth.random_binary_tree(LEAVES, seed=14))
    rng = np.random.default_rng(15)
    k = np.floor(np.exp(rng.uniform(np.log(2), np.log(513), rows))).astype(np.int64).clip(2, 512)
    leaf_ids = np.asarray(tree.leaf_node_ids, dtype=np.int64)
    return tree, [np.sort(rng.choice(leaf_ids, int(n), replace=False)) for n in k]


def sample(sets):
    """One row per partner-count decile (the row whose count is nearest the decile's middle)."""
    k = np.array([len(s) for s in sets])
    order = np.argsort(k, kind="stable")
    return [int(order[int((d + 0.5) * len(k) / 10)]) for d in range(10)]


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def loop(tree, sets, universe, sigmas):
    """The route of the parent commit: one pairwise_distances per row and relabelling, reduced with numpy."""
    where = np.full(tree.size, -1, dtype=np.int64)
    where[universe] = np.arange(len(universe))
    t0 = time.perf_counter()
    out = np.empty((len(sets), len(sigmas), 2))
    for r, s in enumerate(sets):
        pos = where[s]
        for p, sigma in enumerate(sigmas):
            M = tree.pairwise_distances(universe[sigma[pos]].tolist())
            k = len(pos)
            out[r, p, 0] = M.sum() / (k * (k - 1))
            np.fill_diagonal(M, np.inf)
            out[r, p, 1] = M.min(axis=1).mean()
    return time.perf_counter() - t0, out


def call(tree, sets):
    t0 = time.perf_counter()
    res = tree.dispersion(sets, permutations=PERMUTATIONS, seed=SEED, keep_null=True)
    return time.perf_counter() - t0, res


def run(reps, rows):
    from suchtree_amd import compare
    tree, sets = system(rows)
    universe = tree._depth_first_leaves()
    k = np.array([len(s) for s in sets], dtype=np.int64)
    gathers = int((k * (k - 1)).sum()) * (PERMUTATIONS + 1)
    picked = sample(sets)
    s_sets = [sets[i] for i in picked]
    s_k = k[picked]
    sigmas = [compare.hommola_permutation(SEED, 0, p, 0, LEAVES) for p in range(PERMUTATIONS + 1)]
    res = {"leaves": LEAVES, "rows": rows, "permutations": PERMUTATIONS, "gathers": gathers, "sample_rows": len(picked),
           "sample_partner_counts": s_k.tolist(), "sample_gathers": int((s_k * (s_k - 1)).sum()) * (PERMUTATIONS + 1)}
    loop(tree, s_sets[:2], universe, sigmas[:20])      # warm-up of both routes
    call(tree, s_sets)
    t_loop, t_new = [], []
    for _ in range(reps):      # alternating
        t, want = loop(tree, s_sets, universe, sigmas)
        t_loop.append(t)
        t, got = call(tree, s_sets)
        t_new.append(t)
        print("sample: loop %.3f s, dispersion %.4f s" % (t_loop[-1], t_new[-1]), file=sys.stderr, flush=True)
    # the two routes agree (float32 distances: the loop's matrix is the mirrored upper triangle)
    res["sample_max_rel_diff_mpd"] = float(np.max(np.abs(np.column_stack([got.mpd, got.null_mpd]) / want[:, :, 0] - 1)))
    res["sample_max_rel_diff_mntd"] = float(np.max(np.abs(np.column_stack([got.mntd, got.null_mntd]) / want[:, :, 1] - 1)))
    res["sample"] = {"loop": spread(t_loop), "dispersion": spread(t_new), "speedup": float(np.median(t_loop) / np.median(t_new)),
                     "loop_all_extrapolated_s": float(np.median(t_loop) * float((k * k).sum()) / float((s_k * s_k).sum())),
                     "beats_loop_beyond_spread": bool(max(t_new) < min(t_loop))}
    call(tree, sets)
    ts = []
    for _ in range(reps):
        t, full = call(tree, sets)
        ts.append(t)
        print("full: %.3f s" % t, file=sys.stderr, flush=True)
    med = float(np.median(ts))
    res["full"] = dict(spread(ts), rows_per_s=rows / med, gathers_per_s_wall=gathers / med,
                       n_clustered_at_0_05=int(np.count_nonzero(full.mpd_p <= 0.05)))
    return res


def profile(rows):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="dispersion_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "pd", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--rows", str(rows)]
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
            kind = ("sigma" if "k_dispersion_sigma" in name else "tasks_packed" if "k_dispersion_tasks_packed" in name
                    else "tasks_wave" if "k_dispersion_tasks_wave" in name else "tasks_group" if "k_dispersion_tasks_group" in name
                    else "distance" if ("k_canopy" in name or "k_walk" in name) else "other")
            sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        # (the trace covers the warm-up call as well: halve)
        secs = {k: v / 2e9 for k, v in sums.items()}
        tasks = sum(v for k, v in secs.items() if k.startswith("tasks_"))
        return {"kernel_s": secs, "tasks_s": tasks, "gathers_per_s_tasks": wall["gathers"] / tasks if tasks else None,
                "call_wall_s": wall["wall_s"], "host_and_copies_s": wall["wall_s"] - sum(secs.values()),
                "note": "one whole call (the trace holds two identical calls; halved)"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        tree, sets = system(a.rows)
        k = np.array([len(s) for s in sets], dtype=np.int64)
        call(tree, sets)
        print(json.dumps({"wall_s": call(tree, sets)[0], "gathers": int((k * (k - 1)).sum()) * (PERMUTATIONS + 1)}))
        return
    res = run(max(a.reps, 5), a.rows)
    res["kernels"] = None if a.no_profile else profile(a.rows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
