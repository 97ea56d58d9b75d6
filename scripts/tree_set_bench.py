"""Measure st_rf_tasks (compare.tree_set, compare.rf_relabelled) -- the clades every two trees of a set share, one task
per workgroup -- and print one JSON line.

  small     1000 trees of 1024 leaves, the whole triangle (499,500 pairs, with the per-clade counts).  Each tree is one
            seeded tree after a seeded number (0 .. 39) of random prune-and-regraft moves; the quartiles of `shared` are
            printed.  After a warm-up the routes alternate, `reps` times each: the device call over the whole triangle;
            the loop of _capi.clade_match(device=0) calls over the first 2000 pairs (the only device route there was);
            the host restatement (device = -1, one thread) over the same 2000 pairs.  Pairs per second, clades tested per
            second and the bytes a task has to move (two rows of positions, j's ranges, i's keys, the result).
  large     64 trees of 16384 leaves, 2016 pairs; the same yardsticks on the first 20 pairs.
  sweep     where the device call overtakes the host restatement: trees of 64, 1024 and 16384 leaves, 2 .. 64 trees (the
            whole triangle), both routes alternating.
  relabel   999 relabellings at n = 256 and n = 4096: compare.rf_relabelled on the device and on the host against
            compare.dendrogram_congruence's loop with the matches on the device and on the host, the same dendrogram and
            seed; perm_rf is asserted equal.  The loop on the host at n = 4096 runs once.
  kernels   from a run of its own under `rocprofv3 --kernel-trace --stats` per workload: the time of k_rf_tasks in one
            device call.  No further run is started after one that fails.

    python scripts/tree_set_bench.py [--reps 5] [--only small,large,sweep,relabel,kernels]
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


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def regraft(parent, rng):
    """one random prune-and-regraft move on a binary parent array, in place: the subtree of v, with its parent p, leaves
    its place and p is put on the edge above u"""
    n = len(parent)
    while True:
        v, u = (int(x) for x in rng.integers(0, n, size=2))
        p = int(parent[v])
        if p < 0 or u == v or u == p:
            continue
        x = u
        while x >= 0 and x != v:
            x = int(parent[x])
        if x == v:      # (u is inside the subtree that moves)
            continue
        s = int([c for c in np.flatnonzero(parent == p) if c != v][0])
        if u == s:      # (back where it was)
            continue
        parent[s] = parent[p]
        parent[p] = parent[u]
        parent[u] = p
        return


def tree_set(n_trees, m, seed, max_moves=40):
    """(where, offsets, lo, hi, sides) of n_trees unrooted trees of m leaves a few moves away from one seeded tree"""
    from suchtree_amd import _capi, synth
    base = np.asarray(synth.random_binary_tree_levels(m, seed=seed)[0]).astype(np.int32)
    leaves = np.arange(m, dtype=np.int64) * 2
    rng = np.random.default_rng(seed + 1)
    sides = []
    for _ in range(n_trees):
        parent = base.copy()
        for _ in range(int(rng.integers(0, max_moves))):
            regraft(parent, rng)
        sides.append(_capi.clade_ranges(parent, leaves, False))
    where = np.empty((n_trees, m), dtype=np.int32)
    for t, side in enumerate(sides):
        where[t, side[0]] = np.arange(m, dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s[1]) for s in sides])]).astype(np.int64)
    return where, offsets, np.concatenate([s[2] for s in sides]), np.concatenate([s[3] for s in sides]), sides


def pair_of(k):
    i = int((1 + np.sqrt(8.0 * k + 1.0)) // 2)
    while i * (i - 1) // 2 > k:
        i -= 1
    while (i + 1) * i // 2 <= k:
        i += 1
    return i, k - i * (i - 1) // 2


def run_triangle(n_trees, m, yard_pairs, reps, seed):
    from suchtree_amd import _capi
    where, offsets, lo, hi, sides = tree_set(n_trees, m, seed)
    total = n_trees * (n_trees - 1) // 2
    n_clades = np.diff(offsets)

    def device():
        return _capi.rf_tasks(m, where, offsets, lo, hi, device=0)

    def host():
        return _capi.rf_tasks(m, where, offsets, lo, hi, count=yard_pairs, want_count=False, device=-1)[0]

    def loop():
        out = np.zeros(yard_pairs, dtype=np.int64)
        for k in range(yard_pairs):
            i, j = pair_of(k)
            distance, match, _ = _capi.clade_match(m, where[j][sides[i][0]], sides[i][2], sides[i][3], sides[j][2], sides[j][3], False, 0)
            out[k] = int(((match >= 0) & (distance == 0)).sum())
        return out
    shared, counts = device()      # warm-up
    assert (host() == shared[:yard_pairs]).all() and (loop() == shared[:yard_pairs]).all()
    t_dev, t_loop, t_host = [], [], []
    for _ in range(reps):      # alternating
        t_dev.append(timed(device)[0])
        t_loop.append(timed(loop)[0])
        t_host.append(timed(host)[0])
        print("%d x %d: device %.4f s (%d pairs), clade_match loop %.4f s, host %.4f s (%d pairs)" % (n_trees, m, t_dev[-1], total, t_loop[-1], t_host[-1],
                                                                                                      yard_pairs), file=sys.stderr, flush=True)
    i, j = np.array([pair_of(k) for k in range(total)]).T
    tested = int(n_clades[j].sum())
    dev = float(np.median(t_dev))
    return {"trees": n_trees, "leaves": m, "pairs": total, "yardstick_pairs": yard_pairs, "shared_quartiles": np.percentile(shared, [0, 25, 50, 75, 100]).tolist(),
            "clades_per_tree_median": float(np.median(n_clades)), "device": spread(t_dev), "clade_match_loop": spread(t_loop), "host": spread(t_host),
            "device_pairs_per_s": total / dev, "device_clades_tested_per_s": tested / dev,
            "loop_pairs_per_s": yard_pairs / float(np.median(t_loop)), "host_pairs_per_s": yard_pairs / float(np.median(t_host)),
            "loop_whole_triangle_s_extrapolated": float(np.median(t_loop)) * total / yard_pairs,
            "host_whole_triangle_s_extrapolated": float(np.median(t_host)) * total / yard_pairs,
            "bytes_per_task": float(4 * m + 4 * np.mean(n_clades[j]) + 4 * np.mean(n_clades[i]) + 4),
            "frequency_quartiles": np.percentile(counts + 1, [0, 25, 50, 75, 100]).tolist()}


def run_sweep(reps):
    from suchtree_amd import _capi
    res = {}
    _capi.rf_tasks(8, np.tile(np.arange(8, dtype=np.int32), (2, 1)), [0, 0, 0], [], [], device=0)
    for m in (64, 1024, 16384):
        where, offsets, lo, hi, _ = tree_set(64, m, 3 * m, max_moves=10)
        for n in (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
            w, o = where[:n], offsets[:n + 1]
            l, h = lo[:o[-1]], hi[:o[-1]]
            t_dev, t_host = [], []
            for _ in range(reps):
                t, dev = timed(lambda: _capi.rf_tasks(m, w, o, l, h, device=0))
                t_dev.append(t)
                t, host = timed(lambda: _capi.rf_tasks(m, w, o, l, h, device=-1))
                t_host.append(t)
            assert (dev[0] == host[0]).all() and (dev[1] == host[1]).all()
            res["%d_%d" % (m, n)] = {"tasks": n * (n - 1) // 2, "device": spread(t_dev), "host": spread(t_host),
                                     "device_faster_beyond_either_spread": bool(max(t_dev) < min(t_host)),
                                     "host_faster_beyond_either_spread": bool(max(t_host) < min(t_dev))}
            print("sweep m = %d, %d tasks: device %.5f s, host %.5f s" % (m, n * (n - 1) // 2, np.median(t_dev), np.median(t_host)), file=sys.stderr, flush=True)
    return res


def run_relabel(reps, permutations=999):
    from suchtree_amd import compare
    res = {}
    for n in (256, 4096):
        rng = np.random.default_rng
        tree = compare.linkage(rng(7 * n).random(n * (n - 1) // 2), device=None).to_flat()
        ids = np.fromiter((tree.leaves[str(i)] for i in range(n)), dtype=np.int64, count=n)
        dend = compare.linkage(rng(n).random(n * (n - 1) // 2), device=None)
        d_flat = dend.to_flat()
        d_ids = np.fromiter((d_flat.leaves[str(i)] for i in range(n)), dtype=np.int64, count=n)
        batch = {"device": lambda: compare.rf_relabelled(tree, ids, d_flat, d_ids, permutations=permutations, seed=1, device=0),
                 "host": lambda: compare.rf_relabelled(tree, ids, d_flat, d_ids, permutations=permutations, seed=1, device=None)}
        loops = {"device": lambda: compare.dendrogram_congruence(tree, ids, dend, permutations=permutations, seed=1, keep_stats=True, device=0),
                 "host": lambda: compare.dendrogram_congruence(tree, ids, dend, permutations=permutations, seed=1, keep_stats=True, device=None)}
        batch["device"]()
        compare.dendrogram_congruence(tree, ids, dend, permutations=3, seed=1, device=0)
        times = {"batch_device": [], "batch_host": [], "loop_device": [], "loop_host": []}
        for r in range(reps):      # alternating
            t, got = timed(batch["device"])
            times["batch_device"].append(t)
            t, on_host = timed(batch["host"])
            times["batch_host"].append(t)
            t, want = timed(loops["device"])
            times["loop_device"].append(t)
            assert got.perm_rf.tolist() == want.perm_rf.tolist() == on_host.perm_rf.tolist() and (got.rf, got.n_le) == (want.rf, want.n_le)
            if n <= 256 or r == 0:
                t, slow = timed(loops["host"])
                times["loop_host"].append(t)
                assert slow.perm_rf.tolist() == got.perm_rf.tolist()
            print("relabel n = %d: %s" % (n, {k: round(v[-1], 4) for k, v in times.items() if v}), file=sys.stderr, flush=True)
        res[str(n)] = {k: dict(spread(v), per_relabelling_s=float(np.median(v)) / permutations) for k, v in times.items()}
        res[str(n)].update(rf=got.rf, n_le=got.n_le, perm_rf_sum=int(got.perm_rf.sum()))
    return res


def profile(which):
    """the time of k_rf_tasks in one device call of workload `which` from a traced run of its own; {"error": ...} where it fails"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="tree_set_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "rf", "--", sys.executable, os.path.abspath(__file__), "--child", which]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except subprocess.TimeoutExpired:
            return {"error": "time limit"}
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        wall = json.loads(p.stdout.strip().splitlines()[-1])
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(traces[0])) if "k_rf_tasks" in r["Kernel_Name"]]
        kernel = sum(ns) / 1e9
        return {"launches": len(ns), "kernel_s": kernel, "call_wall_s": wall["wall_s"], "host_and_copies_s": wall["wall_s"] - kernel, "tasks": wall["tasks"],
                "kernel_s_per_task": kernel / wall["tasks"]}
    finally:
        shutil.rmtree(out, ignore_errors=True)


CHILD = {"small": (1000, 1024, 11), "large": (64, 16384, 12)}


def child(which):
    from suchtree_amd import _capi, compare
    if which in CHILD:
        n_trees, m, seed = CHILD[which]
        where, offsets, lo, hi, _ = tree_set(n_trees, m, seed)
        t, got = timed(lambda: _capi.rf_tasks(m, where, offsets, lo, hi, device=0))      # (the one device call of the trace)
        print(json.dumps({"wall_s": t, "tasks": len(got[0])}))
        return
    n = int(which)
    tree = compare.linkage(np.random.default_rng(7 * n).random(n * (n - 1) // 2), device=None).to_flat()
    ids = np.fromiter((tree.leaves[str(i)] for i in range(n)), dtype=np.int64, count=n)
    d_flat = compare.linkage(np.random.default_rng(n).random(n * (n - 1) // 2), device=None).to_flat()
    d_ids = np.fromiter((d_flat.leaves[str(i)] for i in range(n)), dtype=np.int64, count=n)
    t, got = timed(lambda: compare.rf_relabelled(tree, ids, d_flat, d_ids, permutations=999, seed=1, device=0))
    print(json.dumps({"wall_s": t, "tasks": 1000}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="small,large,sweep,relabel,kernels")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return
    only, reps, res = a.only.split(","), max(a.reps, 1), {}
    if "small" in only:
        res["small"] = run_triangle(*CHILD["small"][:2], 2000, reps, CHILD["small"][2])
    if "large" in only:
        res["large"] = run_triangle(*CHILD["large"][:2], 20, reps, CHILD["large"][2])
    if "sweep" in only:
        res["sweep"] = run_sweep(reps)
    if "relabel" in only:
        res["relabel"] = run_relabel(reps)
    if "kernels" in only:
        res["kernels"] = {}
        for which in ("small", "large", "256", "4096"):
            got = res["kernels"][which] = profile(which)
            print("kernels %s: %s" % (which, json.dumps(got)), file=sys.stderr, flush=True)
            if "error" in got:
                res["kernels_stopped_after"] = which
                break
    print(json.dumps(res))


if __name__ == "__main__":
    main()
