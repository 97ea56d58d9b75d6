"""Measure SuchTree.beta_dispersion against the per-pair, per-permutation loop it replaces and print one JSON line.  A seeded
synthetic system from suchtree_amd.synth: a random binary tree of 4096 leaves, `--sets` sets (default 256) whose sizes are
spread log-uniformly over 2 .. 512, every pair of them (32,640 at 256 sets), permutations=999.

  sample   ten pairs, one per decile of k_i k_j.  `loop`: for each pair and each of the 1000 relabellings (the same sigma,
           computed beforehand and not timed), pairwise_distances on the two relabelled lists together, the cross block's
           mean and its row and column minima with numpy on the host -- the only route before beta_dispersion;
           `beta_dispersion`: the same ten pairs, one call of two sets each.  Both after a warm-up, alternating, `reps` times
           each: median, min and max wall time.  `speedup` = loop median over beta_dispersion median;
           `loop_all_extrapolated_s` scales the loop's time to every pair by (k_i + k_j)^2, the matrix the loop builds
           (an extrapolation, not a measurement).
  full     the whole call over every pair: median / min / max wall time, pairs/s, matrix entries gathered per second over
           the wall time (2 k_i k_j gathers per pair and relabelling: both directions).
  kernels  from a second run under `rocprofv3 --kernel-trace --stats` of one whole call: summed kernel time of the
           distance kernels (the matrix), k_dispersion_sigma and the three k_setpair_tasks forms, the gather rate over
           the task kernels' time; `host_and_copies_s` is that call's wall time less their sum.

    python scripts/beta_dispersion_bench.py [--reps 5] [--sets 256] [--no-profile]
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


def system(n_sets):
    """(tree, sets of leaf ids): seeded."""
    from suchtree_amd import SuchTree, synth
    tree = SuchTree(synth.random_binary_tree(LEAVES, seed=14))
    rng = np.random.default_rng(21)
    k = np.floor(np.exp(rng.uniform(np.log(2), np.log(513), n_sets))).astype(np.int64).clip(2, 512)
    leaf_ids = np.asarray(tree.leaf_node_ids, dtype=np.int64)
    return tree, [np.sort(rng.choice(leaf_ids, int(n), replace=False)) for n in k]


def triangle(n_sets):
    i, j = np.tril_indices(n_sets, -1)      # (row-major over i, j < i: the order k = i (i - 1) / 2 + j)
    return i, j


def sample(k, i, j):
    """One pair per decile of k_i k_j (the pair whose product is nearest the decile's middle)."""
    order = np.argsort(k[i] * k[j], kind="stable")
    return [int(order[int((d + 0.5) * len(order) / 10)]) for d in range(10)]


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def loop(tree, pairs, universe, sigmas):
    """The route of the parent commit: one pairwise_distances per pair and relabelling, reduced with numpy."""
    where = np.full(tree.size, -1, dtype=np.int64)
    where[universe] = np.arange(len(universe))
    t0 = time.perf_counter()
    out = np.empty((len(pairs), len(sigmas), 2))
    for r, (a, b) in enumerate(pairs):
        pa, pb = where[a], where[b]
        for p, sigma in enumerate(sigmas):
            M = tree.pairwise_distances(np.concatenate([universe[sigma[pa]], universe[sigma[pb]]]).tolist())
            block = M[:len(pa), len(pa):]
            out[r, p, 0] = block.mean()
            out[r, p, 1] = (block.min(axis=1).sum() + block.min(axis=0).sum()) / (len(pa) + len(pb))
    return time.perf_counter() - t0, out


def call_pairs(tree, pairs):
    t0 = time.perf_counter()
    res = [tree.beta_dispersion([b, a], permutations=PERMUTATIONS, seed=SEED, keep_null=True) for a, b in pairs]
    return time.perf_counter() - t0, res


def call(tree, sets):
    t0 = time.perf_counter()
    res = tree.beta_dispersion(sets, permutations=PERMUTATIONS, seed=SEED)
    return time.perf_counter() - t0, res


def run(reps, n_sets):
    from suchtree_amd import compare
    tree, sets = system(n_sets)
    universe = tree._depth_first_leaves()
    k = np.array([len(s) for s in sets], dtype=np.int64)
    i, j = triangle(n_sets)
    gathers = 2 * int((k[i] * k[j]).sum()) * (PERMUTATIONS + 1)
    picked = sample(k, i, j)
    pairs = [(sets[i[x]], sets[j[x]]) for x in picked]
    s_ki, s_kj = k[i[picked]], k[j[picked]]
    sigmas = [compare.hommola_permutation(SEED, 0, p, 0, LEAVES) for p in range(PERMUTATIONS + 1)]
    res = {"leaves": LEAVES, "sets": n_sets, "pairs": len(i), "permutations": PERMUTATIONS, "gathers": gathers, "sample_pairs": len(picked),
           "sample_sizes": [[int(a), int(b)] for a, b in zip(s_ki, s_kj)], "sample_gathers": 2 * int((s_ki * s_kj).sum()) * (PERMUTATIONS + 1)}
    loop(tree, pairs[:2], universe, sigmas[:20])      # warm-up of both routes
    call_pairs(tree, pairs)
    t_loop, t_new = [], []
    for _ in range(reps):      # alternating
        t, want = loop(tree, pairs, universe, sigmas)
        t_loop.append(t)
        t, got = call_pairs(tree, pairs)
        t_new.append(t)
        print("sample: loop %.3f s, beta_dispersion %.4f s" % (t_loop[-1], t_new[-1]), file=sys.stderr, flush=True)
    # the two routes agree (float32 distances: the loop's matrix is the mirrored upper triangle)
    mine = np.array([[np.concatenate([[g.beta_mpd[0]], g.null_beta_mpd[0]]), np.concatenate([[g.beta_mntd[0]], g.null_beta_mntd[0]])] for g in got])
    res["sample_max_rel_diff_beta_mpd"] = float(np.max(np.abs(mine[:, 0, :] / want[:, :, 0] - 1)))
    res["sample_max_rel_diff_beta_mntd"] = float(np.max(np.abs(mine[:, 1, :] / want[:, :, 1] - 1)))
    scale = float(((k[i] + k[j]) ** 2).sum()) / float(((s_ki + s_kj) ** 2).sum())
    res["sample"] = {"loop": spread(t_loop), "beta_dispersion": spread(t_new), "speedup": float(np.median(t_loop) / np.median(t_new)),
                     "loop_all_extrapolated_s": float(np.median(t_loop) * scale), "beats_loop_beyond_spread": bool(max(t_new) < min(t_loop))}
    call(tree, sets)
    ts = []
    for _ in range(reps):
        t, full = call(tree, sets)
        ts.append(t)
        print("full: %.3f s" % t, file=sys.stderr, flush=True)
    med = float(np.median(ts))
    res["full"] = dict(spread(ts), pairs_per_s=len(i) / med, gathers_per_s_wall=gathers / med,
                       n_beta_nti_below_minus_2=int(np.count_nonzero(full.beta_mntd_ses < -2)),
                       n_beta_nti_above_2=int(np.count_nonzero(full.beta_mntd_ses > 2)))
    return res


def profile(n_sets):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="beta_dispersion_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "bd", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--sets", str(n_sets)]
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
            kind = ("sigma" if "k_dispersion_sigma" in name else "tasks_packed" if "k_setpair_tasks_packed" in name
                    else "tasks_wave" if "k_setpair_tasks_wave" in name else "tasks_group" if "k_setpair_tasks_group" in name
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
    ap.add_argument("--sets", type=int, default=256)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        tree, sets = system(a.sets)
        k = np.array([len(s) for s in sets], dtype=np.int64)
        i, j = triangle(a.sets)
        call(tree, sets)
        print(json.dumps({"wall_s": call(tree, sets)[0], "gathers": 2 * int((k[i] * k[j]).sum()) * (PERMUTATIONS + 1)}))
        return
    res = run(max(a.reps, 5), a.sets)
    res["kernels"] = None if a.no_profile else profile(a.sets)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
