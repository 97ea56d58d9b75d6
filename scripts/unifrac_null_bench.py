"""Measure SuchTree.unifrac_null against the per-permutation loop it replaces and print one JSON line.  A seeded synthetic
system from suchtree_amd.synth: a random binary tree of 4096 leaves, `--sets` sets (default 256) whose sizes are spread
log-uniformly over 2 .. 512, every pair of them (32,640 at 256 sets), permutations=999.

  shared   the first `--loop-perms` permutations (default 20: p = 0 .. 19), which both routes run on the same sets.
           `loop`: the only route before unifrac_null -- for each p relabel every set on the host by sigma_p (computed
           beforehand and not timed), sort it, and call compare.unifrac_from_depths(device=0), which uploads the set table
           again; `unifrac_null_depths`: one library call for the same columns from the same quantised depths.  Both
           after a warm-up, alternating, `reps` times each: median, min and max wall time.  The integers of the two
           routes are compared.  `beats_loop_beyond_spread`: the new call's slowest run against the loop's fastest.
           `loop_999_extrapolated_s` scales the loop's median by 1000 / loop-perms: an extrapolation, not a measurement.
  full     999 permutations: `unifrac_null_depths` (the library call alone, 2 x 261 MB of int64 results at 256 sets) and
           `unifrac_null` (the facade on the tree: depths, groups of pairs, every null column reduced with numpy):
           median / min / max wall time, (pair, permutation) tasks per second over the wall time.
  kernels  from a second run under `rocprofv3 --kernel-trace --stats` of one library call at 999 permutations: summed
           kernel time of k_dispersion_sigma, k_null_unifrac_sets, k_null_unifrac_lane, k_null_unifrac_wave and the
           table kernel; `host_and_copies_s` is that call's wall time less their sum.

    python scripts/unifrac_null_bench.py [--reps 5] [--sets 256] [--loop-perms 20] [--no-profile]
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
    """(tree, sets of leaf ids): seeded, the system of scripts/beta_dispersion_bench.py."""
    from suchtree_amd import SuchTree, synth
    tree = SuchTree(synth.random_binary_tree(LEAVES, seed=14))
    rng = np.random.default_rng(21)
    k = np.floor(np.exp(rng.uniform(np.log(2), np.log(513), n_sets))).astype(np.int64).clip(2, 512)
    leaf_ids = np.asarray(tree.leaf_node_ids, dtype=np.int64)
    return tree, [np.sort(rng.choice(leaf_ids, int(n), replace=False)) for n in k]


def depths(tree, sets):
    """(universe, position sets, float32 d, h): what the loop starts from."""
    univ = tree._depth_first_leaves()
    where = np.full(tree.size, -1, dtype=np.int64)
    where[univ] = np.arange(len(univ))
    pos = [np.sort(where[s]) for s in sets]
    _, _, _, d, h = tree._device_tree().unifrac_host(tree.root_node, univ, [np.arange(len(univ))], 0, 0)
    return univ, pos, d, h


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def loop(d, h, pos, sigmas, shift):
    """The route of the parent commit: per permutation relabel on the host, sort, one unifrac_from_depths on the device."""
    from suchtree_amd import compare
    t0 = time.perf_counter()
    out = [compare.unifrac_from_depths(d, h, [np.sort(sigma[s]) for s in pos], shift=shift, device=0) for sigma in sigmas]
    return time.perf_counter() - t0, out


def call_depths(d_q, h_q, pos, perms):
    from suchtree_amd import _capi
    t0 = time.perf_counter()
    out = _capi.unifrac_null_depths(d_q, h_q, pos, permutations=perms, seed=SEED, stream=0, device=0)
    return time.perf_counter() - t0, out


def call_facade(tree, sets):
    t0 = time.perf_counter()
    res = tree.unifrac_null(sets, permutations=PERMUTATIONS, seed=SEED)
    return time.perf_counter() - t0, res


def run(reps, n_sets, loop_perms):
    from suchtree_amd import _capi, compare
    tree, sets = system(n_sets)
    univ, pos, d, h = depths(tree, sets)
    d_q, h_q, shift = _capi.unifrac_quantise(d, h)
    pairs = n_sets * (n_sets - 1) // 2
    sigmas = [compare.hommola_permutation(SEED, 0, p, 0, LEAVES) for p in range(loop_perms)]
    k = np.array([len(s) for s in sets], dtype=np.int64)
    res = {"leaves": LEAVES, "sets": n_sets, "pairs": pairs, "permutations": PERMUTATIONS, "positions": int(k.sum()), "shift": shift,
           "shared_permutations": loop_perms}
    loop(d, h, pos, sigmas[:2], shift)      # warm-up of both routes
    call_depths(d_q, h_q, pos, loop_perms - 1)
    t_loop, t_new = [], []
    for _ in range(reps):      # alternating
        t, want = loop(d, h, pos, sigmas, shift)
        t_loop.append(t)
        t, got = call_depths(d_q, h_q, pos, loop_perms - 1)
        t_new.append(t)
        print("shared: loop %.3f s, unifrac_null_depths %.4f s" % (t_loop[-1], t_new[-1]), file=sys.stderr, flush=True)
    same = all((w.pd_q == got[0][:, p]).all() and (w.union_q == got[1][:, p]).all() for p, w in enumerate(want))
    res["shared"] = {"loop": spread(t_loop), "unifrac_null_depths": spread(t_new), "speedup": float(np.median(t_loop) / np.median(t_new)),
                     "same_integers": bool(same), "beats_loop_beyond_spread": bool(max(t_new) < min(t_loop)),
                     "loop_999_extrapolated_s": float(np.median(t_loop) * (PERMUTATIONS + 1) / loop_perms)}
    tasks = (pairs + n_sets) * (PERMUTATIONS + 1)
    res["full"] = {}
    for name, fn in (("unifrac_null_depths", lambda: call_depths(d_q, h_q, pos, PERMUTATIONS)), ("unifrac_null", lambda: call_facade(tree, sets))):
        fn()
        ts = []
        for _ in range(reps):
            t, full = fn()
            ts.append(t)
            print("full %s: %.3f s" % (name, t), file=sys.stderr, flush=True)
        res["full"][name] = dict(spread(ts), tasks_per_s=tasks / float(np.median(ts)))
    res["full"]["n_unifrac_p_ge_at_most_0.05"] = int(np.count_nonzero(full.unifrac_p_ge <= 0.05))
    res["full"]["n_pd_ses_below_minus_2"] = int(np.count_nonzero(full.pd_ses < -2))
    return res


def profile(n_sets):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="unifrac_null_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "un", "--", sys.executable,
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
            kind = next((k for k in ("k_dispersion_sigma", "k_null_unifrac_sets", "k_null_unifrac_lane", "k_null_unifrac_wave", "k_unifrac_table")
                         if k in name), "other")
            sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        # (the trace covers the depths and the warm-up call as well: `other` holds the depth kernels, the rest is halved)
        secs = {k: v / (1e9 if k == "other" else 2e9) for k, v in sums.items()}
        mine = sum(v for k, v in secs.items() if k != "other")
        return {"kernel_s": secs, "call_wall_s": wall["wall_s"], "host_and_copies_s": wall["wall_s"] - mine,
                "note": "one library call at 999 permutations (the trace holds two identical calls; halved)"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", type=int, default=256)
    ap.add_argument("--loop-perms", type=int, default=20)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        from suchtree_amd import _capi
        tree, sets = system(a.sets)
        _, pos, d, h = depths(tree, sets)
        d_q, h_q, _ = _capi.unifrac_quantise(d, h)
        call_depths(d_q, h_q, pos, PERMUTATIONS)
        print(json.dumps({"wall_s": call_depths(d_q, h_q, pos, PERMUTATIONS)[0]}))
        return
    res = run(max(a.reps, 5), a.sets, max(a.loop_perms, 2))
    res["kernels"] = None if a.no_profile else profile(a.sets)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
