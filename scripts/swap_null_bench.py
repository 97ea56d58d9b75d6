"""Measure the swap null of SuchTree.dispersion on the workload of scripts/dispersion_bench.py -- a seeded random binary
tree of 4096 leaves, `--rows` rows (default 4096) of 2 to 512 partners, permutations=999, default iterations
(max(1000, 10 x the links)) -- and print one JSON line.  Every timing is the median of `reps` (at least 5) runs with its
range.

  call        SuchTree.dispersion(null="swap") and the taxa-labels call on the same sets, alternating: wall time.
  kernels     from a run under `rocprofv3 --kernel-trace` of a warm-up and `reps` swap calls: per call the time of
              k_swap_chains and the summed time of the three k_swap_tasks forms; trials per second over the chain
              kernel's time; the same for the taxa-labels call (k_dispersion_sigma, k_dispersion_tasks).
  forms       the batched chain kernel against the plain form (SUCHTREE_AMD_SWAP_PLAIN=1: one trial per wave step) and
              the form that loads before the prefix is known (SUCHTREE_AMD_SWAP_EARLY=1), alternating, at
              `--ab-iterations` trials a chain (default: the links, a tenth of the default chain) through
              st_swap_null_tables with 999 chains and with 256.
  schedule    the mean prefix (trials per wave step) of one chain of `--schedule-iterations` trials, run on the host in
              the wave's schedule (st_swap_null_schedule); the share of trials accepted, from the call.
  host        the host restatement on 8 chains, one thread: trials per second, and its time scaled to 999 chains -- an
              extrapolation, not a measurement.

    python scripts/swap_null_bench.py [--reps 5] [--rows 4096] [--no-profile]
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

from dispersion_bench import LEAVES, PERMUTATIONS, SEED, system      # noqa: E402  (the workload)


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def call(tree, sets, null):
    t0 = time.perf_counter()
    res = tree.dispersion(sets, permutations=PERMUTATIONS, seed=SEED, null=null)
    return time.perf_counter() - t0, res


def positions(tree, sets):
    univ, rows = tree._universe_and_sets(sets, None)
    return tree._position_table(univ, rows)


FORMS = {"batched": None, "early": "SUCHTREE_AMD_SWAP_EARLY", "plain": "SUCHTREE_AMD_SWAP_PLAIN"}      # the chain kernel's forms (host_swap.h)


def timed_tables(pos_off, iterations, chains, form):
    from suchtree_amd import _capi
    if FORMS[form]:
        os.environ[FORMS[form]] = "1"
    try:
        t0 = time.perf_counter()
        out = _capi.swap_null_tables(pos_off, LEAVES, permutations=chains - 1, begin=1, iterations=iterations, seed=SEED, device=0)
        return time.perf_counter() - t0, out
    finally:
        if FORMS[form]:
            del os.environ[FORMS[form]]


def run(a):
    from suchtree_amd import _capi
    reps = max(a.reps, 5)
    tree, sets = system(a.rows)
    pos, off = positions(tree, sets)
    links = len(pos)
    iterations = _capi.swap_iterations(None, links)
    res = {"leaves": LEAVES, "rows": a.rows, "permutations": PERMUTATIONS, "links": links, "iterations": iterations,
           "trials": iterations * PERMUTATIONS}
    call(tree, sets, "swap")      # warm-up of both calls
    call(tree, sets, "taxa.labels")
    t_swap, t_taxa = [], []
    for _ in range(reps):      # alternating
        t, swap = call(tree, sets, "swap")
        t_swap.append(t)
        t, taxa = call(tree, sets, "taxa.labels")
        t_taxa.append(t)
        print("call: swap %.3f s, taxa.labels %.3f s" % (t_swap[-1], t_taxa[-1]), file=sys.stderr, flush=True)
    assert swap.mpd.tobytes() == taxa.mpd.tobytes()      # (the observation is the same)
    res["call"] = {"swap": spread(t_swap), "taxa_labels": spread(t_taxa),
                   "accepted_share": float(swap.swap_accepted[1:].sum() / (iterations * PERMUTATIONS)),
                   "n_clustered_at_0_05": {"swap": int(np.count_nonzero(swap.mpd_p <= 0.05)), "taxa_labels": int(np.count_nonzero(taxa.mpd_p <= 0.05))}}
    # the forms of the chain kernel, alternating, with the chip full (999 chains) and a quarter full (256): the same tables
    ab_iterations = a.ab_iterations or links
    res["forms"] = {"iterations": ab_iterations, "note": "wall time of st_swap_null_tables: the kernel and the copy of the table rows"}
    for chains in (PERMUTATIONS, 256):
        timed_tables((pos, off), ab_iterations, chains, "batched")
        ts, got = {f: [] for f in FORMS}, {}
        for _ in range(reps):
            for f in FORMS:
                t, got[f] = timed_tables((pos, off), ab_iterations, chains, f)
                ts[f].append(t)
            print("forms, %d chains: %s" % (chains, ", ".join("%s %.3f s" % (f, ts[f][-1]) for f in FORMS)), file=sys.stderr, flush=True)
        assert all(np.array_equal(got[f][0], got["batched"][0]) and np.array_equal(got[f][2], got["batched"][2]) for f in FORMS)
        res["forms"]["chains_%d" % chains] = dict({f: spread(ts[f]) for f in FORMS},
                                                  batched_beats_plain_beyond_spread=bool(max(ts["batched"]) < min(ts["plain"])),
                                                  batched_beats_early_beyond_spread=bool(max(ts["batched"]) < min(ts["early"])))
    # the wave's schedule on the host: trials per step
    row, accepted, steps = _capi.swap_null_schedule((pos, off), LEAVES, 1, iterations=a.schedule_iterations, seed=SEED)
    res["schedule"] = {"iterations": a.schedule_iterations, "steps": steps, "mean_prefix": a.schedule_iterations / steps,
                       "accepted_share": accepted / a.schedule_iterations}
    # the host restatement: 8 chains, one thread
    t0 = time.perf_counter()
    _capi.swap_null_tables((pos, off), LEAVES, permutations=7, begin=1, iterations=iterations, seed=SEED, device=-1)
    t_host = time.perf_counter() - t0
    res["host"] = {"chains": 8, "wall_s": t_host, "trials_per_s": 8 * iterations / t_host,
                   "all_chains_extrapolated_s": t_host * PERMUTATIONS / 8, "note": "scaled to 999 chains: an extrapolation"}
    return res


def profile(a):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="swap_null_bench_")
    reps = max(a.reps, 5)
    try:
        cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "sw", "--", sys.executable, os.path.abspath(__file__), "--child",
               "--rows", str(a.rows), "--reps", str(reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        info = json.loads(p.stdout.strip().splitlines()[-1])
        rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
        kinds = (("chains", "k_swap_chains"), ("swap_tasks", "k_swap_tasks"), ("sigma", "k_dispersion_sigma"), ("taxa_tasks", "k_dispersion_tasks"))
        calls = {"swap": [], "taxa_labels": []}      # per call: {kind: seconds}; a call begins at its first chain / sigma kernel after the other's
        last = None
        for r in rows:
            kind = next((k for k, s in kinds if s in r["Kernel_Name"]), None)
            if kind is None:
                continue
            which = "swap" if kind in ("chains", "swap_tasks") else "taxa_labels"
            if which != last:
                calls[which].append({})
                last = which
            c = calls[which][-1]
            c[kind] = c.get(kind, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e9
        res = {"calls_traced": {k: len(v) for k, v in calls.items()}, "note": "the first call of each kind is the warm-up and is left out"}
        for which, kind_list in (("swap", ("chains", "swap_tasks")), ("taxa_labels", ("sigma", "taxa_tasks"))):
            for kind in kind_list:
                res[kind] = spread([c.get(kind, 0.0) for c in calls[which][1:]])
        res["trials_per_s"] = info["trials"] / res["chains"]["median_s"]
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--ab-iterations", type=int, default=0)
    ap.add_argument("--schedule-iterations", type=int, default=2_000_000)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:      # under the profiler: a warm-up and `reps` calls of each null, alternating
        from suchtree_amd import _capi
        tree, sets = system(a.rows)
        for _ in range(a.reps + 1):
            call(tree, sets, "swap")
            call(tree, sets, "taxa.labels")
        print(json.dumps({"trials": _capi.swap_iterations(None, len(positions(tree, sets)[0])) * PERMUTATIONS}))
        return
    res = run(a)
    res["kernels"] = None if a.no_profile else profile(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
