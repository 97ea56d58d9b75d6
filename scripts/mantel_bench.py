"""Measure st_mantel_codes against the per-permutation numpy loop it replaces and print one JSON line.  Seeded random
codes of |value| < 2^19 (so that the numpy route's int64 dot product is exact too; the kernels' time does not depend on
the values), the simple test.

  workloads  n = 4096 with 999 permutations, n = 64 with 99,999 and n = 16384 with 99: after a warm-up, `reps` calls
             each: median, min and max wall time of the library call (the symmetry check, the invariant sums, the
             uploads, the kernels, the read-back) and pair terms per second over it.
  shared     the first `--loop-perms` permutations (default 20: p = 0 .. 19) of the n = 4096 workload, which both routes
             run.  `numpy`: the only route before -- per permutation x[np.ix_(s, s)], condensed, one dot product in
             int64 (sigma_p computed beforehand and not timed); `mantel_codes`: one library call for the same records.
             Alternating, `reps` times each: median, min and max.  The integers of the two routes are compared.
             `numpy_999_extrapolated_s` scales the numpy median by 1000 / loop-perms: an extrapolation, not a measurement.
  forms      the n = 4096 workload with the row staged in LDS (the product) and with SUCHTREE_AMD_MANTEL_GATHER=1 (the
             same tasks, the word gathered from the row in global memory), alternating: wall time and records compared.
  kernels    from runs of their own under `rocprofv3 --kernel-trace --stats`, one per workload and form: summed kernel
             time of k_dispersion_sigma, k_mantel_rows / k_mantel_wave and k_mantel_fold of one call, the pair rate over
             the task kernel's time, and `host_and_copies_s`, the call's wall time less the kernels.

    python scripts/mantel_bench.py [--reps 5] [--loop-perms 20] [--no-profile]
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

SEED = 5
WORKLOADS = {"n4096": (4096, 999), "n64": (64, 99999), "n16384": (16384, 99)}


def codes(n):
    """(x_sq int32 symmetric, y int32 condensed): seeded, |value| < 2^19"""
    rng = np.random.default_rng(n)
    a = rng.integers(-(1 << 19) + 1, 1 << 19, (n, n), dtype=np.int32)
    upper = np.triu(a, 1)
    return upper + upper.T, rng.integers(-(1 << 19) + 1, 1 << 19, n * (n - 1) // 2, dtype=np.int32)


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def call(x, y, perms):
    from suchtree_amd import _capi
    t0 = time.perf_counter()
    _, rec = _capi.mantel_codes(x, y, None, perms, SEED, 0, 0)      # (returns after the read-back: the stream has drained)
    return time.perf_counter() - t0, rec


def numpy_route(x, y64, sigmas, tri):
    t0 = time.perf_counter()
    out = [int(np.dot(x[np.ix_(s, s)][tri].astype(np.int64), y64)) for s in sigmas]
    return time.perf_counter() - t0, out


def pairs_of(n, perms):
    return n * (n - 1) // 2 * (perms + 1)


def run(reps, loop_perms):
    from suchtree_amd import _capi, compare
    res = {"workloads": {}}
    data = {}
    for name, (n, perms) in WORKLOADS.items():
        x, y = data[name] = codes(n)
        call(x, y, min(perms, 9))      # warm-up
        call(x, y, perms)
        ts = []
        for _ in range(reps):
            ts.append(call(x, y, perms)[0])
            print("%s: %.4f s" % (name, ts[-1]), file=sys.stderr, flush=True)
        res["workloads"][name] = dict(spread(ts), n=n, permutations=perms, pair_terms=pairs_of(n, perms),
                                      pair_terms_per_s_over_wall=pairs_of(n, perms) / float(np.median(ts)))
    n, perms = WORKLOADS["n4096"]
    x, y = data["n4096"]
    y64, tri = y.astype(np.int64), np.tril_indices(n, -1)
    sigmas = [compare.hommola_permutation(SEED, 0, p, 0, n) for p in range(loop_perms)]
    numpy_route(x, y64, sigmas[:2], tri)
    call(x, y, loop_perms - 1)
    t_np, t_new = [], []
    for _ in range(reps):      # alternating
        t, want = numpy_route(x, y64, sigmas, tri)
        t_np.append(t)
        t, got = call(x, y, loop_perms - 1)
        t_new.append(t)
        print("shared: numpy %.3f s, mantel_codes %.4f s" % (t_np[-1], t_new[-1]), file=sys.stderr, flush=True)
    res["shared"] = {"permutations": loop_perms, "numpy": spread(t_np), "mantel_codes": spread(t_new),
                     "speedup": float(np.median(t_np) / np.median(t_new)), "same_integers": _capi.mantel_ints(got, "sxy") == want,
                     "beats_numpy_beyond_spread": bool(max(t_new) < min(t_np)),
                     "numpy_999_extrapolated_s": float(np.median(t_np) * (perms + 1) / loop_perms)}
    t_lds, t_gather = [], []
    try:
        for _ in range(reps):      # alternating
            os.environ.pop("SUCHTREE_AMD_MANTEL_GATHER", None)
            t, staged = call(x, y, perms)
            t_lds.append(t)
            os.environ["SUCHTREE_AMD_MANTEL_GATHER"] = "1"
            if not t_gather:
                call(x, y, perms)      # warm-up of the other kernel
            t, gathered = call(x, y, perms)
            t_gather.append(t)
            print("forms: lds row %.4f s, gather %.4f s" % (t_lds[-1], t_gather[-1]), file=sys.stderr, flush=True)
    finally:
        os.environ.pop("SUCHTREE_AMD_MANTEL_GATHER", None)
    res["forms"] = {"lds_row": spread(t_lds), "gather": spread(t_gather), "same_records": staged.tobytes() == gathered.tobytes()}
    return res


def profile(name, gather):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="mantel_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "mt", "--", sys.executable, os.path.abspath(__file__),
               "--child", name]
        env = dict(os.environ)
        env.pop("SUCHTREE_AMD_MANTEL_GATHER", None)
        if gather:
            env["SUCHTREE_AMD_MANTEL_GATHER"] = "1"
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        wall = json.loads(p.stdout.strip().splitlines()[-1])
        sums = {}
        for r in csv.DictReader(open(traces[0])):
            kind = next((k for k in ("k_dispersion_sigma", "k_mantel_rows", "k_mantel_wave", "k_mantel_fold") if k in r["Kernel_Name"]), "other")
            sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        secs = {k: v / 2e9 for k, v in sums.items()}      # (the trace holds two identical calls: halved)
        task = secs.get("k_mantel_rows", 0.0) + secs.get("k_mantel_wave", 0.0)
        n, perms = WORKLOADS[name]
        return {"kernel_s": secs, "call_wall_s": wall["wall_s"], "host_and_copies_s": wall["wall_s"] - sum(secs.values()),
                "pair_terms_per_s_over_task_kernel": pairs_of(n, perms) / task if task else None,
                "note": "one library call (the trace holds two identical calls; halved)"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-perms", type=int, default=20)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        n, perms = WORKLOADS[a.child]
        x, y = codes(n)
        call(x, y, perms)
        print(json.dumps({"wall_s": call(x, y, perms)[0]}))
        return
    res = run(max(a.reps, 5), max(a.loop_perms, 2))
    if not a.no_profile:
        res["kernels"] = {name: profile(name, False) for name in WORKLOADS}
        res["kernels"]["n4096_gather"] = profile("n4096", True)
    res["reference_rate"] = {"k_dispersion_tasks_gathers_per_s": 6.0e10, "note": "DESIGN.md section 18; for comparison, no threshold"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
