"""Measure st_group_sums_codes against the only GPU route there was for these sums -- st_mantel_codes with x the 0/1
co-membership matrix, which gives the sum over all groups only -- and against the per-permutation numpy loop, and print
one JSON line.  Seeded random codes of |value| < 2^19 (the kernels' time does not depend on the values).

  workloads  n = 4096 with 999 permutations and 8 groups of unequal size; n = 64 with 99,999 permutations and 4 groups.
             After a warm-up the two routes alternate on the same y, grouping, seed and permutations, `reps` times each:
             median, min and max wall time of the library call (checks, uploads, kernels, read-back), and pair terms
             per second over it.  The row sums of the new call are compared with the Mantel route's integers.
  slices     the n = 4096 workload under SUCHTREE_AMD_GROUP_SLICE = 4, 8, 16, 32, 64: wall time (median of `reps`) and,
             from a run of its own under `rocprofv3 --kernel-trace --stats`, the kernel time; the sums are compared.
  numpy      the first `--loop-perms` permutations (default 20) of the n = 4096 workload per permutation in numpy
             (sigma_p computed beforehand and not timed) against one library call for the same rows, alternating.
             `numpy_999_extrapolated_s` scales the numpy median by 1000 / loop-perms: an extrapolation, not a measurement.
  kernels    from runs of their own under `rocprofv3 --kernel-trace --stats`, one per workload and route: summed kernel
             time of one call by kernel, the pair rate over the task kernel's time, and `host_and_copies_s`, the call's
             wall time less the kernels.

    python scripts/group_test_bench.py [--reps 5] [--loop-perms 20] [--no-profile]
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
WORKLOADS = {"n4096": (4096, 999, (1200, 900, 700, 500, 350, 250, 150, 46)), "n64": (64, 99999, (28, 18, 12, 6))}
SLICES = (4, 8, 16, 32, 64)
KERNELS = ("k_dispersion_sigma", "k_group_relabel", "k_group_rows", "k_group_wave", "k_group_fold", "k_mantel_rows", "k_mantel_wave", "k_mantel_fold")


def inputs(name):
    """(y int32 condensed, group uint8 shuffled, n_groups, permutations): seeded, |code| < 2^19"""
    n, perms, sizes = WORKLOADS[name]
    assert sum(sizes) == n
    rng = np.random.default_rng(n)
    y = rng.integers(-(1 << 19) + 1, 1 << 19, n * (n - 1) // 2, dtype=np.int32)
    return y, rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.uint8), len(sizes), perms


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def call_group(y, g, a, perms):
    from suchtree_amd import _capi
    t0 = time.perf_counter()
    out = _capi.group_sums_codes(y, g, a, perms, SEED, 0, 0)      # (returns after the read-back: the stream has drained)
    return time.perf_counter() - t0, out


def call_mantel(x, y, perms):
    from suchtree_amd import _capi
    t0 = time.perf_counter()
    _, rec = _capi.mantel_codes(x, y, None, perms, SEED, 0, 0)
    return time.perf_counter() - t0, rec


def indicator(g):
    return (g[:, None] == g[None, :]).astype(np.int32)


def numpy_route(y64, g, a, sigmas, tri):
    t0 = time.perf_counter()
    out = []
    for s in sigmas:
        lab = g[s]
        li = lab[tri[0]]
        same = li == lab[tri[1]]
        out.append([int(y64[same & (li == h)].sum()) for h in range(a)])
    return time.perf_counter() - t0, out


def pairs_of(n, perms):
    return n * (n - 1) // 2 * (perms + 1)


def run(reps, loop_perms):
    from suchtree_amd import _capi, compare
    res = {"workloads": {}}
    for name, (n, perms, sizes) in WORKLOADS.items():
        y, g, a, _ = inputs(name)
        x = indicator(g)
        call_group(y, g, a, min(perms, 9))      # warm-up
        call_mantel(x, y, min(perms, 9))
        call_group(y, g, a, perms)
        call_mantel(x, y, perms)
        t_new, t_old = [], []
        for _ in range(reps):      # alternating
            t, sums = call_group(y, g, a, perms)
            t_new.append(t)
            t, rec = call_mantel(x, y, perms)
            t_old.append(t)
            print("%s: group_sums_codes %.4f s, mantel_codes %.4f s" % (name, t_new[-1], t_old[-1]), file=sys.stderr, flush=True)
        res["workloads"][name] = {
            "n": n, "permutations": perms, "group_sizes": list(sizes), "pair_terms": pairs_of(n, perms),
            "group_sums_codes": dict(spread(t_new), pair_terms_per_s_over_wall=pairs_of(n, perms) / float(np.median(t_new))),
            "mantel_codes_on_indicator": dict(spread(t_old), pair_terms_per_s_over_wall=pairs_of(n, perms) / float(np.median(t_old))),
            "speedup_of_medians": float(np.median(t_old) / np.median(t_new)),
            "faster_beyond_either_spread": bool(max(t_new) < min(t_old)),
            "same_integers": sums.sum(axis=1).tolist() == _capi.mantel_ints(rec, "sxy")}
    y, g, a, perms = inputs("n4096")
    n = WORKLOADS["n4096"][0]
    res["slices"] = {}
    try:
        for s in SLICES:
            os.environ["SUCHTREE_AMD_GROUP_SLICE"] = str(s)
            call_group(y, g, a, perms)
            ts = []
            for _ in range(reps):
                t, got = call_group(y, g, a, perms)
                ts.append(t)
            res["slices"][str(s)] = dict(spread(ts), same_sums=got.tobytes() == sums_4096(y, g, a, perms).tobytes())
            print("slice %d: %.4f s" % (s, float(np.median(ts))), file=sys.stderr, flush=True)
    finally:
        os.environ.pop("SUCHTREE_AMD_GROUP_SLICE", None)
    y64, tri = y.astype(np.int64), np.tril_indices(n, -1)
    sigmas = [compare.hommola_permutation(SEED, 0, p, 0, n) for p in range(loop_perms)]
    numpy_route(y64, g, a, sigmas[:2], tri)
    call_group(y, g, a, loop_perms - 1)
    t_np, t_new = [], []
    for _ in range(reps):      # alternating
        t, want = numpy_route(y64, g, a, sigmas, tri)
        t_np.append(t)
        t, got = call_group(y, g, a, loop_perms - 1)
        t_new.append(t)
        print("numpy %.3f s, group_sums_codes %.4f s" % (t_np[-1], t_new[-1]), file=sys.stderr, flush=True)
    res["numpy"] = {"permutations": loop_perms, "numpy": spread(t_np), "group_sums_codes": spread(t_new),
                    "speedup": float(np.median(t_np) / np.median(t_new)), "same_integers": got.tolist() == want,
                    "numpy_999_extrapolated_s": float(np.median(t_np) * (perms + 1) / loop_perms)}
    return res


_default = {}


def sums_4096(y, g, a, perms):
    """the n = 4096 sums under the built-in slice, computed once"""
    if "sums" not in _default:
        saved = os.environ.pop("SUCHTREE_AMD_GROUP_SLICE", None)
        _default["sums"] = call_group(y, g, a, perms)[1]
        if saved is not None:
            os.environ["SUCHTREE_AMD_GROUP_SLICE"] = saved
    return _default["sums"]


def profile(name, route, slice_len=None):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="group_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "gt", "--", sys.executable, os.path.abspath(__file__),
               "--child", name, "--route", route]
        env = dict(os.environ)
        env.pop("SUCHTREE_AMD_GROUP_SLICE", None)
        if slice_len:
            env["SUCHTREE_AMD_GROUP_SLICE"] = str(slice_len)
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        wall = json.loads(p.stdout.strip().splitlines()[-1])
        sums = {}
        for r in csv.DictReader(open(traces[0])):
            kind = next((k for k in KERNELS if k in r["Kernel_Name"]), "other")
            sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        secs = {k: v / 2e9 for k, v in sums.items()}      # (the trace holds two identical calls: halved)
        task = secs.get("k_group_rows", 0.0) + secs.get("k_group_wave", 0.0) + secs.get("k_mantel_rows", 0.0) + secs.get("k_mantel_wave", 0.0)
        n, perms, _ = WORKLOADS[name]
        return {"kernel_s": secs, "kernels_total_s": sum(secs.values()), "call_wall_s": wall["wall_s"],
                "host_and_copies_s": wall["wall_s"] - sum(secs.values()),
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
    ap.add_argument("--route", default="group", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        y, g, n_groups, perms = inputs(a.child)
        if a.route == "group":
            call_group(y, g, n_groups, perms)
            wall = call_group(y, g, n_groups, perms)[0]
        else:
            x = indicator(g)
            call_mantel(x, y, perms)
            wall = call_mantel(x, y, perms)[0]
        print(json.dumps({"wall_s": wall}))
        return
    res = run(max(a.reps, 5), max(a.loop_perms, 2))
    if not a.no_profile:
        res["kernels"] = {"%s_%s" % (name, route): profile(name, route) for name in WORKLOADS for route in ("group", "mantel")}
        res["slice_kernels"] = {str(s): profile("n4096", "group", s) for s in SLICES}
    res["reference_rate"] = {"k_mantel_rows_pair_terms_per_s": 8.08e11, "note": "DESIGN.md section 23; for comparison, no threshold"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
