"""Measure st_class_sums_codes -- every distance class of a Mantel correlogram in one pass -- against the only GPU route
there was for these sums, one st_mantel_codes call per class on the class's 0/1 indicator matrix, and against the
per-permutation numpy loop, and print one JSON line.  Seeded random codes of |value| < 2^19 and seeded random classes of
equal probability (the kernels' time does not depend on the values).

  workloads  n = 4096 with 999 permutations and K = 24 classes (Sturges' rule for that n); n = 64 with 99,999
             permutations and K = 12.  After a warm-up the two routes alternate on the same y, classes, seed and
             permutations, `reps` times each: median, min and max wall time of the library calls (checks, uploads,
             kernels, read-back; the K indicator matrices of the old route are built outside its timer), and pair terms
             per second over it.  Every column of the new call is compared with the old route's integers.
  numpy      the first `--loop-perms` permutations (default 20) of the n = 4096 workload per permutation in numpy -- the
             relabelled class of every pair, one mask and one int64 sum per class; sigma_p computed beforehand and not
             timed -- against one library call for the same rows, alternating.  `numpy_999_extrapolated_s` scales the
             numpy median by 1000 / loop-perms: an extrapolation, not a measurement.
  accumulator  the n = 4096 workload at K = 8 and K = 32 with the LDS accumulators (the default) and under
             SUCHTREE_AMD_CLASS_ACC=compare (a compare-and-add pass per class, no accumulators): wall time and, from
             runs of their own, kernel time; the sums are compared.
  slices     the n = 4096 workload under SUCHTREE_AMD_CLASS_SLICE = 4, 8, 16, 32, 64: the same two figures.
  kernels    from runs of their own under `rocprofv3 --kernel-trace --stats`, one per workload and route: summed kernel
             time of one route by kernel, the pair rate over the task kernel's time, and `host_and_copies_s`, the
             route's wall time less the kernels.  No further run is started after one that fails.

    python scripts/correlogram_bench.py [--reps 5] [--loop-perms 20] [--no-profile]
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
WORKLOADS = {"n4096": (4096, 999, 24), "n64": (64, 99999, 12)}
SLICES = (4, 8, 16, 32, 64)
AB_CLASSES = (8, 32)
KERNELS = ("k_dispersion_sigma", "k_class_expand", "k_class_rows", "k_class_wave", "k_class_fold", "k_mantel_rows", "k_mantel_wave", "k_mantel_fold")
ENV = ("SUCHTREE_AMD_CLASS_SLICE", "SUCHTREE_AMD_CLASS_ACC")


def inputs(name, n_classes=None):
    """(y int32 condensed, cls uint8 condensed, n_classes, permutations): seeded, |code| < 2^19"""
    n, perms, K = WORKLOADS[name]
    K = n_classes or K
    rng = np.random.default_rng(n)
    m = n * (n - 1) // 2
    return rng.integers(-(1 << 19) + 1, 1 << 19, m, dtype=np.int32), rng.integers(0, K, m).astype(np.uint8), K, perms


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def call_class(y, cls, K, perms):
    from suchtree_amd import _capi
    t0 = time.perf_counter()
    out = _capi.class_sums_codes(y, cls, K, perms, SEED, 0, 0)      # (returns after the read-back: the stream has drained)
    return time.perf_counter() - t0, out


def route_mantel(y, cls, K, perms, n):
    """(summed wall time of the K library calls, the K columns): the indicator matrices are built outside the timer"""
    from suchtree_amd import _capi, compare
    total, cols = 0.0, []
    for c in range(K):
        x = compare.mantel_square((cls == c).astype(np.int32), n)
        t0 = time.perf_counter()
        _, rec = _capi.mantel_codes(x, y, None, perms, SEED, 0, 0)
        total += time.perf_counter() - t0
        cols.append(_capi.mantel_ints(rec, "sxy"))
    return total, cols


def numpy_route(y64, cls_sq, K, sigmas, tri):
    t0 = time.perf_counter()
    out = []
    for s in sigmas:
        relabelled = cls_sq[s[tri[0]], s[tri[1]]]
        out.append([int(y64[relabelled == c].sum()) for c in range(K)])
    return time.perf_counter() - t0, out


def pairs_of(n, perms):
    return n * (n - 1) // 2 * (perms + 1)


def run(reps, loop_perms):
    from suchtree_amd import compare
    res = {"workloads": {}}
    for name, (n, perms, _) in WORKLOADS.items():
        y, cls, K, _ = inputs(name)
        call_class(y, cls, K, min(perms, 9))      # warm-up
        route_mantel(y, cls, 1, min(perms, 9), n)
        call_class(y, cls, K, perms)
        route_mantel(y, cls, 1, perms, n)
        t_new, t_old = [], []
        for _ in range(reps):      # alternating
            t, sums = call_class(y, cls, K, perms)
            t_new.append(t)
            t, cols = route_mantel(y, cls, K, perms, n)
            t_old.append(t)
            print("%s: class_sums_codes %.4f s, %d x mantel_codes %.4f s" % (name, t_new[-1], K, t_old[-1]), file=sys.stderr, flush=True)
        res["workloads"][name] = {
            "n": n, "permutations": perms, "n_classes": K, "pair_terms": pairs_of(n, perms),
            "class_sums_codes": dict(spread(t_new), pair_terms_per_s_over_wall=pairs_of(n, perms) / float(np.median(t_new))),
            "mantel_codes_per_class": dict(spread(t_old), calls=K, pair_terms_per_s_over_wall=pairs_of(n, perms) / float(np.median(t_old))),
            "speedup_of_medians": float(np.median(t_old) / np.median(t_new)),
            "faster_beyond_either_spread": bool(max(t_new) < min(t_old)),
            "same_integers": all(sums[:, c].tolist() == cols[c] for c in range(K))}
    n, perms, _ = WORKLOADS["n4096"]
    res["accumulator"], res["slices"] = {}, {}
    try:
        for K in AB_CLASSES:
            y, cls, _, _ = inputs("n4096", K)
            want = None
            for form in ("lds", "compare"):
                os.environ.pop("SUCHTREE_AMD_CLASS_ACC", None)
                if form == "compare":
                    os.environ["SUCHTREE_AMD_CLASS_ACC"] = "compare"
                call_class(y, cls, K, perms)
                ts = []
                for _ in range(reps):
                    t, got = call_class(y, cls, K, perms)
                    ts.append(t)
                want = got if want is None else want
                res["accumulator"]["K%d_%s" % (K, form)] = dict(spread(ts), same_sums=got.tobytes() == want.tobytes())
                print("K = %d, %s: %.4f s" % (K, form, float(np.median(ts))), file=sys.stderr, flush=True)
        os.environ.pop("SUCHTREE_AMD_CLASS_ACC", None)
        y, cls, K, _ = inputs("n4096")
        want = call_class(y, cls, K, perms)[1]
        for s in SLICES:
            os.environ["SUCHTREE_AMD_CLASS_SLICE"] = str(s)
            call_class(y, cls, K, perms)
            ts = []
            for _ in range(reps):
                t, got = call_class(y, cls, K, perms)
                ts.append(t)
            res["slices"][str(s)] = dict(spread(ts), same_sums=got.tobytes() == want.tobytes())
            print("slice %d: %.4f s" % (s, float(np.median(ts))), file=sys.stderr, flush=True)
    finally:
        for k in ENV:
            os.environ.pop(k, None)
    y64, tri = y.astype(np.int64), np.tril_indices(n, -1)
    cls_sq = np.full((n, n), 255, dtype=np.uint8)
    cls_sq[tri] = cls
    cls_sq[tri[1], tri[0]] = cls
    sigmas = [compare.hommola_permutation(SEED, 0, p, 0, n) for p in range(loop_perms)]
    numpy_route(y64, cls_sq, K, sigmas[:1], tri)
    call_class(y, cls, K, loop_perms - 1)
    t_np, t_new = [], []
    for _ in range(reps):      # alternating
        t, rows = numpy_route(y64, cls_sq, K, sigmas, tri)
        t_np.append(t)
        t, got = call_class(y, cls, K, loop_perms - 1)
        t_new.append(t)
        print("numpy %.3f s, class_sums_codes %.4f s" % (t_np[-1], t_new[-1]), file=sys.stderr, flush=True)
    res["numpy"] = {"permutations": loop_perms, "numpy": spread(t_np), "class_sums_codes": spread(t_new),
                    "speedup": float(np.median(t_np) / np.median(t_new)), "same_integers": got.tolist() == rows,
                    "numpy_999_extrapolated_s": float(np.median(t_np) * (perms + 1) / loop_perms)}
    return res


def profile(name, route, n_classes=None, env=None):
    """the kernel times of one route of workload `name` from a traced run of its own; {"error": ...} where it fails"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="correlogram_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "mc", "--", sys.executable, os.path.abspath(__file__),
               "--child", name, "--route", route, "--classes", str(n_classes or 0)]
        child_env = {k: v for k, v in os.environ.items() if k not in ENV}
        child_env.update(env or {})
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=child_env)
        except subprocess.TimeoutExpired:
            return {"error": "time limit"}
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        wall = json.loads(p.stdout.strip().splitlines()[-1])
        sums, launches = {}, {}
        for r in csv.DictReader(open(traces[0])):
            kind = next((k for k in KERNELS if k in r["Kernel_Name"]), "other")
            sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            launches[kind] = launches.get(kind, 0) + 1
        secs = {k: v / 2e9 for k, v in sums.items()}      # (the trace holds the route twice: halved)
        task = sum(secs.get(k, 0.0) for k in ("k_class_rows", "k_class_wave", "k_mantel_rows", "k_mantel_wave"))
        n, perms, _ = WORKLOADS[name]
        return {"kernel_s": secs, "launches": {k: v // 2 for k, v in launches.items()}, "kernels_total_s": sum(secs.values()), "route_wall_s": wall["wall_s"],
                "host_and_copies_s": wall["wall_s"] - sum(secs.values()),
                "pair_terms_per_s_over_task_kernel": pairs_of(n, perms) / task if task else None,
                "note": "one route (the trace holds it twice; halved)"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def profiles():
    """every traced run, in order; none is started after one that failed"""
    plan = [("kernels", "%s_%s" % (name, route), (name, route), {}) for name in WORKLOADS for route in ("class", "mantel")]
    plan += [("accumulator_kernels", "K%d_%s" % (K, form), ("n4096", "class", K), {"SUCHTREE_AMD_CLASS_ACC": "compare"} if form == "compare" else {})
             for K in AB_CLASSES for form in ("lds", "compare")]
    plan += [("slice_kernels", str(s), ("n4096", "class"), {"SUCHTREE_AMD_CLASS_SLICE": str(s)}) for s in SLICES]
    res = {}
    for section, key, args, env in plan:
        got = profile(*args, env=env)
        res.setdefault(section, {})[key] = got
        print("%s %s: %s" % (section, key, json.dumps(got.get("kernel_s", got))), file=sys.stderr, flush=True)
        if "error" in got:
            res["stopped_after"] = "%s %s" % (section, key)
            break
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-perms", type=int, default=20)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--only-profile", action="store_true", help="the traced runs alone")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--route", default="class", help=argparse.SUPPRESS)
    ap.add_argument("--classes", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        y, cls, K, perms = inputs(a.child, a.classes or None)
        n = WORKLOADS[a.child][0]
        if a.route == "class":
            call_class(y, cls, K, perms)
            wall = call_class(y, cls, K, perms)[0]
        else:
            route_mantel(y, cls, K, perms, n)
            wall = route_mantel(y, cls, K, perms, n)[0]
        print(json.dumps({"wall_s": wall}))
        return
    res = {} if a.only_profile else run(max(a.reps, 5), max(a.loop_perms, 2))
    if not a.no_profile:
        res.update(profiles())
    res["reference_rates"] = {"k_mantel_rows_pair_terms_per_s": 8.36e11, "k_group_rows_pair_terms_per_s": 3.57e12,
                              "note": "profiles/group_tests_r27.log; for comparison, no thresholds"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
