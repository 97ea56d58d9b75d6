"""Measure compare.linkage -- exact UPGMA through st_linkage_codes -- on the device, against its host restatement and
against scipy.cluster.hierarchy.linkage on the same float matrix, and the topology test's relabellings, and print one
JSON line.  Seeded random distances (numpy.random.default_rng(n).random), method average.

  linkage   n = 1024, 4096 and 16384.  After a warm-up the device call and the host restatement alternate on the same
            matrix, `reps` times each: median, min and max wall time of compare.linkage (checks, quantising, upload,
            kernels, read-back, the Dendrogram); scipy's linkage(method="average") on the same condensed float64 values in
            scipy's pair order, where scipy is installed, takes its turn in the same loop.  The device's rows are compared
            with the host's byte for byte.
  cache     n = 1024 and 4096 under SUCHTREE_AMD_LINKAGE_CACHE = lds and global: the same figure.
  kernels   from runs of their own under `rocprofv3 --kernel-trace --stats`, one per n: the time of the two grid passes
            and of the chain, and the chain's time per step.  No further run is started after one that fails.
  rescans   rows the cache scans again per step, row a's included, counted by the host restatement (the device scans
            the same rows): scripts/micro/linkage_rescans.cpp, built here with g++.
  test      dendrogram_congruence with 999 relabellings at n = 256 and n = 4096 against the dendrogram of a second
            random matrix, matches on the device and on the host: wall time of the loop per relabelling.

    python scripts/linkage_bench.py [--reps 5] [--sizes 1024,4096,16384] [--no-profile] [--no-scipy]
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

KERNELS = ("k_linkage_expand", "k_linkage_nearest", "k_linkage_chain")
ENV = "SUCHTREE_AMD_LINKAGE_CACHE"


def matrix(n, seed=None):
    """condensed float64 distances in this library's pair order"""
    return np.random.default_rng(n if seed is None else seed).random(n * (n - 1) // 2)


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def scipy_order(v, n):
    """the same values condensed as scipy reads them (row-major over the upper triangle)"""
    sq = np.zeros((n, n))
    i, j = np.tril_indices(n, -1)
    sq[i, j] = sq[j, i] = v
    return sq[np.triu_indices(n, 1)]


def run_linkage(sizes, reps, with_scipy):
    from suchtree_amd import compare
    hier = None
    if with_scipy:
        try:
            import scipy.cluster.hierarchy as hier
        except ImportError:
            hier = None
    res = {}
    compare.linkage(matrix(8), device=0)
    for n in sizes:
        v = matrix(n)
        u = scipy_order(v, n) if hier else None
        compare.linkage(v, device=0)      # warm-up of this shape
        t_dev, t_host, t_sci = [], [], []
        for _ in range(reps):      # alternating
            t, dev = timed(lambda: compare.linkage(v, device=0))
            t_dev.append(t)
            t, host = timed(lambda: compare.linkage(v, device=None))
            t_host.append(t)
            if hier:
                t, _ = timed(lambda: hier.linkage(u, method="average"))
                t_sci.append(t)
            print("n = %d: device %.4f s, host %.4f s%s" % (n, t_dev[-1], t_host[-1], ", scipy %.4f s" % t_sci[-1] if hier else ""), file=sys.stderr, flush=True)
        same = all(getattr(dev, k).tobytes() == getattr(host, k).tobytes() for k in ("left", "right", "size", "num", "den"))
        res[str(n)] = {"device": spread(t_dev), "host": spread(t_host), "scipy": spread(t_sci) if hier else None, "same_integers": same,
                       "host_over_device": float(np.median(t_host) / np.median(t_dev)),
                       "device_faster_beyond_either_spread": bool(max(t_dev) < min(t_host)),
                       "host_faster_beyond_either_spread": bool(max(t_host) < min(t_dev))}
    return res


def run_cache(sizes, reps):
    from suchtree_amd import compare
    res = {}
    try:
        for n in sizes:
            v = matrix(n)
            for form in ("lds", "global"):
                os.environ[ENV] = form
                compare.linkage(v, device=0)
                ts = [timed(lambda: compare.linkage(v, device=0))[0] for _ in range(reps)]
                res["%d_%s" % (n, form)] = spread(ts)
                print("n = %d, cache %s: %.4f s" % (n, form, float(np.median(ts))), file=sys.stderr, flush=True)
    finally:
        os.environ.pop(ENV, None)
    return res


def run_rescans(sizes):
    cxx = shutil.which("g++")
    if cxx is None:
        return {"error": "g++ not found"}
    from suchtree_amd import _capi
    tmp = tempfile.mkdtemp(prefix="linkage_rescans_")
    try:
        exe = os.path.join(tmp, "linkage_rescans")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "scripts", "micro", "linkage_rescans.cpp"),
                               os.path.join(ROOT, "suchtree_amd", "csrc", "linkage_plan.cpp")])
        res = {}
        for n in sizes:
            codes, _ = _capi.mantel_quantise(matrix(n))
            path = os.path.join(tmp, "codes.bin")
            codes.tofile(path)
            _, steps, rescans = (int(x) for x in subprocess.run([exe, path, str(n), "0"], capture_output=True, text=True, check=True).stdout.split())
            res[str(n)] = {"steps": steps, "rescans": rescans, "per_step": rescans / steps}
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run_test(reps_sizes=(256, 4096), permutations=999):
    from suchtree_amd import compare
    res = {}
    for n in reps_sizes:
        tree = compare.linkage(matrix(n, 7 * n), device=None).to_flat()
        ids = np.fromiter((tree.leaves[str(i)] for i in range(n)), dtype=np.int64, count=n)
        dend = compare.linkage(matrix(n), device=None)
        for name, device in (("device", 0), ("host", None)):
            compare.dendrogram_congruence(tree, ids, dend, permutations=3, seed=1, device=device)
            t0, _ = timed(lambda: compare.dendrogram_congruence(tree, ids, dend, permutations=0, seed=1, device=device))
            t, got = timed(lambda: compare.dendrogram_congruence(tree, ids, dend, permutations=permutations, seed=1, keep_stats=True, device=device))
            res["%d_%s" % (n, name)] = {"wall_s": t, "without_relabellings_s": t0, "per_relabelling_s": (t - t0) / permutations, "rf": got.rf,
                                        "n_le": got.n_le, "perm_rf_sum": int(got.perm_rf.sum())}
            print("test n = %d, %s: %.3f s, %.3g s a relabelling" % (n, name, t, (t - t0) / permutations), file=sys.stderr, flush=True)
    return res


def profile(n):
    """the kernel times of one device call at n from a traced run of its own; {"error": ...} where it fails"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="linkage_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "lk", "--", sys.executable, os.path.abspath(__file__), "--child", str(n)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env={k: v for k, v in os.environ.items() if k != ENV})
        except subprocess.TimeoutExpired:
            return {"error": "time limit"}
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
        secs = {k: v / 2e9 for k, v in sums.items()}      # (the trace holds the call twice: halved)
        return {"kernel_s": secs, "chain_s_per_step": secs.get("k_linkage_chain", 0.0) / (n - 1), "call_wall_s": wall["wall_s"],
                "host_and_copies_s": wall["wall_s"] - sum(secs.values()), "note": "one call (the trace holds it twice; halved)"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-test", action="store_true")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        from suchtree_amd import _capi
        codes, _ = _capi.mantel_quantise(matrix(a.child))
        _capi.linkage_codes(codes, device=0)
        print(json.dumps({"wall_s": timed(lambda: _capi.linkage_codes(codes, device=0))[0]}))
        return
    sizes = [int(s) for s in a.sizes.split(",")]
    res = {"linkage": run_linkage(sizes, max(a.reps, 5), not a.no_scipy), "cache": run_cache([n for n in sizes if n <= 4096], max(a.reps, 5)),
           "rescans": run_rescans(sizes)}
    if not a.no_test:
        res["test"] = run_test()
    if not a.no_profile:
        res["kernels"] = {}
        for n in sizes:
            got = res["kernels"][str(n)] = profile(n)
            print("kernels n = %d: %s" % (n, json.dumps(got)), file=sys.stderr, flush=True)
            if "error" in got:
                res["kernels_stopped_after"] = n
                break
    print(json.dumps(res))


if __name__ == "__main__":
    main()
