"""Measure st_parafit_codes against the per-permutation numpy loop it replaces and print one JSON line (progress on
stderr).  Seeded random symmetric codes of |value| < 2^19 (so that the numpy route's int64 sums are exact too; the
kernels' time does not depend on the values), seeded random distinct links.

  workloads  L = 2048 links over 1024 x 1024 positions with 999 permutations, gopher / louse (the golden system, its
             centred and quantised tree distances, TreeB held) with 99,999 and L = 16384 over 1024 x 1024 with 99: after a
             warm-up, `reps` calls each: median, min and max wall time of the library call (the checks, the uploads, the
             kernels, the read-back of totals, observations and counts) and pair terms (L^2 per permutation) per second.
  shared     the first `--loop-perms` permutations (default 20: p = 0 .. 19) of the L = 2048 workload, which both routes
             run.  `numpy`: the only route before -- per permutation T = P * g_s[np.ix_(r, r)] in int64 with P the
             expanded held side, its row sums, the trace and 2 x row sum - diagonal (the relabelled positions r computed
             beforehand and not timed); `parafit_codes`: one library call for the same values, every link row kept.
             Alternating, `reps` times each: median, min and max.  The integers of the two routes are compared.
             `numpy_999_extrapolated_s` scales the numpy median by 1000 / loop-perms: an extrapolation, not a measurement.
  kernels    from runs of their own under `rocprofv3 --kernel-trace --stats`, one per workload: summed kernel time of
             k_parafit_expand, k_parafit_relabel*, k_parafit_rows / k_parafit_wave and k_parafit_fold of one call, the
             pair rate over the task kernel's time, the share of the relabel kernels, and `host_and_copies_s`, the
             call's wall time less the kernels.

    python scripts/parafit_bench.py [--reps 5] [--loop-perms 20] [--no-profile]
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
WORKLOADS = {"L2048": (1024, 1024, 2048, 999), "gopher_louse": (None, None, None, 99999), "L16384": (1024, 1024, 16384, 99)}
KERNELS = ("k_parafit_expand", "k_parafit_relabel", "k_parafit_rows", "k_parafit_wave", "k_parafit_fold")


def symmetric(rng, n):
    a = rng.integers(-(1 << 19) + 1, 1 << 19, (n, n), dtype=np.int32)
    return np.tril(a) + np.tril(a, -1).T


def case(name):
    """(g_f, g_s, link_f, link_s, stream_f, permutations) of a workload"""
    n_f, n_s, L, perms = WORKLOADS[name]
    if name == "gopher_louse":
        import pandas as pd
        from suchtree_amd import SuchTree, _capi, compare
        d = os.path.join(ROOT, "tests", "golden", "gopher_louse")
        ta, tb, table = SuchTree(d + "/gopher.tree"), SuchTree(d + "/lice.tree"), pd.read_csv(d + "/links.csv", index_col=0)
        ids_a, ids_b = sorted(ta.leaves.values()), sorted(tb.leaves.values())
        links = sorted((ids_b.index(tb.leaves[b]), ids_a.index(ta.leaves[a])) for a in table.index for b in table.columns if table.loc[a, b] > 0)
        g = [_capi.mantel_quantise(compare.parafit_centre(compare.mantel_condensed(t.pairwise_distances(ids))[0], len(ids)))[0]
             for t, ids in ((tb, ids_b), (ta, ids_a))]
        links = np.array(links)
        return g[0], g[1], links[:, 0], links[:, 1], np.arange(len(ids_b)), perms
    rng = np.random.default_rng(L)
    cells = np.sort(rng.choice(n_f * n_s, L, replace=False))
    return symmetric(rng, n_f), symmetric(rng, n_s), cells // n_s, cells % n_s, np.arange(n_f), perms


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def call(c, perms, keep=False):
    from suchtree_amd import _capi
    t0 = time.perf_counter()
    out = _capi.parafit_codes(c[0], c[1], c[2], c[3], c[4], perms, SEED, 0, 0, keep=keep)      # (returns after the read-back: the stream has drained)
    return time.perf_counter() - t0, out


def numpy_route(P, g_s, images):
    t0 = time.perf_counter()
    out = []
    for r in images:
        T = P * g_s[np.ix_(r, r)].astype(np.int64)
        rows = T.sum(axis=1)
        out.append((int(rows.sum()), (2 * rows - np.diag(T)).tolist()))
    return time.perf_counter() - t0, out


def images_of(c, n_perms):
    """the relabelled S position of every link for p = 0 .. n_perms - 1"""
    from suchtree_amd import compare
    _, g_s, link_f, link_s, stream_f, _ = c
    out = []
    for p in range(n_perms):
        r = link_s.copy()
        if p:
            for f in np.unique(link_f).tolist():
                sigma = np.asarray(compare.hommola_permutation(SEED, int(stream_f[f]), p, 0, len(g_s)))
                mine = link_f == f
                r[mine] = sigma[link_s[mine]]
        out.append(r)
    return out


def run(reps, loop_perms):
    from suchtree_amd import _capi
    res = {"workloads": {}}
    cases = {}
    for name in WORKLOADS:
        c = cases[name] = case(name)
        perms, L = c[5], len(c[2])
        call(c, min(perms, 9))      # warm-up
        call(c, perms)
        ts = []
        for _ in range(reps):
            ts.append(call(c, perms)[0])
            print("%s: %.4f s" % (name, ts[-1]), file=sys.stderr, flush=True)
        terms = L * L * (perms + 1)
        res["workloads"][name] = dict(spread(ts), n_f=len(c[0]), n_s=len(c[1]), n_links=L, permutations=perms, pair_terms=terms,
                                      pair_terms_per_s_over_wall=terms / float(np.median(ts)))
    c = cases["L2048"]
    P = c[0][np.ix_(c[2], c[2])].astype(np.int64)      # (the expansion is not timed either)
    images = images_of(c, loop_perms)
    numpy_route(P, c[1], images[:2])
    call(c, loop_perms - 1, keep=True)
    t_np, t_new = [], []
    for _ in range(reps):      # alternating
        t, want = numpy_route(P, c[1], images)
        t_np.append(t)
        t, got = call(c, loop_perms - 1, keep=True)
        t_new.append(t)
        print("shared: numpy %.3f s, parafit_codes %.4f s" % (t_np[-1], t_new[-1]), file=sys.stderr, flush=True)
    mine = list(zip(_capi.parafit_ints(got[0]), _capi.parafit_ints(got[3])))
    res["shared"] = {"permutations": loop_perms, "numpy": spread(t_np), "parafit_codes": spread(t_new),
                     "speedup": float(np.median(t_np) / np.median(t_new)), "same_integers": mine == want,
                     "beats_numpy_beyond_spread": bool(max(t_new) < min(t_np)),
                     "numpy_999_extrapolated_s": float(np.median(t_np) * (c[5] + 1) / loop_perms)}
    return res


def profile(name):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="parafit_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "pf", "--", sys.executable, os.path.abspath(__file__),
               "--child", name]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
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
        other = sums.pop("other", 0) / 1e9      # (the golden system's distance kernels run once, before the calls)
        secs = {k: v / 2e9 for k, v in sums.items()}      # (the trace holds two identical calls: halved)
        task = secs.get("k_parafit_rows", 0.0) + secs.get("k_parafit_wave", 0.0)
        total = sum(secs.values())
        return {"kernel_s": secs, "other_kernels_s": other, "call_wall_s": wall["wall_s"], "host_and_copies_s": wall["wall_s"] - total,
                "pair_terms_per_s_over_task_kernel": wall["pair_terms"] / task if task else None,
                "relabel_share_of_kernel_time": secs.get("k_parafit_relabel", 0.0) / total if total else None,
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
        c = case(a.child)
        call(c, c[5])
        print(json.dumps({"wall_s": call(c, c[5])[0], "pair_terms": len(c[2]) ** 2 * (c[5] + 1)}))
        return
    res = run(max(a.reps, 5), max(a.loop_perms, 2))
    if not a.no_profile:
        res["kernels"] = {name: profile(name) for name in WORKLOADS}
    res["reference_rate"] = {"k_mantel_rows_pair_terms_per_s": 8.08e11, "note": "DESIGN.md section 23; for comparison, no threshold"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
