"""Measure the compare path (SuchTree.compare_distances) on all pairs of ml.tree vs nj.tree (54,327 shared taxa,
1,475,684,301 pairs) and print one JSON line:

  moments_s / moments_pairs_per_s     moments only (one pass)
  hist64_s / hist64_pairs_per_s       moments + a 64 x 64 histogram with given edges (one pass)
  kernels                             from a second run of this script under `rocprofv3 --kernel-trace --stats`:
                                      summed kernel time of the two trees' float32 triangle launches and of the reduction
                                      kernels (k_pair_*), each for the moments-only and the histogram pass, and the
                                      reduction's share of the summed kernel time

    python scripts/compare_bench.py [--reps 3] [--no-profile]

With --spearman it measures the exact Spearman rank correlation of the same pairs instead
(compare_distances(spearman=True): three passes over the pairs) and prints

  spearman_r, rank sums, distinct_x / distinct_y    of the full population
  moments_s                                         the moments-only call (one pass): the yardstick is three of it
  spearman_s                                        the ranks call, wall
  atomics_gadds_per_s                               scattered no-return uint32 atomic adds (libst_microbench.so) into
                                                    4 MiB, 256 MiB and 1 GiB of counters: the rate that bounds the count pass
  kernels                                           under rocprofv3: summed time of the distance kernels and of each
                                                    rank kernel (occupancy, count, scan, dot) of one ranks call

With --kendall it measures exact Kendall's tau-b (compare_distances(kendall=True): one pass over the pairs that keeps
every pair's 64-bit key, then two merge sorts and three tie scans on the device) at 1e7 pairs, 1e8 pairs and all pairs,
and writes the result, one JSON line and a readable table, to --log (default profiles/kendall_tau_r12.log):

  kendall_s                     the Kendall call, wall (best of --reps), with tau and the exact counts
  moments_s                     yardstick 1: one moments-only call over the same pairs -- the distance pass it contains
  spearman_s                    yardstick 2: a spearman=True call over the same pairs
  scipy_fetch_s / scipy_tau_s   yardstick 3, at 1e7 pairs: both distance columns fetched to the host (triangle_host), then
                                scipy.stats.kendalltau on them
  kernels                       under rocprofv3: the summed time of each kernel kind of one Kendall call per size

Reads the committed fixtures under tests/golden only.
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


def load():
    from suchtree_amd import SuchTree
    g = os.path.join(ROOT, "tests", "golden")
    z1, z2 = np.load(os.path.join(g, "ml_tree.npz")), np.load(os.path.join(g, "nj_tree.npz"))
    nj_of = np.load(os.path.join(g, "ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    T1 = SuchTree((z1["parent"], z1["distance"])).to_device()
    T2 = SuchTree((z2["parent"], z2["distance"])).to_device()
    return T1._device_tree(), T2._device_tree(), z1["leaf_ids"].astype(np.int64), nj_of


def run(reps):
    from suchtree_amd.compare import histogram_edges
    dx, dy, ids_x, ids_y = load()
    n = len(ids_x) * (len(ids_x) - 1) // 2
    dx.compare_triangle_host(dy, ids_x[:3000], ids_y[:3000])          # warm-up (kernels loaded, pipes built)
    best_m, m = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        m, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
        t = time.perf_counter() - t0
        best_m = t if best_m is None else min(best_m, t)
    edges = histogram_edges(64, None, (m.min_x, m.max_x, m.min_y, m.max_y))
    best_h, h = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        _, h = dx.compare_triangle_host(dy, ids_x, ids_y, edges=edges)
        t = time.perf_counter() - t0
        best_h = t if best_h is None else min(best_h, t)
    from suchtree_amd.compare import DistanceComparison
    r = DistanceComparison.from_moments(m).pearson_r
    return {"pairs": n, "pearson_r": r, "hist_total": int(h.sum()), "moments_s": best_m, "moments_pairs_per_s": n / best_m,
            "hist64_s": best_h, "hist64_pairs_per_s": n / best_h, "reps": reps}


def atomic_rates():
    """G adds/s of scattered no-return uint32 atomic adds, by table size."""
    import ctypes
    from suchtree_amd import build
    lib = ctypes.CDLL(build.build_microbench())
    lib.stmb_scatter_atomic_u32.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    out = {}
    for mib in (4, 256, 1024):
        rate = ctypes.c_double(0.0)
        rc = lib.stmb_scatter_atomic_u32(0, mib << 20, 4096, 3, ctypes.byref(rate))
        out["%d_MiB" % mib] = rate.value if rc == 0 else None
    return out


def run_spearman(reps):
    from suchtree_amd.compare import rank_fields
    dx, dy, ids_x, ids_y = load()
    n = len(ids_x) * (len(ids_x) - 1) // 2
    dx.compare_triangle_ranks_host(dy, ids_x[:3000], ids_y[:3000])      # warm-up (kernels loaded, pipes built)
    best_m = best_s = ranks = None
    for _ in range(reps):
        t0 = time.perf_counter()
        dx.compare_triangle_host(dy, ids_x, ids_y)
        t = time.perf_counter() - t0
        best_m = t if best_m is None else min(best_m, t)
    for _ in range(reps):
        t0 = time.perf_counter()
        _, ranks = dx.compare_triangle_ranks_host(dy, ids_x, ids_y)
        t = time.perf_counter() - t0
        best_s = t if best_s is None else min(best_s, t)
    f = rank_fields(ranks)
    return {"pairs": n, "spearman_r": f["spearman_r"], "rank_sxy": str(f["rank_sxy"]), "rank_sxx": str(f["rank_sxx"]),
            "rank_syy": str(f["rank_syy"]), "distinct_x": f["distinct_x"], "distinct_y": f["distinct_y"], "moments_s": best_m,
            "three_moments_s": 3 * best_m, "spearman_s": best_s, "spearman_pairs_per_s": n / best_s, "reps": reps}


def profile_spearman():
    """One ranks call (and its small warm-up) under rocprofv3: kernel time by kind."""
    rows = _trace(["--spearman", "--child"])
    if isinstance(rows, dict):
        return rows
    kinds = {"distance_ns": 0, "moments_ns": 0, "occupancy_ns": 0, "count_ns": 0, "scan_ns": 0, "dot_ns": 0, "other_ns": 0}
    for r in rows:
        name, ns = r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        kind = ("occupancy_ns" if "k_rank_occupancy" in name else "count_ns" if "k_rank_count" in name else
                "scan_ns" if "k_rank_block_sums" in name or "k_rank_scan" in name else "dot_ns" if "k_rank_dot" in name else
                "moments_ns" if "k_pair_" in name else "distance_ns" if "k_canopy" in name or "k_walk" in name else "other_ns")
        kinds[kind] += ns
    return kinds


KENDALL_SIZES = (10 ** 7, 10 ** 8, None)      # pairs of the triangle over all shared leaves, from pair 0; None: all of them
KENDALL_KINDS = (("k_kendall_keys", "keys_ns"), ("k_kendall_tile_sortIy", "tile_sort64_ns"), ("k_kendall_mergeIy", "merge64_ns"),
                 ("k_kendall_tile_sortIj", "tile_sort32_ns"), ("k_kendall_mergeIj", "merge32_ns"), ("k_kendall_low_words", "low_words_ns"),
                 ("k_kendall_tie", "ties_ns"), ("k_kendall_final", "final_ns"), ("k_pair_", "moments_ns"), ("k_canopy", "distance_ns"),
                 ("k_walk", "distance_ns"))
KENDALL_DEMANGLED = (("k_kendall_tile_sort<unsigned long", "tile_sort64_ns"), ("k_kendall_merge<unsigned long", "merge64_ns"),
                     ("k_kendall_tile_sort<unsigned int", "tile_sort32_ns"), ("k_kendall_merge<unsigned int", "merge32_ns"))


def _best(reps, call):
    best = out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best, out


def run_kendall(reps):
    from scipy.stats import kendalltau
    from suchtree_amd.compare import kendall_fields, rank_fields
    dx, dy, ids_x, ids_y = load()
    total = len(ids_x) * (len(ids_x) - 1) // 2
    dx.compare_triangle_kendall_host(dy, ids_x[:3000], ids_y[:3000])      # warm-up (kernels loaded, pipes built)
    dx.compare_triangle_ranks_host(dy, ids_x[:3000], ids_y[:3000])
    sizes = []
    for size in KENDALL_SIZES:
        n = total if size is None else size
        moments_s, _ = _best(reps, lambda: dx.compare_triangle_host(dy, ids_x, ids_y, 0, n))
        spearman_s, (_, ranks) = _best(reps, lambda: dx.compare_triangle_ranks_host(dy, ids_x, ids_y, 0, n))
        kendall_s, (_, counts) = _best(reps, lambda: dx.compare_triangle_kendall_host(dy, ids_x, ids_y, 0, n))
        f = kendall_fields(counts)
        row = {"pairs": n, "moments_s": moments_s, "spearman_s": spearman_s, "kendall_s": kendall_s, "kendall_pairs_per_s": n / kendall_s,
               "device_bytes": 16 * n, "kendall_tau": f["kendall_tau"], "spearman_r": rank_fields(ranks)["spearman_r"],
               "concordant": f["concordant"], "discordant": f["discordant"], "ties_x": f["ties_x"], "ties_y": f["ties_y"], "ties_xy": f["ties_xy"]}
        if size == KENDALL_SIZES[0]:      # the host route, once, at the smallest size
            t0 = time.perf_counter()
            x = dx.triangle_host(ids_x, 0, n)[0].astype(np.float32)
            y = dy.triangle_host(ids_y, 0, n)[0].astype(np.float32)
            row["scipy_fetch_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            row["scipy_tau"] = float(kendalltau(x, y)[0])
            row["scipy_tau_s"] = time.perf_counter() - t0
        sizes.append(row)
    return {"reps": reps, "sizes": sizes}


def profile_kendall():
    """One Kendall call per size (after a small warm-up) under rocprofv3: kernel time by kind, per call."""
    rows = _trace(["--kendall", "--child"])
    if isinstance(rows, dict):
        return rows
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {}
    for r in rows:
        name, ns = r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        kind = next((k for frag, k in KENDALL_DEMANGLED + KENDALL_KINDS if frag in name), "other_ns")
        cur[kind] = cur.get(kind, 0) + ns
        cur["launches"] = cur.get("launches", 0) + 1
        if kind == "final_ns":      # (the last kernel of a call)
            calls.append(cur)
            cur = {}
    return calls[1:]                # (without the warm-up)


def kendall_report(res):
    lines = ["exact Kendall tau-b over the triangle of ml.tree vs nj.tree (scripts/compare_bench.py --kendall), wall seconds, best of %d"
             % res["reps"], "%14s %10s %10s %10s %12s %22s" % ("pairs", "moments", "spearman", "kendall", "pairs/s", "tau")]
    for r in res["sizes"]:
        lines.append("%14d %10.4f %10.4f %10.4f %12.3e %22.17g" % (r["pairs"], r["moments_s"], r["spearman_s"], r["kendall_s"],
                                                                  r["kendall_pairs_per_s"], r["kendall_tau"]))
    r = res["sizes"][0]
    lines.append("host route at %d pairs: both columns fetched in %.3f s, scipy.stats.kendalltau %.3f s (tau %.17g)"
                 % (r["pairs"], r["scipy_fetch_s"], r["scipy_tau_s"], r["scipy_tau"]))
    if isinstance(res.get("kernels"), list):
        for r, k in zip(res["sizes"], res["kernels"]):
            tot = sum(v for name, v in k.items() if name.endswith("_ns"))
            lines.append("kernels at %d pairs (%d launches, %.4f s summed): " % (r["pairs"], k.get("launches", 0), tot * 1e-9) +
                         ", ".join("%s %.4f" % (name[:-3], v * 1e-9) for name, v in sorted(k.items(), key=lambda kv: -kv[1]) if name.endswith("_ns")))
    return lines


def _trace(child_args):
    """The kernel-trace rows of this script run once more under rocprofv3 (a dict describing the failure otherwise)."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="compare_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "cmp", "--", sys.executable,
               os.path.abspath(__file__)] + child_args
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        return list(csv.DictReader(open(traces[0])))
    finally:
        shutil.rmtree(out, ignore_errors=True)


def profile():
    """Run this script once more (one rep) under rocprofv3 and sum the kernel time by kind."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="compare_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "cmp", "--", sys.executable,
               os.path.abspath(__file__), "--child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written", "files": sorted(os.path.relpath(f, out) for f in
                                                                   glob.glob(os.path.join(out, "**", "*"), recursive=True))[:20]}
        rows = list(csv.DictReader(open(traces[0])))
        # the child's phases are told apart by the reduction kernel each uses: moments-only or histogram form
        phases = {"moments": {"triangle_ns": 0, "reduction_ns": 0}, "hist64": {"triangle_ns": 0, "reduction_ns": 0}}
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        pending = 0
        for r in rows:
            name, ns = r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            if "k_pair_moments<true>" in name or "k_pair_momentsILb1E" in name:
                phases["hist64"]["reduction_ns"] += ns
                phases["hist64"]["triangle_ns"] += pending
                pending = 0
            elif "k_pair_moments<false>" in name or "k_pair_momentsILb0E" in name:
                phases["moments"]["reduction_ns"] += ns
                phases["moments"]["triangle_ns"] += pending
                pending = 0
            elif "k_pair_shift" in name or "k_pair_moments_final" in name:
                pass      # (a few microseconds per call)
            elif "k_canopy" in name or "k_walk" in name:
                pending += ns
        for ph in phases.values():
            tot = ph["triangle_ns"] + ph["reduction_ns"]
            ph["reduction_share"] = ph["reduction_ns"] / tot if tot else None
        return phases
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--spearman", action="store_true", help="measure the exact Spearman rank correlation instead")
    ap.add_argument("--kendall", action="store_true", help="measure exact Kendall's tau-b instead")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "kendall_tau_r12.log"), help="where --kendall writes its report")
    ap.add_argument("--kendall-measure", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kendall_measure:
        print(json.dumps(run_kendall(a.reps)))
        return
    if a.kendall:
        if a.child:      # (under rocprofv3: one Kendall call per size, after its small warm-up)
            dx, dy, ids_x, ids_y = load()
            dx.compare_triangle_kendall_host(dy, ids_x[:3000], ids_y[:3000])
            for size in KENDALL_SIZES:
                dx.compare_triangle_kendall_host(dy, ids_x, ids_y, 0, size)
            return
        # (the measurement in a child process of its own: its 24 GB of device memory are gone before the profiled run)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kendall-measure", "--reps", str(a.reps)], capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit("the measuring child failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
        res = json.loads(p.stdout.strip().splitlines()[-1])
        res["kernels"] = None if a.no_profile else profile_kendall()
        text = "\n".join(kendall_report(res) + [json.dumps(res)]) + "\n"
        with open(a.log, "w") as f:
            f.write(text)
        sys.stdout.write(text)
        return
    if a.spearman:
        if a.child:      # (under rocprofv3: the ranks call alone, after its small warm-up)
            dx, dy, ids_x, ids_y = load()
            dx.compare_triangle_ranks_host(dy, ids_x[:3000], ids_y[:3000])
            dx.compare_triangle_ranks_host(dy, ids_x, ids_y)
            return
        res = run_spearman(a.reps)
        res["atomics_gadds_per_s"] = atomic_rates()
        res["kernels"] = None if a.no_profile else profile_spearman()
        print(json.dumps(res))
        return
    if a.child:       # (under rocprofv3: one rep of each phase, the warm-up's small triangle included)
        run(1)
        return
    res = run(a.reps)
    res["kernels"] = None if a.no_profile else profile()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
