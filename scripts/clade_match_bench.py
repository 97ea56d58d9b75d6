"""Measure st_clade_match (SuchTree.compare_clades, SuchTree.transfer_support) and print one JSON line.  The ranges are
built once, outside the timed calls (their time is reported as `ranges_s`); a timed call is _capi.clade_match: the sort of
the candidates and the windows, the upload, every chunk, the read-back.

  ml_nj_unrooted / ml_nj_rooted   tests/golden/ml_tree.npz against nj_tree.npz, all 54,327 shared leaves.
  balanced_caterpillar            a balanced tree against a caterpillar, 65,536 leaves, leaf k of one is leaf k of the
                                  other (unrooted): every candidate size occurs once.
  transfer_support                20 replicates of a seeded random tree of 16,384 leaves, each 200 seeded nearest-neighbour
                                  interchanges away from it: per replicate the range builder and one st_clade_match, A's
                                  ranges built once -- the loop of SuchTree.transfer_support, over parent arrays.
  Each: median / min / max wall time of `--reps` calls after a warm-up; rows x candidates per second (the problem's size
  over the time) and the candidate evaluations the kernel really made per second (the windows, plus all candidates for
  the rows that fell back: counted on the host from the results); both with the size windows on and off
  (SUCHTREE_AMD_CLADE_MATCH_WINDOW).
  host     st_clade_match(device = -1), the one-thread restatement, over 256 rows spread across the size deciles, against
           all candidates; `all_rows_extrapolated_s` scales it to every row (an extrapolation, not a measurement).
  sets     the route the reference's bipartitions() offers: every candidate as a Python frozenset, 8 rows matched with
           len(a & b); `all_rows_extrapolated_s` likewise.  Not run where the candidates' sets would not fit in memory.
  kernels  from further runs under `rocprofv3 --kernel-trace --stats`, one child per workload and window setting, each
           under its own time limit, stopping at the first that fails: the summed time of k_clade_match.

    python scripts/clade_match_bench.py [--reps 5] [--no-profile]
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

WINDOW = "SUCHTREE_AMD_CLADE_MATCH_WINDOW"
NAMES = ("ml_nj_unrooted", "ml_nj_rooted", "balanced_caterpillar", "transfer_support")


def sides(parent_a, ids_a, parent_b, ids_b, rooted, side_a=None):
    """(m, pos_b, a_lo, a_hi, b_lo, b_hi) of two parent arrays over aligned leaf-id lists."""
    from suchtree_amd import _capi
    side_a = side_a or _capi.clade_ranges(parent_a, ids_a, rooted)
    side_b = _capi.clade_ranges(parent_b, ids_b, rooted)
    m = len(ids_a)
    where_b = np.empty(m, dtype=np.int32)
    where_b[side_b[0]] = np.arange(m, dtype=np.int32)
    return m, where_b[side_a[0]], side_a[2], side_a[3], side_b[2], side_b[3]


def interchanges(parent, count, rng):
    """`count` random nearest-neighbour interchanges on a copy of a binary parent array."""
    parent = np.array(parent)
    kids = [[] for _ in parent]
    for v, p in enumerate(parent):
        if p >= 0:
            kids[p].append(v)
    inner = [v for v in range(len(parent)) if kids[v] and parent[v] >= 0]
    done = 0
    while done < count:
        v = inner[int(rng.integers(len(inner)))]
        p = int(parent[v])
        moved, sibling = kids[v][int(rng.integers(2))], [c for c in kids[p] if c != v][0]
        kids[v][kids[v].index(moved)], kids[p][kids[p].index(sibling)] = sibling, moved
        parent[moved], parent[sibling] = p, v
        done += 1
    return parent


class Work:
    """One prepared workload: a list of (m, pos_b, a_lo, a_hi, b_lo, b_hi) and the mode; `prepare` is timed in the call
    where a replicate's ranges are part of it."""

    def __init__(self, name, rooted, cases=None, prepare=None, n_prepare=0):
        self.name, self.rooted, self.cases, self.prepare, self.n_prepare = name, rooted, cases, prepare, n_prepare

    def call(self, device=0):
        from suchtree_amd import _capi
        t0 = time.perf_counter()
        cases = self.cases if self.prepare is None else (self.prepare(r) for r in range(self.n_prepare))
        out = [_capi.clade_match(*c, rooted=self.rooted, device=device) for c in cases]
        return time.perf_counter() - t0, out

    def all_cases(self):
        return self.cases if self.prepare is None else [self.prepare(r) for r in range(self.n_prepare)]


def workloads(only=None):
    from suchtree_amd import _capi, synth
    out = []
    if only is None or only.startswith("ml_nj"):
        g = os.path.join(ROOT, "tests", "golden")
        ml, nj = np.load(os.path.join(g, "ml_tree.npz")), np.load(os.path.join(g, "nj_tree.npz"))
        ids = ml["leaf_ids"].astype(np.int64)
        nj_of = np.load(os.path.join(g, "ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
        for rooted in (False, True):
            name = "ml_nj_rooted" if rooted else "ml_nj_unrooted"
            if only in (None, name):
                t0 = time.perf_counter()
                case = sides(ml["parent"], ids, nj["parent"], nj_of, rooted)
                w = Work(name, rooted, [case])
                w.ranges_s = time.perf_counter() - t0
                out.append(w)
    if only in (None, "balanced_caterpillar"):
        n = 65_536
        ids = np.arange(n, dtype=np.int64) * 2
        t0 = time.perf_counter()
        case = sides(synth.balanced_tree(16)[0], ids, synth.caterpillar_tree(n)[0], ids, False)
        w = Work("balanced_caterpillar", False, [case])
        w.ranges_s = time.perf_counter() - t0
        out.append(w)
    if only in (None, "transfer_support"):
        n = 16_384
        parent = synth.random_binary_tree(n, seed=31)[0].astype(np.int32)
        ids = np.arange(n, dtype=np.int64) * 2
        rng = np.random.default_rng(32)
        reps = [interchanges(parent, 200, rng).astype(np.int32) for _ in range(20)]
        side_a = _capi.clade_ranges(parent, ids, False)
        w = Work("transfer_support", False, prepare=lambda r: sides(parent, ids, reps[r], ids, False, side_a), n_prepare=20)
        w.ranges_s = None      # (inside the timed call)
        out.append(w)
    return out


def evaluations(case, rooted, distance):
    """(rows x candidates, the evaluations the windowed kernel makes) of one case, from its results."""
    m, _, a_lo, a_hi, b_lo, b_hi = case
    sa, sb = (a_hi - a_lo).astype(np.int64), np.sort((b_hi - b_lo).astype(np.int64))
    bound = (sa if rooted else np.minimum(sa, m - sa)) - 1
    span = lambda x, y: np.maximum(np.searchsorted(sb, y, "right") - np.searchsorted(sb, x, "left"), 0)      # noqa: E731
    win = span(sa - bound + 1, sa + bound - 1)
    if not rooted:
        both = span(np.minimum(sa, m - sa) - bound + 1, np.maximum(sa, m - sa) + bound - 1)
        win = np.minimum(win + span(m - sa - bound + 1, m - sa + bound - 1), both)      # (two windows that meet are one)
    fell_back = (distance < 0) | (distance >= bound)
    return len(sa) * len(sb), int(win.sum() + fell_back.sum() * len(sb)), int(fell_back.sum())


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def measure(w, reps):
    from suchtree_amd import _capi
    cases = w.all_cases()
    res = {"rooted": w.rooted, "leaves": int(cases[0][0]), "rows": int(sum(len(c[2]) for c in cases)), "candidates": int(sum(len(c[4]) for c in cases)),
           "calls": len(cases), "ranges_s": w.ranges_s}
    first = None
    for value in ("1", "0"):
        os.environ[WINDOW] = value
        _, got = w.call()
        if first is None:
            first = got
        assert all((g[k] == f[k]).all() for g, f in zip(got, first) for k in range(3))
        ts = []
        for _ in range(reps):
            ts.append(w.call()[0])
            print("%s window %s: %.4f s" % (w.name, value, ts[-1]), file=sys.stderr, flush=True)
        counts = [evaluations(c, w.rooted, g[0].astype(np.int64)) for c, g in zip(cases, first)]
        nominal, windowed, fell = (sum(c[k] for c in counts) for k in range(3))
        med = float(np.median(ts))
        res["window_on" if value == "1" else "window_off"] = dict(
            spread(ts), rows_x_candidates=nominal, rows_x_candidates_per_s=nominal / med,
            evaluations=windowed if value == "1" else nominal, evaluations_per_s=(windowed if value == "1" else nominal) / med,
            rows_that_scanned_all=fell if value == "1" else res["rows"])
    del os.environ[WINDOW]
    res["exact"] = int(sum(int((g[0] == 0).sum()) for g in first))
    # the one-thread restatement over 256 rows spread across the size deciles of the first case
    m, pos, a_lo, a_hi, b_lo, b_hi = cases[0]
    by_size = np.argsort(a_hi - a_lo, kind="stable")
    rows = by_size[np.linspace(0, len(by_size) - 1, 256).astype(np.int64)]
    t0 = time.perf_counter()
    host = _capi.clade_match(m, pos, a_lo[rows], a_hi[rows], b_lo, b_hi, rooted=w.rooted, device=-1)
    hs = time.perf_counter() - t0
    assert all((host[k] == first[0][k][rows]).all() for k in range(3))
    all_rows = hs * res["rows"] / 256
    res["host"] = {"rows": 256, "wall_s": hs, "evaluations_per_s": 256 * len(b_lo) / hs, "all_rows_extrapolated_s": all_rows,
                   "note": "one thread; all rows of the workload scaled from 256 rows: an extrapolation"}
    res["device_over_host"] = res["host"]["all_rows_extrapolated_s"] / res["window_on"]["median_s"]
    # the Python set route on 8 rows
    if int((b_hi - b_lo).astype(np.int64).sum()) <= 20_000_000:
        where = np.empty(m, dtype=np.int64)      # A position of B position
        where[pos] = np.arange(m)
        t0 = time.perf_counter()
        b_sets = [frozenset(where[lo:hi].tolist()) for lo, hi in zip(b_lo, b_hi)]
        build_s = time.perf_counter() - t0
        pick = rows[np.linspace(0, 255, 8).astype(np.int64)]
        t0 = time.perf_counter()
        for r in pick:
            a = frozenset(range(int(a_lo[r]), int(a_hi[r])))
            best = None
            for index, b in enumerate(b_sets):
                d = len(a) + len(b) - 2 * len(a & b)
                d = d if w.rooted else min(d, m - d)
                if best is None or (d, index) < best:
                    best = (d, index)
            assert best == (int(first[0][0][r]), int(first[0][1][r]))
        ss = time.perf_counter() - t0
        res["sets"] = {"rows": 8, "build_candidate_sets_s": build_s, "wall_s": ss, "all_rows_extrapolated_s": build_s + ss * res["rows"] / 8,
                       "note": "frozensets and len(a & b); all rows scaled from 8 rows: an extrapolation"}
    else:
        res["sets"] = {"skipped": "the candidates' sets hold %d elements" % int((b_hi - b_lo).astype(np.int64).sum())}
    return res


def profile(names=NAMES):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    res = {}
    for name in names:
        for value in ("1", "0"):
            key = "%s_window_%s" % (name, "on" if value == "1" else "off")
            out = tempfile.mkdtemp(prefix="clade_match_bench_")
            try:
                cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "cm", "--", sys.executable,
                       os.path.abspath(__file__), "--child", name]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **{WINDOW: value}))
                if p.returncode != 0:      # (a child that failed may have faulted the GPU: nothing more is started on it)
                    res[key] = {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
                    res["error"] = "%s: rocprofv3 exit %d; profiling stopped" % (key, p.returncode)
                    return res
                traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
                if not traces:
                    res[key] = {"error": "no kernel trace written"}
                    continue
                wall = json.loads(p.stdout.strip().splitlines()[-1])
                total, launches = 0, 0
                for r in csv.DictReader(open(traces[0])):
                    if "k_clade_match" in r["Kernel_Name"]:
                        total += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                        launches += 1
                kernel_s = total / 2e9      # (the trace covers the warm-up call as well: halve)
                res[key] = {"kernel_s": kernel_s, "launches": launches // 2, "call_wall_s": wall["wall_s"],
                            "rows_x_candidates_per_s_kernel": wall["nominal"] / kernel_s if kernel_s else None,
                            "upload_read_back_and_host_s": wall["wall_s"] - kernel_s}
            except subprocess.TimeoutExpired:
                res[key] = {"error": "time limit"}
                res["error"] = "%s: time limit; profiling stopped" % key
                return res
            finally:
                shutil.rmtree(out, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        w, = workloads(a.child)
        w.call()
        cases = w.all_cases()
        print(json.dumps({"wall_s": w.call()[0], "nominal": int(sum(len(c[2]) * len(c[4]) for c in cases))}))
        return
    res = {}
    for w in workloads():
        res[w.name] = measure(w, max(a.reps, 5))
    res["kernels"] = None if a.no_profile else profile()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
