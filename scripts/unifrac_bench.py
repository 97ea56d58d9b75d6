"""Measure st_unifrac_host (SuchTree.unifrac, SuchLinkedTrees.partner_unifrac) and print one JSON line.  The sets are
prepared once, outside the timed calls; a timed call is TreeHandle.unifrac_host: depths, table, every chunk, read-back.

  a_rows_A   the system of scripts/clade_bench.py (TreeB 100,000 leaves, TreeA 256, 149,685 links): of="A", every TreeA
             row with a partner, all pairs of the triangle -- 256 sets of about 585 partners, every pair in the wave form.
  a_rows_B   the same system, of="B": every TreeB row with a partner (sets of one or two TreeA leaves, every pair in the
             lane form).  The whole triangle is 5e9 pairs: `--range-rows` whole rows from the middle of it are timed, and
             `whole_triangle_extrapolated_s` scales that by the pair count (an extrapolation, not a measurement).
  b          4096 sets of 2 .. 512 leaves (log-uniform) over a 65,536-leaf universe, all pairs: both forms.
  Each: median / min / max wall time of `--reps` calls after a warm-up, pairs/s and merged elements/s (the sum of
  |A u B| over the pairs, counted on the host).
  host       st_unifrac_depths(device = -1), the one-thread restatement, over the first 1e6 pairs of the same range (all
             of them where the range is shorter); its results equal the device's.
  sweep      workload b under SUCHTREE_AMD_UNIFRAC_LANE_MAX = 0 (every pair in the wave form) .. 4096 (every pair in the
             lane form); the default is ST_UNIFRAC_LANE_MAX.
  kernels    from a second run under `rocprofv3 --kernel-trace --stats` of one call per workload: summed kernel time of
             k_unifrac_lane, k_unifrac_wave, k_unifrac_table and the distance kernels; `read_back_and_host_s` is that
             call's wall time less their sum (8 bytes per pair leave over the link).  `sweep_b_kernels`: the same for
             workload b under every threshold of the sweep.

    python scripts/unifrac_bench.py [--reps 5] [--range-rows 2048] [--no-profile]
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

SWEEP = (0, 8, 16, 32, 64, 128, 256, 512, 4096)


class Work:
    """One prepared call: the tree handle, root, universe, (set_pos, offsets) and a triangle range of whole rows."""

    def __init__(self, name, tree, root, member_ids, row_begin=0, row_end=None):
        self.name, self.dev, self.root = name, tree._device_tree(), int(root)
        order = tree._depth_first_leaves()
        member = np.zeros(tree.size, dtype=bool)
        member[np.concatenate(member_ids)] = True
        self.univ = order[member[order]]
        where = np.full(tree.size, -1, dtype=np.int64)
        where[self.univ] = np.arange(len(self.univ))
        pos = [np.sort(where[ids]).astype(np.int32) for ids in member_ids]
        self.k = np.array([len(p) for p in pos], dtype=np.int64)
        self.offsets = np.zeros(len(pos) + 1, dtype=np.int64)
        np.cumsum(self.k, out=self.offsets[1:])
        self.set_pos = np.concatenate(pos)
        n_sets = len(pos)
        row_end = n_sets if row_end is None else row_end
        self.begin, self.count = row_begin * (row_begin - 1) // 2, row_end * (row_end - 1) // 2 - row_begin * (row_begin - 1) // 2
        self.total = n_sets * (n_sets - 1) // 2
        # merged elements of the range: sum over its pairs of |A| + |B| - |A n B|
        seen = np.zeros(len(self.univ), dtype=np.int64)      # sets j < i that hold a position
        prefix = np.concatenate(([0], np.cumsum(self.k)))
        merged = 0
        for i in range(row_end):
            p = pos[i]
            if i >= row_begin:
                merged += i * int(self.k[i]) + int(prefix[i]) - int(seen[p].sum())
            seen[p] += 1
        self.merged = merged

    def call(self, **kw):
        t0 = time.perf_counter()
        out = self.dev.unifrac_host(self.root, self.univ, (self.set_pos, self.offsets), self.begin, self.count, **kw)
        return time.perf_counter() - t0, out

    def describe(self):
        return {"sets": len(self.k), "universe": len(self.univ), "set_size_min": int(self.k.min()), "set_size_median": float(np.median(self.k)),
                "set_size_max": int(self.k.max()), "pairs": self.count, "pairs_whole_triangle": self.total, "merged_elements": self.merged}


def workloads(range_rows, only=None):
    from suchtree_amd import SuchTree, synth
    out = []
    if only in (None, "a_rows_A", "a_rows_B"):
        import clade_bench
        S = clade_bench.system()
        _, tb, root_b, _, sets_a = S._partner_rows("A", 1, None)
        _, ta, root_a, _, sets_b = S._partner_rows("B", 1, None)
        if only in (None, "a_rows_A"):
            out.append(Work("a_rows_A", tb, root_b, sets_a))
        if only in (None, "a_rows_B"):
            lo = len(sets_b) // 2
            out.append(Work("a_rows_B", ta, root_a, sets_b, lo, min(lo + range_rows, len(sets_b))))
    if only in (None, "b"):
        tree = SuchTree(synth.random_binary_tree(65_536, seed=21))
        rng = np.random.default_rng(22)
        k = np.floor(np.exp(rng.uniform(np.log(2), np.log(513), 4096))).astype(np.int64).clip(2, 512)
        leaf_ids = np.asarray(tree.leaf_node_ids, dtype=np.int64)
        out.append(Work("b", tree, tree.root_node, [rng.choice(leaf_ids, int(n), replace=False) for n in k]))
    return out


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def measure(w, reps):
    from suchtree_amd import _capi
    res = w.describe()
    _, first = w.call()
    ts = []
    for _ in range(reps):
        t, got = w.call()
        ts.append(t)
        print("%s: %.4f s" % (w.name, t), file=sys.stderr, flush=True)
    assert (got[0] == first[0]).all() and (got[1] == first[1]).all()
    med = float(np.median(ts))
    res["device"] = dict(spread(ts), pairs_per_s=w.count / med, merged_elements_per_s=w.merged / med, result_bytes_per_s=8 * w.count / med)
    # the host restatement on one thread over the first 1e6 pairs of the range
    sample = min(w.count, 1_000_000)
    d_q, h_q, shift = _capi.unifrac_quantise(first[3], first[4])
    assert shift == first[2]
    hs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pd_q, union_q = _capi.unifrac_depths(d_q, h_q, (w.set_pos, w.offsets), w.begin, sample, device=-1)
        hs.append(time.perf_counter() - t0)
    assert (union_q == first[1][:sample]).all() and (pd_q == first[0]).all()
    hm = float(np.median(hs))
    res["host"] = dict(spread(hs), pairs=sample, pairs_per_s=sample / hm, note="includes PD of every set and the table; one thread")
    res["device_over_host_pairs_per_s"] = (w.count / med) / (sample / hm)
    if w.count < w.total:
        res["whole_triangle_extrapolated_s"] = med * w.total / w.count
    return res


def sweep(w, reps):
    out = []
    for v in SWEEP:
        os.environ["SUCHTREE_AMD_UNIFRAC_LANE_MAX"] = str(v)
        w.call()
        ts = [w.call()[0] for _ in range(reps)]
        heavy = int(np.count_nonzero((w.k[:, None] + w.k[None, :])[np.tril_indices(len(w.k), -1)] > v))
        out.append(dict(spread(ts), lane_max=v, pairs_in_wave_form=heavy, pairs_per_s=w.count / float(np.median(ts))))
        print("sweep %d: %.4f s" % (v, float(np.median(ts))), file=sys.stderr, flush=True)
    del os.environ["SUCHTREE_AMD_UNIFRAC_LANE_MAX"]
    return out


def profile(range_rows, names=("a_rows_A", "a_rows_B", "b")):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    res = {}
    for name in names:
        out = tempfile.mkdtemp(prefix="unifrac_bench_")
        try:
            cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "uf", "--", sys.executable,
                   os.path.abspath(__file__), "--child", name, "--range-rows", str(range_rows)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:      # (a child that failed may have faulted the GPU: nothing more is started on it)
                res[name] = {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
                res["error"] = "%s: rocprofv3 exit %d; profiling stopped" % (name, p.returncode)
                return res
            traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
            if not traces:
                res[name] = {"error": "no kernel trace written"}
                continue
            wall = json.loads(p.stdout.strip().splitlines()[-1])
            sums = {}
            for r in csv.DictReader(open(traces[0])):
                kn = r["Kernel_Name"]
                kind = next((k for k in ("k_unifrac_lane", "k_unifrac_wave", "k_unifrac_table", "k_unifrac_widen") if k in kn),
                            "distance" if ("k_canopy" in kn or "k_walk" in kn or "k_mrca" in kn) else "other")
                sums[kind] = sums.get(kind, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            secs = {k: v / 2e9 for k, v in sums.items()}      # (the trace covers the warm-up call as well: halve)
            pair_s = secs.get("k_unifrac_lane", 0.0) + secs.get("k_unifrac_wave", 0.0)
            res[name] = {"kernel_s": secs, "pair_kernels_s": pair_s, "pairs_per_s_pair_kernels": wall["pairs"] / pair_s if pair_s else None,
                         "merged_elements_per_s_pair_kernels": wall["merged"] / pair_s if pair_s else None, "call_wall_s": wall["wall_s"],
                         "read_back_and_host_s": wall["wall_s"] - sum(secs.values()),
                         "note": "one whole call (the trace holds two identical calls; halved); pair kernels include PD of every set"}
        finally:
            shutil.rmtree(out, ignore_errors=True)
    return res


def profile_sweep(range_rows):
    """Kernel time of workload b's pair kernels under every threshold of the sweep."""
    out = []
    for v in SWEEP:
        os.environ["SUCHTREE_AMD_UNIFRAC_LANE_MAX"] = str(v)
        r = profile(range_rows, ("b",)).get("b", {})
        out.append({"lane_max": v, "pair_kernels_s": r.get("pair_kernels_s"), "kernel_s": r.get("kernel_s"), "error": r.get("error")})
        if r.get("error"):      # (as in profile: stop at the first child that failed)
            break
    del os.environ["SUCHTREE_AMD_UNIFRAC_LANE_MAX"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--range-rows", type=int, default=2048)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        w, = workloads(a.range_rows, a.child)
        w.call()
        print(json.dumps({"wall_s": w.call()[0], "pairs": w.count, "merged": w.merged}))
        return
    from suchtree_amd import _capi
    reps = max(a.reps, 5)
    res = {"lane_max_default": _capi.UNIFRAC_LANE_MAX, "range_rows": a.range_rows}
    for w in workloads(a.range_rows):
        res[w.name] = measure(w, reps)
        if w.name == "b":
            res["sweep_b"] = sweep(w, reps)
    res["kernels"] = None if a.no_profile else profile(a.range_rows)
    res["sweep_b_kernels"] = None if a.no_profile or res["kernels"].get("error") else profile_sweep(a.range_rows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
