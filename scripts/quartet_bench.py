"""Measure the quartet comparison (SuchTree.compare_quartets) on ml.tree vs nj.tree over their 54,327 shared leaves and
print JSON lines:

  {"what": "compare_quartets", "samples": n, ...}   one per sample size: wall_s (host clock around the call, which ends
                                                    in a device synchronise; best of --reps), quartets_per_s, the table's
                                                    similarity, and device_s with its split by kernel -- the summed kernel
                                                    time of one such call in a second run of this script under
                                                    `rocprofv3 --kernel-trace --stats`
  {"what": "yardstick", "samples": n, ...}          what the public API offered for the same question before: draw the
                                                    quartets on the host (numpy), quartet_topologies_bulk on both trees,
                                                    count in numpy -- in batches of 1e7 quartets; wall_s and its phases
  {"what": "mrca_rate", ...}                        MRCA ids alone (bench_legs.mrca_ids_only, the leg bench.py reports) on
                                                    uniform random leaf pairs of each tree, and per sample size the ratio
                                                    ideal / measured, ideal = 6 n ids in each tree at those rates
  {"what": "check", ...}                            both ways give the same table over the same 1e6 quartets

    python scripts/quartet_bench.py [--samples 1e6,1e7,1e8,1e9] [--yardstick 1e7,1e8] [--reps 3] [--no-profile]

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
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 1 << 22          # csrc/host_quartets.h: kQuartetChunk, the default chunk of a call
WARM = 3000
SEED = 20261017


def load():
    from suchtree_amd import SuchTree
    g = os.path.join(ROOT, "tests", "golden")
    z1, z2 = np.load(os.path.join(g, "ml_tree.npz")), np.load(os.path.join(g, "nj_tree.npz"))
    nj_of = np.load(os.path.join(g, "ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    T1 = SuchTree((z1["parent"], z1["distance"])).to_device()
    T2 = SuchTree((z2["parent"], z2["distance"])).to_device()
    return T1, T2, z1["leaf_ids"].astype(np.int64), nj_of


def classes(q, topo):
    """Class of each quartet from quartet_topologies_bulk's row: the sister of column 0."""
    sister = np.where(topo[:, 0] == q[:, 0], topo[:, 1], topo[:, 3])
    return np.where(sister == q[:, 1], 0, np.where(sister == q[:, 2], 1, 2))


def table_by_topologies(T1, T2, qx, qy, phases=None):
    t0 = time.perf_counter()
    tx, ty = T1.quartet_topologies_bulk(qx), T2.quartet_topologies_bulk(qy)
    t1 = time.perf_counter()
    table = np.bincount(4 * classes(qx, tx) + classes(qy, ty), minlength=16).reshape(4, 4)
    if phases is not None:
        phases["topologies_s"] += t1 - t0
        phases["count_s"] += time.perf_counter() - t1
    return table


def yardstick(T1, T2, ids_x, ids_y, n, batch=10_000_000):
    rng = np.random.default_rng(SEED)
    phases = {"draw_s": 0.0, "gather_s": 0.0, "topologies_s": 0.0, "count_s": 0.0}
    table = np.zeros((4, 4), dtype=np.int64)
    t_all = time.perf_counter()
    for off in range(0, n, batch):
        c = min(batch, n - off)
        t0 = time.perf_counter()
        pos = rng.integers(0, len(ids_x), (c, 4))      # (with replacement: a repeat in 1 of 9000 rows; it only favours the yardstick)
        t1 = time.perf_counter()
        qx, qy = ids_x[pos], ids_y[pos]
        phases["draw_s"] += t1 - t0
        phases["gather_s"] += time.perf_counter() - t1
        table += table_by_topologies(T1, T2, qx, qy, phases)
    wall = time.perf_counter() - t_all
    agree = int(table[0, 0] + table[1, 1] + table[2, 2])
    return dict(what="yardstick", samples=n, wall_s=wall, quartets_per_s=n / wall, similarity=agree / n, batch=batch, **phases)


def new_path(T1, T2, ids_x, ids_y, n, reps):
    best, r = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = T1.compare_quartets(T2, leaves=(ids_x, ids_y), samples=n, seed=SEED)
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return dict(what="compare_quartets", samples=n, wall_s=best, quartets_per_s=n / best, similarity=r.similarity, stderr=r.stderr,
                unresolved=r.unresolved, reps=reps)


def mrca_rates(T1, T2, ids_x, ids_y, n_pairs=100_000_000):
    """ids/s of MRCA-only requests on each tree: bench.py's own leg, on uniform random leaf pairs of that tree."""
    import torch
    import bench_legs
    dev = torch.device("cuda", 0)
    out = {}
    for name, T, ids in (("ml", T1, ids_x), ("nj", T2, ids_y)):
        rng = np.random.default_rng(3)
        pairs = torch.from_numpy(ids[rng.integers(0, len(ids), (n_pairs, 2))]).to(dev)
        tree, stream = T._device_tree(), torch.cuda.Stream(device=dev)
        first = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        with torch.cuda.stream(stream):
            tree.distances_device(pairs.data_ptr(), n_pairs, 0, first.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            be = types.SimpleNamespace(torch=torch, tree=tree, stream=stream, device=dev)
            out[name] = bench_legs.mrca_ids_only(be, pairs, first)["ids_per_s"]
        del pairs, first
    return out


def child(sizes):
    """Under rocprofv3: the warm-up, then one call per size."""
    T1, T2, ids_x, ids_y = load()
    T1.compare_quartets(T2, leaves=(ids_x, ids_y), samples=WARM, seed=SEED)
    for n in sizes:
        T1.compare_quartets(T2, leaves=(ids_x, ids_y), samples=n, seed=SEED)


def profile(sizes):
    """Kernel time of one call per size, by kind.  The calls are told apart by their k_quartet_agree launches: one per
    chunk of 2^22 quartets, after that chunk's draw and MRCA kernels."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="quartet_bench_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "q", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--samples", ",".join(str(n) for n in sizes)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-2000:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written"}
        rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
    finally:
        shutil.rmtree(out, ignore_errors=True)
    rows = [r for r in rows if any(k in r["Kernel_Name"] for k in ("k_quartet", "k_mrca", "k_canopy", "k_walk"))]
    first = next(i for i, r in enumerate(rows) if "k_quartet_draw" in r["Kernel_Name"])      # (skips what creating the trees launched)
    rows = rows[first:]
    res, at = {}, 0
    for n in [WARM] + list(sizes):
        agrees, seg = (n + CHUNK - 1) // CHUNK, {"draw_ns": 0, "mrca_ns": 0, "agree_ns": 0, "mrca_kernels": set()}
        while agrees and at < len(rows):
            name, ns = rows[at]["Kernel_Name"], int(rows[at]["End_Timestamp"]) - int(rows[at]["Start_Timestamp"])
            at += 1
            if "k_quartet_agree" in name:
                seg["agree_ns"] += ns
                agrees -= 1
            elif "k_quartet_draw" in name:
                seg["draw_ns"] += ns
            else:
                seg["mrca_ns"] += ns
                seg["mrca_kernels"].add(name.split("(")[0].split("<")[0])
        seg["mrca_kernels"] = sorted(seg["mrca_kernels"])
        seg["device_s"] = (seg["draw_ns"] + seg["mrca_ns"] + seg["agree_ns"]) * 1e-9
        res[n] = seg
    res.pop(WARM, None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="1e6,1e7,1e8,1e9")
    ap.add_argument("--yardstick", default="1e7,1e8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-rates", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sizes = [int(float(s)) for s in a.samples.split(",") if s]
    if a.child:
        child(sizes)
        return
    T1, T2, ids_x, ids_y = load()
    T1.compare_quartets(T2, leaves=(ids_x, ids_y), samples=WARM, seed=SEED)          # warm-up: code objects loaded
    T1.quartet_topologies_bulk(ids_x[:4000].reshape(-1, 4))                           # ... and the host path's pipes built
    T2.quartet_topologies_bulk(ids_y[:4000].reshape(-1, 4))

    # both ways over the same quartets: the same table
    from suchtree_amd.compare import quartet_positions
    pos = quartet_positions(len(ids_x), samples=1_000_000, seed=SEED)
    want = table_by_topologies(T1, T2, ids_x[pos], ids_y[pos])
    got = T1.compare_quartets(T2, leaves=(ids_x, ids_y), samples=1_000_000, seed=SEED).table
    print(json.dumps({"what": "check", "samples": 1_000_000, "tables_equal": bool(np.array_equal(got, want)), "table": got.tolist()}), flush=True)

    # the two paths alternate, size by size
    lines = {}
    yard = [int(float(s)) for s in a.yardstick.split(",") if s]
    for n in sorted(set(sizes) | set(yard)):
        if n in sizes:
            lines[n] = new_path(T1, T2, ids_x, ids_y, n, a.reps)
        if n in yard:
            y = yardstick(T1, T2, ids_x, ids_y, n)
            if n in lines:
                y["new_path_wall_s"] = lines[n]["wall_s"]
                y["yardstick_over_new"] = y["wall_s"] / lines[n]["wall_s"]
            print(json.dumps(y), flush=True)
    prof = {} if a.no_profile else profile(sizes)
    rates = None if a.no_rates else mrca_rates(T1, T2, ids_x, ids_y)
    for n in sizes:
        seg = prof.get(n)
        if seg:
            lines[n].update(device_s=seg["device_s"], draw_s=seg["draw_ns"] * 1e-9, mrca_s=seg["mrca_ns"] * 1e-9,
                            agree_s=seg["agree_ns"] * 1e-9, mrca_kernels=seg["mrca_kernels"])
        print(json.dumps(lines[n]), flush=True)
    if "error" in prof:
        print(json.dumps({"what": "profile", **prof}), flush=True)
    if rates:
        line = {"what": "mrca_rate", "ml_ids_per_s": rates["ml"], "nj_ids_per_s": rates["nj"], "ratio_ideal_over_measured": {}}
        for n in sizes:
            ideal = 6 * n / rates["ml"] + 6 * n / rates["nj"]
            line["ratio_ideal_over_measured"][str(n)] = {"ideal_s": ideal, "over_wall": ideal / lines[n]["wall_s"],
                                                         "over_device": ideal / lines[n]["device_s"] if "device_s" in lines[n] else None}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
