#!/usr/bin/env python3
"""LRU model of one XCD's L2 under a kernel that gathers from a table and streams its pairs and results.

    python scripts/l2_lru_model.py                       # the table of LAB_NOTES.md 9 (2^20 / 2^19 / 2^18 leaves)
    python scripts/l2_lru_model.py --table-bytes 8388608 --cache-bytes 4194304 --stream-in 16 --stream-out 12

The cache is fully associative with true LRU replacement and lines of --line-bytes.  Per pair it sees
  * two reads of table lines drawn uniformly from the table (the two nodes of a random pair),
  * --stream-in bytes of a pair array read front to back: every line-bytes / stream-in pairs a line nobody asks for again,
  * --stream-out bytes of result arrays written front to back, likewise.
A stream line that allocates enters at the most-recently-used end and pushes the least-recently-used line out; with
--bypass it does not enter the cache at all (what a non-temporal load or store is meant to achieve: either no allocation
or one marked for early eviction).  Reported: the hit rate of the table reads and the fabric reads per pair,
2 x (1 - hit rate) + stream-in / line-bytes (a stream-in line is fetched once whether it allocates or not; stream-out
lines are written, not read).

Uniform random reads make an LRU cache of C lines over a table of T > C lines hit C / T of the time, and no replacement
policy does better; the streams lower that because every one of their lines takes a table line's place for a full trip
through the LRU order.  CPU only, standard library only.
"""
import argparse
import json
import random
from collections import OrderedDict


def simulate(table_lines, cache_lines, stream_in=16.0, stream_out=12.0, line_bytes=128.0, bypass=False, pairs=None, seed=0):
    """Hit rate of the table reads and fabric reads per pair.  `pairs`: pairs counted after a warm-up of four cache fills
    (default: enough for a standard error of the hit rate below 0.001)."""
    rng = random.Random(seed)
    cache = OrderedDict()
    if pairs is None:
        pairs = max(200_000, 8 * cache_lines)
    warm = 4 * cache_lines
    share = 0.0 if bypass else (stream_in + stream_out) / line_bytes      # stream lines that allocate, per pair
    acc, stream_id = 0.0, -1
    hits = reads = 0
    move, pop, rand = cache.move_to_end, cache.popitem, rng.randrange
    for k in range(warm + pairs):
        counted = k >= warm
        for _ in range(2):
            line = rand(table_lines)
            if line in cache:
                move(line)
                hits += counted
            else:
                cache[line] = None
                if len(cache) > cache_lines:
                    pop(last=False)
            reads += counted
        acc += share
        while acc >= 1.0:      # a fresh stream line: allocated, never asked for again
            acc -= 1.0
            cache[stream_id] = None
            stream_id -= 1
            if len(cache) > cache_lines:
                pop(last=False)
    hit = hits / reads
    return {"table_lines": table_lines, "cache_lines": cache_lines, "streams_allocate": not bypass,
            "stream_lines_per_pair": (stream_in + stream_out) / line_bytes, "line_hit_rate": hit,
            "fabric_reads_per_pair": 2.0 * (1.0 - hit) + stream_in / line_bytes, "pairs": pairs}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--table-bytes", type=int, action="append", help="gathered table; repeatable (default: 8, 4 and 2 MiB of heap lines)")
    ap.add_argument("--cache-bytes", type=int, default=4 << 20, help="one XCD's L2 (default 4 MiB)")
    ap.add_argument("--line-bytes", type=int, default=128)
    ap.add_argument("--stream-in", type=float, default=16.0, help="bytes of pairs read per pair (default 16: int64 x 2)")
    ap.add_argument("--stream-out", type=float, default=12.0, help="bytes of results written per pair (default 12: float64 + int32)")
    ap.add_argument("--scale", type=int, default=8, help="divide table and cache by this (the model depends on their ratio only; default 8)")
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args(argv)
    rows = []
    for table in args.table_bytes or [8 << 20, 4 << 20, 2 << 20]:
        for bypass in (False, True):
            r = simulate(max(1, table // args.line_bytes // args.scale), max(1, args.cache_bytes // args.line_bytes // args.scale),
                         args.stream_in, args.stream_out, args.line_bytes, bypass, args.pairs, args.seed)
            r["table_bytes"], r["cache_bytes"] = table, args.cache_bytes
            rows.append(r)
    if args.json:
        print(json.dumps(rows))
        return rows
    print("%12s %12s %-18s %14s %22s" % ("table bytes", "cache bytes", "streams", "line hit rate", "fabric reads per pair"))
    for r in rows:
        print("%12d %12d %-18s %14.3f %22.3f" % (r["table_bytes"], r["cache_bytes"], "allocate in L2" if r["streams_allocate"] else "bypass L2",
                                                  r["line_hit_rate"], r["fabric_reads_per_pair"]))
    return rows


if __name__ == "__main__":
    main()
