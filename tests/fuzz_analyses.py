"""Seeded fuzz of the array-level analyses: the set passes (dispersion, beta dispersion, UniFrac, the UniFrac null), Mantel,
clade matching, Kendall's counts and the keyed permutation.  Generators and checkers only: tests/test_fuzz_analyses_host.py
runs the "host" layer (the library's host forms against the independent references under tests/, small sizes, no GPU) and
tests/test_gpu_fuzz_analyses.py the "device" layer (the kernels against the host restatement on the same arguments, bytes
and integers compared exactly, wider sizes, the form-switching environment variables drawn per case).

Case c of a session draws from np.random.default_rng([seed, family index, c]), so one case replays alone.  A session is a
fixed number of cases and counts, from the drawn arguments and the layout rules of the plan headers restated below (cut,
the size classes), which situations it reached: run() fails when one of REQUIRED is missing.  By hand:
  python tests/fuzz_analyses.py FAMILY [cases] [seed] [host|device] [first case]"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
from suchtree_amd import _capi, compare, synth      # noqa: E402

FAMILIES = ("dispersion", "beta", "unifrac", "null", "mantel", "clade", "kendall", "permutation")
LANE, WINDOW, GATHER = "SUCHTREE_AMD_UNIFRAC_LANE_MAX", "SUCHTREE_AMD_CLADE_MATCH_WINDOW", "SUCHTREE_AMD_MANTEL_GATHER"
TILE = 2048      # ST_KENDALL_TILE

# n_max: universes in general; large: one case in sixteen draws 2049 .. large; huge: where no n x n matrix is held;
# perms: permutations; work: inner steps of the yardstick per case; chunks: launches' worth of chunks per case
LAYERS = {
    "host": {"device": -1, "n_max": 256, "large": 0, "huge": 0, "mantel": 40, "mantel_huge": 0, "perms": 6, "work": 1.0e4, "chunks": 1 << 30},
    "device": {"device": 0, "n_max": 2100, "large": 8300, "huge": 16384, "mantel": 2100, "mantel_huge": 8660, "perms": 40, "work": 2.0e7,
               "chunks": 400},
}

# ---- the layout rules of the plan headers, restated (dispersion_plan.h, mantel_plan.h, unifrac_plan.h) ----


def cut(n_univ, rows, live, chunk_tasks, table_entries=0, block_cap=None):
    """(perm_block, [(p_begin, n_perms, task_begin, n_tasks)]) of dispersion_cut / mantel_plan"""
    block = (64 << 20) // (2 * (n_univ + table_entries))
    if block_cap is not None:
        block = min(block, block_cap)
    block, cap = max(1, block), 1 << 20
    if chunk_tasks > 0:
        block, cap = min(block, chunk_tasks), min(chunk_tasks, 1 << 30)
    perm_block = min(block, rows)
    chunks = []
    if live:
        for p0 in range(0, rows, perm_block):
            n_p = min(perm_block, rows - p0)
            chunks += [(p0, n_p, t, min(cap, live * n_p - t)) for t in range(0, live * n_p, cap)]
    return perm_block, chunks


def n_chunks(n_univ, rows, live, chunk_tasks, table_entries=0, block_cap=None):
    """len(cut(...)[1]) without the list"""
    block = (64 << 20) // (2 * (n_univ + table_entries))
    if block_cap is not None:
        block = min(block, block_cap)
    block, cap = max(1, block), 1 << 20
    if chunk_tasks > 0:
        block, cap = min(block, chunk_tasks), min(chunk_tasks, 1 << 30)
    perm_block = min(block, rows)
    full, rest = divmod(rows, perm_block)
    return full * -(-live * perm_block // cap) + (-(-live * rest // cap) if rest else 0)


def size_class(k):
    """dispersion_class: K' = 2, 4, .. 64 are classes 0 .. 5, more than 64 positions class 6"""
    return 6 if k > 64 else max(0, (k - 1).bit_length() - 1)


def triangle(n_sets):
    return [(i, j) for i in range(n_sets) for j in range(i)]


# ---- draws shared by the families ----


def _seed64(rng):
    return int(rng.integers(0, 1 << 64, dtype=np.uint64))


def _stream(rng):
    return int(rng.integers(0, 1 << 31)) if rng.integers(2) else 0


def _universe(rng, L, lo, top=None, huge=0):
    top = top or L["n_max"]
    if L["large"] and rng.integers(16) == 0:
        return int(rng.integers(2049, (huge if huge and rng.integers(3) == 0 else L["large"]) + 1))
    u = int(rng.integers(4))
    if u == 0:
        return int(rng.integers(lo, min(64, top) + 1))
    if u == 1:
        k = int(rng.integers(2, int(math.log2(top)) + 1))
        return int(min(top, max(lo, (1 << k) + int(rng.integers(-1, 2)))))
    return int(min(top, max(lo, round(2.0 ** rng.uniform(math.log2(lo), math.log2(top))))))


def _size(rng, n):
    """0, 1 and 2; the whole universe; 2^k - 1, 2^k, 2^k + 1; log-uniform up to n"""
    u = int(rng.integers(10))
    if u < 3:
        return min(n, int(rng.integers(0, 3)))
    if u == 3:
        return n
    if u < 7:
        k = int(rng.integers(1, max(1, n.bit_length() - 1) + 1))
        return min(n, max(0, (1 << k) + int(rng.integers(-1, 2))))
    return min(n, int(2.0 ** rng.uniform(0.0, math.log2(n + 1))))


def _sets(rng, n, n_sets):
    """sorted position sets; sometimes a copy of an earlier one, sometimes a prefix of one"""
    sets = []
    for _ in range(n_sets):
        u = int(rng.integers(12))
        if sets and u == 0:
            sets.append(sets[int(rng.integers(len(sets)))].copy())
        elif sets and u == 1:
            s = sets[int(rng.integers(len(sets)))]
            sets.append(s[: int(rng.integers(0, len(s) + 1))].copy())
        else:
            sets.append(np.sort(rng.choice(n, _size(rng, n), replace=False)).astype(np.int64))
    return sets


def _halve_largest(sets):
    i = max(range(len(sets)), key=lambda r: len(sets[r]))
    sets[i] = sets[i][: len(sets[i]) // 2]


def _chunk_kind(rng):
    return int(rng.integers(4)), int(rng.integers(2, 50)), int(rng.integers(1, 100))


def _chunk(kind, tasks, count, bound):
    """0, 1, a small value or one above the task count; a cut into more than `bound` chunks is coarsened"""
    u, small, above = kind
    chunk = (0, 1, small, tasks + above)[u]
    while chunk > 0 and count(chunk) > bound:
        chunk *= 2
    return chunk


def _range(rng, total):
    if rng.integers(3) == 0:
        return 0, total
    begin = int(rng.integers(0, total + 1))
    return begin, int(rng.integers(0, total - begin + 1))


def _toggles(rng):
    lane = (None, "0", "8", str(int(rng.integers(1, 300))))[int(rng.integers(4))]
    return {LANE: lane, WINDOW: (None, "0", "1")[int(rng.integers(3))], GATHER: (None, "1")[int(rng.integers(2))]}


def _lane_max(env):
    return 512 if env[LANE] is None else int(env[LANE])


def _matrix(rng, n, special):
    """float32 distances as a tree's would be: positive, a few orders of magnitude, not symmetric; `special`: NaN, +inf,
    -0.0 and 0.0 sprinkled over it"""
    D = (1.0 - rng.random((n, n), dtype=np.float32)) * (10.0 ** rng.integers(-2, 2, n)).astype(np.float32)[:, None]
    if special:
        c = min(200000, max(4, n * n // 10))
        D[rng.integers(0, n, c), rng.integers(0, n, c)] = rng.choice(np.float32([np.nan, np.inf, -0.0, 0.0]), c)
    return D


def _first_diff(got, want, what):
    """None where the two arrays hold the same bytes, else the first cell that differs"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "%s: shape %s %s against %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.tobytes() == want.tobytes():
        return None
    size = got.dtype.itemsize
    bad = np.flatnonzero((got.reshape(-1).view(np.uint8).reshape(-1, size) != want.reshape(-1).view(np.uint8).reshape(-1, size)).any(axis=1))
    at = np.unravel_index(int(bad[0]), got.shape)
    return "%s: %d cells differ, first %s: got %s want %s" % (what, len(bad), tuple(int(v) for v in at), got[at], want[at])


def _kind(v):
    return "nan" if math.isnan(v) else "+inf" if v == math.inf else "-inf" if v == -math.inf else "finite"


def _float_check(got, want, rel, special, what):
    """the stated bound on a sum of positive terms, or where special values are about only where NaN and inf occur"""
    if special or want == 0.0:
        return None if (_kind(got) == _kind(want) and (special or got == 0.0)) else "%s: got %r want %r" % (what, got, want)
    return None if abs(got - want) <= rel * want else "%s: got %r want %r, bound %.3g relative" % (what, got, want, rel)


# ---- dispersion and beta dispersion ----


def _record_draw(rng, L, beta):
    n = _universe(rng, L, 3)
    sets = _sets(rng, n, int(rng.integers(2 if beta else 1, 11)))
    perms = int(rng.integers(0, L["perms"] + 1))
    case = {"n": n, "seed": _seed64(rng), "stream": _stream(rng), "special": bool(rng.integers(5) == 0), "env": _toggles(rng)}
    kind = _chunk_kind(rng)
    pairs = triangle(len(sets))
    if beta:
        case["begin"], case["count"] = _range(rng, len(pairs))
        case["exclude"] = bool(rng.integers(2))
        if case["count"] and rng.integers(4) == 0:      # a one-member set equal to its partner
            i, j = pairs[case["begin"]]
            sets[i] = sets[j] = np.array([int(rng.integers(n))], dtype=np.int64)
        mine = pairs[case["begin"]: case["begin"] + case["count"]]
        steps = lambda: sum(2 * len(sets[i]) * len(sets[j]) for i, j in mine)      # noqa: E731
    else:
        steps = lambda: sum(len(s) ** 2 for s in sets)      # noqa: E731
    while steps() * (perms + 1) > L["work"] and perms > 2:
        perms //= 2
    while steps() * (perms + 1) > L["work"]:
        _halve_largest(sets)
    if beta:
        sizes = [(len(sets[r]), len(sets[c])) for i, j in mine for r, c in ((i, j), (j, i))]
        live = [size_class(kr) if kr >= 2 else 0 for kr, kc in sizes if kr and kc]
    else:
        live = [size_class(len(s)) for s in sets if len(s) >= 2]
    case["classes"] = [live.count(k) for k in range(7)]
    case["sets"], case["perms"] = sets, perms
    case["chunk"] = _chunk(kind, len(live) * (perms + 1), lambda c: n_chunks(n, perms + 1, len(live), c), L["chunks"])
    return case


def _record_census(case, C, beta):
    n, rows, classes = case["n"], case["perms"] + 1, case["classes"]
    begin = np.concatenate([[0], np.cumsum(classes)])
    perm_block, chunks = cut(n, rows, int(begin[-1]), case["chunk"])
    C["form packed"] += any(classes[:5])
    C["form wave"] += classes[5] > 0
    C["form workgroup"] += classes[6] > 0
    C["sort class " + ("wave" if n <= 64 else "small" if n <= 2048 else "large")] += 1
    C["two permutation blocks"] += bool(chunks) and rows > perm_block
    C["chunk starts in mid-set"] += any(t % n_p for _, n_p, t, _ in chunks)
    C["chunk spans two size classes"] += any(
        sum(max(t, begin[k] * n_p) < min(t + c, begin[k + 1] * n_p) for k in range(7)) >= 2 for _, n_p, t, c in chunks)
    C["special values"] += case["special"]
    if beta:
        sets, pairs = case["sets"], triangle(len(case["sets"]))[case["begin"]: case["begin"] + case["count"]]
        C["exclude_shared on"] += case["exclude"]
        C["exclude_shared off"] += not case["exclude"]
        C["one-member set equal to its partner, excluded"] += case["exclude"] and any(
            len(sets[i]) == 1 and len(sets[j]) == 1 and sets[i][0] == sets[j][0] for i, j in pairs)
        C["range begins in mid-row"] += case["count"] > 0 and triangle(len(sets))[case["begin"]][1] != 0


def _dispersion_check(case, rng, L):
    import dispersion_reference
    n, sets, perms, special = case["n"], case["sets"], case["perms"], case["special"]
    D = _matrix(rng, n, special)
    args = (D, sets, perms, case["seed"], case["stream"])
    got = _capi.dispersion_matrix(*args, device=L["device"], chunk_tasks=case["chunk"])
    if L["device"] >= 0:
        return _first_diff(got, _capi.dispersion_matrix(*args, device=-1), "record (set, p)")
    for p in range(perms + 1):
        sigma = compare.hommola_permutation(case["seed"], case["stream"], p, 0, n)
        for r, s in enumerate(sets):
            k = len(s)
            want = dispersion_reference.plain(D, sigma[s])
            for name, w, rel in (("pair_sum", want[0], k * k * 2.0 ** -52), ("nearest_sum", want[1], k * 2.0 ** -52)):
                bad = _float_check(float(got[r, p][name]), w, rel, special, "%s of set %d (k %d) under p %d" % (name, r, k, p))
                if bad:
                    return bad
    return None


def _beta_special(D, sigma, s_r, s_c, exclude):
    """(cross, nearest) of a direction where NaN and inf are about: plain float64 sums, the minimum by v < m ? v : m"""
    if len(s_r) == 0 or len(s_c) == 0:
        return 0.0, 0.0
    sub = D[np.ix_(sigma[s_r], sigma[s_c])].astype(np.float64)
    keep = s_r[:, None] != s_c[None, :] if exclude else np.ones(sub.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        mins = np.where(keep & ~np.isnan(sub), sub, np.inf).min(axis=1)[keep.any(axis=1)]
        return float(sub[keep].sum()), float(mins.sum())


def _beta_check(case, rng, L):
    import beta_dispersion_reference as ref
    n, sets, perms, special, exclude = case["n"], case["sets"], case["perms"], case["special"], case["exclude"]
    D = _matrix(rng, n, special)
    args = (D, sets, case["begin"], case["count"], exclude, perms, case["seed"], case["stream"])
    got = _capi.beta_dispersion_matrix(*args, device=L["device"], chunk_tasks=case["chunk"])
    if L["device"] >= 0:
        return _first_diff(got, _capi.beta_dispersion_matrix(*args, device=-1), "record (pair, direction, p)")
    for p in range(perms + 1):
        sigma = compare.hommola_permutation(case["seed"], case["stream"], p, 0, n)
        for k, (i, j) in enumerate(ref.pairs(len(sets), case["begin"], case["count"])):
            for d, (r, c) in enumerate(((i, j), (j, i))):
                kr, kc = len(sets[r]), len(sets[c])
                want = _beta_special(D, sigma, sets[r], sets[c], exclude) if special else ref.direction(D, sigma, sets[r], sets[c], exclude)
                for name, w, rel in (("pair_sum", want[0], kr * kc * 2.0 ** -52), ("nearest_sum", want[1], kr * 2.0 ** -52)):
                    bad = _float_check(float(got[k, d, p][name]), w, rel, special,
                                       "%s of pair %d (%d, %d) direction %d (k %d, %d) under p %d" % (name, k, i, j, d, kr, kc, p))
                    if bad:
                        return bad
    return None


# ---- UniFrac and its null ----


def _fast_depths(parent, depth, leaf_node):
    """unifrac_cases.depths in O(nodes): the MRCA of two adjacent leaves is the node whose children they end and begin"""
    first = np.full(len(parent), len(leaf_node), dtype=np.int64)
    first[leaf_node] = np.arange(len(leaf_node))
    h = np.zeros(max(len(leaf_node) - 1, 0), dtype=np.int64)
    par, lo = parent.tolist(), first.tolist()
    for v in range(len(par) - 1, 0, -1):
        if lo[v] < lo[par[v]]:
            lo[par[v]] = lo[v]
    for v in range(1, len(par)):      # the child that does not begin its parent's range begins at the boundary
        if lo[v] != lo[par[v]]:
            h[lo[v] - 1] = depth[par[v]]
    return depth[leaf_node].copy(), h


def _unifrac_draw(rng, L, null):
    u = int(rng.integers(10))
    n = _universe(rng, L, 3 if null else 1, huge=L["huge"] if null else 0) if null or u > 1 else u + 1      # (n = 1 and 2: unifrac alone)
    sets = _sets(rng, n, int(rng.integers(0 if rng.integers(20) == 0 else 1, 13)))
    case = {"n": n, "tree_seed": int(rng.integers(1 << 31)), "env": _toggles(rng)}
    case["begin"], case["count"] = _range(rng, len(sets) * (len(sets) - 1) // 2)
    kind = _chunk_kind(rng)
    mine = lambda: triangle(len(sets))[case["begin"]: case["begin"] + case["count"]]      # noqa: E731
    per_step = 1 if null or L["device"] >= 0 else 20      # (the brute force walks every member to the root, in Python)
    perms = 0
    if null:
        perms = int(rng.integers(0, L["perms"] + 1))
        case["seed"], case["stream"] = _seed64(rng), _stream(rng)
        case["pd"], case["union"] = ((True, True), (True, False), (False, True))[int(rng.integers(3))]
    steps = lambda: per_step * (sum(2 * len(s) for s in sets) + sum(len(sets[i]) + len(sets[j]) for i, j in mine())) + (n if null else 0)      # noqa: E731
    while steps() * (perms + 1) > L["work"] and perms > 2:
        perms //= 2
    while steps() * (perms + 1) > L["work"] and any(len(s) > 1 for s in sets):
        _halve_largest(sets)
    case["sets"] = sets
    if null:
        case["perms"] = perms
        items = len(sets) + (case["count"] if case["union"] else 0)
        case["items"], case["n_tab"] = items, sum(len(s) for s in sets) if case["union"] else 0
        case["chunk"] = _chunk(kind, items * (perms + 1), lambda c: n_chunks(n, perms + 1, items, c, case["n_tab"]), L["chunks"])
    else:
        tasks = len(sets) + case["count"]
        case["chunk"] = _chunk(kind, tasks, lambda c: -(-len(sets) // c) - (-case["count"] // c), L["chunks"])
    return case


def _unifrac_census(case, C, null):
    sets, lane_max = case["sets"], _lane_max(case["env"])
    pairs = triangle(len(sets))[case["begin"]: case["begin"] + case["count"]]
    heavy = [len(sets[i]) + len(sets[j]) > lane_max for i, j in pairs]
    C["empty set"] += any(len(s) == 0 for s in sets)
    C["lane threshold from the environment"] += case["env"][LANE] is not None
    if not null:
        C["n = 1"] += case["n"] == 1
        C["n = 2"] += case["n"] == 2
        cap = case["chunk"] or 1 << 22
        own = [2 * len(s) > lane_max for s in sets]
        both = lambda v: any(any(v[t: t + cap]) and not all(v[t: t + cap]) for t in range(0, len(v), cap))      # noqa: E731
        C["light and heavy tasks in one chunk"] += both(own) or both(heavy)
        return
    C["pd only"] += case["pd"] and not case["union"]
    C["union only"] += case["union"] and not case["pd"]
    C["pd and union"] += case["pd"] and case["union"]
    C["more than 64 bitmap words"] += case["n"] > 4096
    perm_block, chunks = cut(case["n"], case["perms"] + 1, case["items"], case["chunk"], case["n_tab"])
    C["two permutation blocks"] += bool(chunks) and case["perms"] + 1 > perm_block
    for _, n_p, t, c in chunks:
        lo, hi = max(t, len(sets) * n_p), t + c      # the chunk's pair tasks
        if hi > lo:
            mine = heavy[lo // n_p - len(sets): (hi - 1) // n_p - len(sets) + 1]
            C["light and heavy tasks in one chunk"] += any(mine) and not all(mine)
            C["chunk ends between the rows of one pair"] += hi % n_p != 0
            C["chunk holds set and pair tasks"] += t < len(sets) * n_p


def _unifrac_check(case, rng, L):
    import unifrac_cases
    n, sets = case["n"], case["sets"]
    parent, depth, leaf_node = unifrac_cases.random_tree(n, case["tree_seed"])
    d, h = _fast_depths(parent, depth, leaf_node)
    args = (d, h, sets, case["begin"], case["count"])
    got = _capi.unifrac_depths(*args, device=L["device"], chunk_pairs=case["chunk"])
    if L["device"] >= 0:
        want = _capi.unifrac_depths(*args, device=-1)
    else:
        slow = unifrac_cases.depths(parent, depth, leaf_node)
        if not (np.array_equal(slow[0], d) and np.array_equal(slow[1], h)):
            return "the harness's own depths differ from unifrac_cases.depths"
        pd, union = unifrac_cases.brute_force(parent, depth, leaf_node, sets)
        want = (pd, union[case["begin"]: case["begin"] + case["count"]])
    return _first_diff(got[0], want[0], "pd of set") or _first_diff(got[1], want[1], "union sum of pair")


def _null_check(case, rng, L):
    import unifrac_null_reference as ref
    d, h = ref.depths(case["n"], case["tree_seed"])
    args = (d, h, case["sets"], case["begin"], case["count"], case["perms"], case["seed"], case["stream"])
    got = _capi.unifrac_null_depths(*args, device=L["device"], chunk_tasks=case["chunk"], pd=case["pd"], union=case["union"])
    if L["device"] >= 0:
        want = _capi.unifrac_null_depths(*args, device=-1)
    else:
        want = ref.compose(d, h, case["sets"], case["perms"], case["seed"], case["stream"], case["begin"], case["count"])
    for k, (on, what) in enumerate(((case["pd"], "pd (set, p)"), (case["union"], "union sum (pair, p)"))):
        if not on and got[k] is not None:
            return "%s came back though it was not asked for" % what
        bad = on and _first_diff(got[k], want[k], what)
        if bad:
            return bad
    return None


# ---- Mantel ----


def _mantel_draw(rng, L):
    n = _universe(rng, L, 3, top=L["mantel"], huge=L["mantel_huge"])
    perms = int(rng.integers(0, L["perms"] + 1))
    case = {"n": n, "regime": ("full", "small", "pool")[int(rng.integers(3))], "z": bool(rng.integers(2)), "seed": _seed64(rng),
            "stream": _stream(rng), "env": _toggles(rng)}
    kind = _chunk_kind(rng)
    while n * n * (2 if L["device"] < 0 else 0.5) * (perms + 1) > L["work"] and perms > 1:
        perms //= 2
    items = 1 if n <= 64 else (n + 1) // 2
    case["perms"], case["items"] = perms, items
    case["chunk"] = _chunk(kind, items * (perms + 1), lambda c: n_chunks(n, perms + 1, items, c, 0, (1 << 22) // items), L["chunks"])
    return case


def _mantel_census(case, C):
    n, rows, rowform = case["n"], case["perms"] + 1, case["n"] > 64
    perm_block, chunks = cut(n, rows, case["items"], case["chunk"], 0, (1 << 22) // case["items"])
    C["wave form"] += not rowform
    C["row form"] += rowform
    C["odd n in the row form"] += rowform and n % 2 == 1
    for r in range(4):
        C["n mod 4 = %d in the row form" % r] += rowform and n % 4 == r
    C["with z"] += case["z"]
    C["without z"] += not case["z"]
    C["two permutation blocks"] += rows > perm_block
    C["a short last block in the row form"] += rowform and rows > perm_block and rows % perm_block != 0
    C["gather form"] += rowform and case["env"][GATHER] == "1"
    C["chunk starts in mid-item"] += any(t % n_p for _, n_p, t, _ in chunks)
    C["sort class " + ("wave" if n <= 64 else "small" if n <= 2048 else "large")] += 1
    C["codes " + case["regime"]] += 1


def _codes(rng, regime, shape, symmetric):
    """int32 codes: the full range, -3 .. 3, or a pool of the extremes; symmetric: a + a^T of one draw, mapped"""
    pool = np.array([-(1 << 31), (1 << 31) - 1, 0, 1, -1], dtype=np.int64).astype(np.int32)
    if regime == "full":
        a = rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)
        return a + a.T if symmetric else a      # (int32 wraps: still uniform)
    if regime == "small":
        a = rng.integers(0, 4, shape, dtype=np.int32) if symmetric else rng.integers(-3, 4, shape, dtype=np.int32)
        return a + a.T - 3 if symmetric else a
    a = rng.integers(0, 5, shape, dtype=np.int32)
    return pool[(a + a.T) % 5] if symmetric else pool[a]


def _mantel_check(case, rng, L):
    import mantel_reference as ref
    n, perms = case["n"], case["perms"]
    m = n * (n - 1) // 2
    x = _codes(rng, case["regime"], (n, n), True)
    y = _codes(rng, case["regime"], m, False)
    z = _codes(rng, case["regime"], m, False) if case["z"] else None
    args = (x, y, z, perms, case["seed"], case["stream"])
    got = _capi.mantel_codes(*args, device=L["device"], chunk_tasks=case["chunk"])
    if L["device"] >= 0:
        want = _capi.mantel_codes(*args, device=-1)
        if got[0] != want[0]:
            return "moments: got %s want %s" % (got[0], want[0])
        return _first_diff(got[1], want[1], "record p")
    want = ref.moments(x, y, z)
    if got[0] != want:
        return "moments: got %s want %s" % (got[0], want)
    mine = list(zip(_capi.mantel_ints(got[1], "sxy"), _capi.mantel_ints(got[1], "sxz")))
    for p, (g, w) in enumerate(zip(mine, ref.records(x, y, z, perms, case["seed"], case["stream"]))):
        if g != w:
            return "record %d: got %s want %s" % (p, g, w)
    return None


# ---- clade matching ----


def _tree_ranges(rng, m, ids, rooted):
    parent, _ = synth.random_binary_tree_levels(m, seed=int(rng.integers(1 << 31)))      # (in-order ids: the leaves are the even ones)
    order, _, lo, hi = _capi.clade_ranges(parent, ids, rooted)
    return order, lo, hi


def _any_ranges(rng, m, count):
    lo = rng.integers(0, m, count)
    hi = lo + 1 + ((m - lo) * rng.random(count) ** 2).astype(np.int64)
    return lo.astype(np.int32), np.minimum(hi, m).astype(np.int32)


def _clade_draw(rng, L):
    u = int(rng.integers(5))
    if u < 2:
        m = 64 * int(rng.integers(1, L["n_max"] // 64 + 1)) + int(rng.integers(-1, 2))
    else:
        m = _universe(rng, L, 4)
    case = {"m": m, "rooted": bool(rng.integers(2)), "env": _toggles(rng)}
    from_a, from_b = int(rng.integers(2)), int(rng.integers(3))      # a tree's clades / arbitrary ranges (/ no candidates)
    ids = 2 * rng.permutation(m).astype(np.int64)
    order_a = order_b = None
    if from_a == 0:
        order_a, a_lo, a_hi = _tree_ranges(rng, m, ids, case["rooted"])
    else:
        a_lo, a_hi = _any_ranges(rng, m, 0 if rng.integers(20) == 0 else int(rng.integers(1, 2 * m)))
    if from_b == 0:
        order_b, b_lo, b_hi = _tree_ranges(rng, m, ids, case["rooted"])
    else:
        b_lo, b_hi = _any_ranges(rng, m, 0 if from_b == 2 else int(rng.integers(1, 2 * m)))
    if order_a is not None and order_b is not None:      # the leaf at A's position k sits at B's position pos_b[k]
        where_b = np.empty(m, dtype=np.int32)
        where_b[order_b] = np.arange(m, dtype=np.int32)
        pos_b = where_b[order_a]
    else:
        pos_b = rng.permutation(m).astype(np.int32)
    kind = _chunk_kind(rng)
    # the yardstick's steps: a prefix count and a scan per row (restatement), or a set intersection per row and candidate
    if L["device"] >= 0:
        rows = int(L["work"] // (m + len(b_lo) + 1))
    else:
        cands = max(1, int(math.sqrt(30 * L["work"] / (m / 4 + 8))))
        keep = np.sort(rng.choice(len(b_lo), min(len(b_lo), cands), replace=False))
        b_lo, b_hi, rows = b_lo[keep], b_hi[keep], cands
    keep = np.sort(rng.choice(len(a_lo), min(len(a_lo), max(rows, 1)), replace=False))
    a_lo, a_hi = a_lo[keep], a_hi[keep]
    case.update(pos_b=pos_b, a_lo=a_lo, a_hi=a_hi, b_lo=b_lo, b_hi=b_hi, source="%s rows, %s candidates" % (
        ("tree", "arbitrary")[from_a], ("tree", "arbitrary", "no")[from_b]))
    case["chunk"] = _chunk(kind, len(a_lo), lambda c: -(-len(a_lo) // c), L["chunks"])
    return case


def _clade_census(case, C):
    m = case["m"]
    for r, name in ((63, "m one below a multiple of 64"), (0, "m a multiple of 64"), (1, "m one above a multiple of 64")):
        C[name] += m % 64 == r
    C["no candidates"] += len(case["b_lo"]) == 0 and len(case["a_lo"]) > 0
    C["rooted"] += case["rooted"]
    C["unrooted"] += not case["rooted"]
    C["more rows than a chunk"] += 0 < case["chunk"] < len(case["a_lo"])
    C["windows on"] += case["env"][WINDOW] != "0"
    C["windows off"] += case["env"][WINDOW] == "0"
    C[case["source"]] += 1


def _clade_check(case, rng, L):
    m = case["m"]
    args = (m, case["pos_b"], case["a_lo"], case["a_hi"], case["b_lo"], case["b_hi"], case["rooted"])
    got = _capi.clade_match(*args, device=L["device"], chunk_rows=case["chunk"])
    if L["device"] >= 0:
        want = _capi.clade_match(*args, device=-1)
    else:
        import clade_match_reference as ref
        at_b = np.empty(m, dtype=np.int64)      # at_b[x]: A's position of the leaf at B's position x
        at_b[case["pos_b"]] = np.arange(m)
        rows = [(None, frozenset(range(lo, hi))) for lo, hi in zip(case["a_lo"].tolist(), case["a_hi"].tolist())]
        cands = [(None, frozenset(at_b[lo:hi].tolist())) for lo, hi in zip(case["b_lo"].tolist(), case["b_hi"].tolist())]
        best = ref.match(rows, cands, m, case["rooted"])
        want = tuple(np.array([b[k] for b in best], dtype=np.int32) for k in range(3))
    for g, w, what in zip(got, want, ("distance of row", "match of row", "intersection of row")):
        bad = _first_diff(g, w, what)
        if bad:
            return bad
    return None


# ---- Kendall ----


def _column(rng, n, pool):
    v = ((rng.integers(0, pool, n) - pool // 2) * 0.5).astype(np.float32)      # (exact: below 2^24)
    if n and rng.integers(2):
        k = rng.integers(0, n, max(1, n // 8))
        v[k] = rng.choice(np.float32([0.0, -0.0, np.inf, -np.inf]), len(k))
    return v


def _kendall_draw(rng, L):
    u = int(rng.integers(10))
    if u < 4:
        n = int(rng.choice([0, 1, 2] if L["device"] < 0 else [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1]))
    elif u < 6 and L["large"]:
        n = int(rng.integers(TILE + 1, L["large"] + 1))
    else:
        n = int(2.0 ** rng.uniform(1.0, math.log2(L["n_max"])))
    pool = (2, 3, 10, 1 << 20)[int(rng.integers(4))]
    if n > TILE and rng.integers(2):      # (a tie group that holds a whole tile needs few values among many keys)
        pool = 2
    x, other = _column(rng, n, pool), _column(rng, n, pool)
    y = np.where(rng.random(n) < 0.5, x, other).astype(np.float32) if rng.integers(2) else other
    nan = n > 0 and rng.integers(8) == 0
    if nan:
        (x if rng.integers(2) else y)[rng.integers(0, n, int(rng.integers(1, 4)))] = np.nan
    return {"n": n, "pool": pool, "nan": bool(nan), "x": x, "y": y, "env": _toggles(rng)}


def _kendall_census(case, C):
    n = case["n"]
    for v, name in ((0, "n = 0"), (1, "n = 1"), (TILE - 1, "one tile less one"), (TILE, "one tile"), (TILE + 1, "one tile and one")):
        C[name] += n == v
    C["a NaN"] += case["nan"]
    C["more than one tile"] += n > TILE
    if n and not case["nan"]:
        C["tie group wider than a tile"] += int(np.unique(case["x"], return_counts=True)[1].max()) > TILE
        xs = np.sort(case["x"])      # a tile of the sorted keys that lies inside one tie group: its block has no run start
        C["a tile without a run start"] += any(xs[b - 1] == xs[min(b + TILE, n) - 1] for b in range(TILE, n, TILE))


def _kendall_check(case, rng, L):
    import kendall_reference as ref
    x, y = case["x"], case["y"]
    if L["device"] >= 0:
        got, want = _capi.kendall_arrays_host(x, y, device=L["device"]).as_tuple(), _capi.kendall_host(x, y).as_tuple()
        return None if got == want else "counts (n, n_nan, discordant, ties_x, ties_y, ties_xy): got %s want %s" % (got, want)
    got, want = _capi.kendall_host(x, y), ref.brute_counts(x, y)
    if got.as_tuple() != tuple(want):
        return "counts (n, n_nan, discordant, ties_x, ties_y, ties_xy): got %s want %s" % (got.as_tuple(), tuple(want))
    mine = ref.tau_b(ref.KendallRef(*got.as_tuple()))
    if case["n"] >= 2 and not case["nan"] and not math.isnan(mine):
        import scipy.stats
        theirs = float(scipy.stats.kendalltau(x, y).statistic)      # (a float formula over the same counts: a few ulps)
        if not abs(mine - theirs) <= 1e-12:
            return "tau-b from the counts %r, scipy's %r" % (mine, theirs)
    return None


# ---- the keyed permutation ----


def _permutation_draw(rng, L):
    n = 1 if rng.integers(12) == 0 else _universe(rng, L, 1, huge=L["huge"])
    return {"n": n, "seed": _seed64(rng), "node": int(rng.integers(0, 1 << 31)), "side": int(rng.integers(2)),
            "p": 0 if rng.integers(6) == 0 else int(rng.integers(1, 1 << int(rng.integers(1, 41)))), "env": _toggles(rng)}


def _permutation_census(case, C):
    n = case["n"]
    C["sort class " + ("wave" if n <= 64 else "small" if n <= 2048 else "large")] += 1
    C["more than 8 keys a lane"] += n > 8192
    C["p = 0"] += case["p"] == 0


def _permutation_check(case, rng, L):
    args = (case["seed"], case["node"], case["p"], case["side"], case["n"])
    host = _capi.hommola_permutation(*args, device=-1)
    if L["device"] >= 0:
        return _first_diff(_capi.hommola_permutation(*args, device=L["device"]), host, "position")
    if not np.array_equal(np.sort(host), np.arange(case["n"])):
        return "not a permutation of 0 .. n - 1"
    if case["p"] == 0 and not np.array_equal(host, np.arange(case["n"])):
        return "p = 0 is not the identity"
    return None


DRAW = {"dispersion": lambda r, L: _record_draw(r, L, False), "beta": lambda r, L: _record_draw(r, L, True),
        "unifrac": lambda r, L: _unifrac_draw(r, L, False), "null": lambda r, L: _unifrac_draw(r, L, True), "mantel": _mantel_draw,
        "clade": _clade_draw, "kendall": _kendall_draw, "permutation": _permutation_draw}
CENSUS = {"dispersion": lambda c, C: _record_census(c, C, False), "beta": lambda c, C: _record_census(c, C, True),
          "unifrac": lambda c, C: _unifrac_census(c, C, False), "null": lambda c, C: _unifrac_census(c, C, True), "mantel": _mantel_census,
          "clade": _clade_census, "kendall": _kendall_census, "permutation": _permutation_census}
CHECK = {"dispersion": _dispersion_check, "beta": _beta_check, "unifrac": _unifrac_check, "null": _null_check, "mantel": _mantel_check,
         "clade": _clade_check, "kendall": _kendall_check, "permutation": _permutation_check}

# What a session must have reached at least once.  The host layer's sizes stop at 256 (Mantel: 40), so what needs more --
# the large sort class, a tile of Kendall keys, 64 bitmap words, the row form -- is the device layer's alone.
_RECORDS = ["form packed", "form wave", "form workgroup", "two permutation blocks", "chunk starts in mid-set", "chunk spans two size classes",
            "special values", "sort class wave", "sort class small"]
_BETA = ["exclude_shared on", "exclude_shared off", "one-member set equal to its partner, excluded", "range begins in mid-row"]
_NULL = ["light and heavy tasks in one chunk", "empty set", "pd only", "union only", "pd and union", "chunk ends between the rows of one pair",
         "two permutation blocks"]
_CLADE = ["m one below a multiple of 64", "m a multiple of 64", "m one above a multiple of 64", "no candidates", "rooted", "unrooted",
          "more rows than a chunk", "windows on", "windows off"]
REQUIRED = {
    "host": {"dispersion": _RECORDS, "beta": _RECORDS + _BETA, "unifrac": ["light and heavy tasks in one chunk", "empty set", "n = 1", "n = 2"],
             "null": _NULL, "mantel": ["wave form", "with z", "without z", "two permutation blocks", "codes full", "codes small", "codes pool"],
             "clade": _CLADE, "kendall": ["n = 0", "n = 1", "a NaN"], "permutation": ["sort class wave", "sort class small", "p = 0"]},
    "device": {"dispersion": _RECORDS + ["sort class large"], "beta": _RECORDS + ["sort class large"] + _BETA,
               "unifrac": ["light and heavy tasks in one chunk", "empty set", "n = 1", "n = 2", "lane threshold from the environment"],
               "null": _NULL + ["more than 64 bitmap words", "lane threshold from the environment"],
               "mantel": ["wave form", "row form", "odd n in the row form"] + ["n mod 4 = %d in the row form" % r for r in range(4)]
               + ["with z", "without z", "two permutation blocks", "a short last block in the row form", "gather form", "sort class large",
                  "codes full", "codes small", "codes pool"],
               "clade": _CLADE,
               "kendall": ["n = 0", "n = 1", "one tile less one", "one tile", "one tile and one", "tie group wider than a tile", "a tile without a run start",
                           "a NaN"],
               "permutation": ["sort class wave", "sort class small", "sort class large", "more than 8 keys a lane", "p = 0"]},
}


class Census(dict):
    def __missing__(self, key):
        return 0


def case_rng(family, seed, c, families=FAMILIES):
    return np.random.default_rng([int(seed), families.index(family), int(c)])


def describe(case):
    """every drawn argument on one line: scalars as they are, sets by their sizes, other arrays by their lengths.  A key
    that begins with "_" is skipped: it is for what a family derives from its draws and keeps in the case (a layout, the
    oracle's columns), never for a drawn argument, which would then be missing from the replay line.  No family of this
    module has such a key."""
    out = []
    for k, v in case.items():
        if k == "env" or k.startswith("_"):
            continue
        if k == "sets":
            v = [len(s) for s in v]
        elif isinstance(v, np.ndarray):
            v = "<%d>" % len(v)
        out.append("%s=%s" % (k, v))
    return " ".join(out) + " env " + " ".join("%s=%s" % (k.replace("SUCHTREE_AMD_", ""), v) for k, v in case["env"].items())


def _tables(tables):
    """the family tables of a fuzz module (FAMILIES, LAYERS, DRAW, CENSUS, CHECK, REQUIRED): this module's by default"""
    return tables or sys.modules[__name__]


def census(family, seed, cases, layer, tables=None):
    """what a session would reach, from the draws alone: no library call but st_clade_ranges (clade, host only), no GPU"""
    T, C = _tables(tables), Census()
    for c in range(cases):
        T.CENSUS[family](T.DRAW[family](case_rng(family, seed, c, T.FAMILIES), T.LAYERS[layer]), C)
    return C


def missing(family, C, layer, tables=None):
    return [k for k in _tables(tables).REQUIRED[layer][family] if not C[k]]


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def run(family, seed, cases, layer, setenv=_setenv, first=0, require=True, tables=None):
    """One session of `cases` cases; returns its census.  A mismatch prints one line with everything needed to repeat it
    and raises; so does an entry that refuses its arguments, and a census without one of REQUIRED.  `tables`: another
    module's families (tests/fuzz_compare.py) under the same rules."""
    T = _tables(tables)
    L, C = T.LAYERS[layer], Census()
    for c in range(first, first + cases):
        rng = case_rng(family, seed, c, T.FAMILIES)
        case = T.DRAW[family](rng, L)
        T.CENSUS[family](case, C)
        for name, value in case["env"].items():
            setenv(name, value)
        try:
            bad = T.CHECK[family](case, rng, L)
        except Exception as e:      # noqa: BLE001 -- the generator draws only what an entry accepts
            bad = "raised %s: %s" % (type(e).__name__, str(e)[:300])
        if bad:
            print("MISMATCH family %s seed %d case %d layer %s: %s: %s" % (family, seed, c, layer, describe(case), bad), flush=True)
            raise AssertionError("fuzz mismatch, family %s seed %d case %d (see the line above): %s" % (family, seed, c, bad))
    gone = missing(family, C, layer, tables) if require else []
    assert not gone, "family %s seed %d, %d cases, layer %s never reached: %s" % (family, seed, cases, layer, gone)
    return C


if __name__ == "__main__":
    family = sys.argv[1]
    n_cases, seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000, int(sys.argv[3]) if len(sys.argv) > 3 else 1
    layer0 = sys.argv[4] if len(sys.argv) > 4 else "host"
    got = run(family, seed0, n_cases, layer0, first=int(sys.argv[5]) if len(sys.argv) > 5 else 0, require=False)
    print("fuzz %s: %d cases, seed %d, layer %s, no mismatch; reached:" % (family, n_cases, seed0, layer0))
    for key in sorted(got):
        print("  %-50s %d" % (key, got[key]))
    print("  never reached: %s" % missing(family, got, layer0))
