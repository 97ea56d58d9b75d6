"""The naive restatement of st_linkage_codes (include/suchtree_hip.h) for the linkage tests: a matrix of Python ints
and a scan of every active pair per step.  No cache, no 128-bit arithmetic to get wrong: fractions compare by
cross-multiplication of unbounded ints."""
import numpy as np


def reference_linkage(codes, n, weights=None, method="average"):
    """The n - 1 rows (left, right, num, den, size) as tuples of Python ints."""
    codes = [int(c) for c in codes]
    size = [1] * n if weights is None else [int(w) for w in weights]
    cid = list(range(n))
    S = [[0] * n for _ in range(n)]
    for i in range(1, n):
        for j in range(i):
            c = codes[i * (i - 1) // 2 + j]
            S[i][j] = S[j][i] = c * size[i] * size[j] if method == "average" else c
    active = list(range(n))
    rows = []
    for t in range(n - 1):
        best = None
        for x, a in enumerate(active):
            for b in active[x + 1:]:
                num, den = S[a][b], size[a] * size[b] if method == "average" else 1
                if best is None or num * best[1] < best[0] * den:      # (strictly less: the first pair in (a, b) order stays)
                    best = (num, den, a, b)
        num, den, a, b = best
        rows.append((min(cid[a], cid[b]), max(cid[a], cid[b]), num, den, size[a] + size[b]))
        for k in active:
            if k != a and k != b:
                va, vb = S[k][a], S[k][b]
                S[k][a] = S[a][k] = va + vb if method == "average" else min(va, vb) if method == "single" else max(va, vb)
        size[a] += size[b]
        cid[a] = n + t
        active.remove(b)
    return rows


def rows_of(records):
    """The records of _capi.linkage_codes in the reference's form."""
    return [(int(r["left"]), int(r["right"]), int(r["num"]), int(r["den"]), int(r["size"])) for r in records]


def random_codes(n, seed, lo=1 << 30, hi=1 << 31):
    """Condensed codes in [lo, hi): distinct with overwhelming probability at the test sizes (checked by the caller)."""
    return np.random.default_rng(seed).integers(lo, hi, size=n * (n - 1) // 2, dtype=np.int64).astype(np.int32)


def ultrametric_codes(n, seed):
    """(condensed cophenetic codes, the member sets of the n - 1 internal nodes) of a seeded random binary ultrametric
    tree over n leaves with distinct node heights: clusters are joined in random order at heights 1000, 2000, ..."""
    rng = np.random.default_rng(seed)
    clusters = [[i] for i in range(n)]
    d = np.zeros((n, n), dtype=np.int64)
    clades = []
    for t in range(n - 1):
        i, j = sorted(rng.choice(len(clusters), size=2, replace=False).tolist())
        a, b = clusters[i], clusters[j]
        d[np.ix_(a, b)] = d[np.ix_(b, a)] = 1000 * (t + 1)
        clusters[i] = a + b
        del clusters[j]
        clades.append(frozenset(clusters[i]))
    r, c = np.tril_indices(n, -1)
    return d[r, c].astype(np.int32), clades
