"""Shared by tests/test_unifrac_null_host.py and tests/test_gpu_unifrac_null.py: the null's expectation composed from calls
that exist without it -- sigma from compare.hommola_permutation on the host, the relabelled sets sorted with numpy,
_capi.unifrac_depths(device=-1) on them (itself pinned to brute force in tests/test_unifrac_host.py) -- and inputs: integer
depths over a universe, and sets at the sizes where a kernel form changes."""
import numpy as np

from suchtree_amd import _capi, compare


def compose(d_q, h_q, sets, permutations, seed, stream, begin=0, count=None):
    """(pd (n_sets, permutations + 1), union (count, permutations + 1)) by one unifrac_depths call per permutation."""
    n = len(d_q)
    sets = [np.asarray(s, dtype=np.int64) for s in sets]
    pd, union = [], []
    for p in range(permutations + 1):
        sigma = compare.hommola_permutation(seed, stream, p, 0, n, device=None)
        relabelled = [np.sort(sigma[s]) for s in sets]
        a, b = _capi.unifrac_depths(d_q, h_q, relabelled, begin, count, device=-1)
        pd.append(a)
        union.append(b)
    return np.stack(pd, axis=1), np.stack(union, axis=1)


def depths(n, seed):
    """Integer depths of a universe of n leaves: d any values, h[k] at most min(d[k], d[k + 1]) -- negative ones among them."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-5000, 1 << 30, n).astype(np.int64)
    h = np.minimum(d[:-1], d[1:]) - rng.integers(0, 1 << 20, n - 1)
    return d, h.astype(np.int64)


def sized_sets(n, sizes, seed):
    """One random set per size that fits in n, then the whole universe, a copy of the largest random set, and positions 0 and
    n - 1 together."""
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(n, k, replace=False)) for k in sizes if k <= n]
    sets += [np.arange(n), max(sets, key=len).copy(), np.array([0, n - 1])]
    return [s.astype(np.int64) for s in sets]
