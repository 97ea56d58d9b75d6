"""The Mantel and partial Mantel tests as the contract of include/suchtree_hip.h (st_mantel_codes) states them, in numpy
and Python ints: no library call except the keyed permutation, which has its own tests.

Both matrices are int32 codes.  x is square (n, n); y and z are condensed in the triangle order k = i (i - 1) / 2 + j,
j < i.  Permutation p relabels x: Sxy_p = sum over j < i of x[sigma_p(i)][sigma_p(j)] * y[k(i, j)], p = 0 the identity."""
import math

import numpy as np

from suchtree_amd import compare


def tri(n):
    """(i, j) of the pairs in triangle order"""
    return np.tril_indices(n, -1)


def condensed(a):
    i, j = tri(len(a))
    return np.asarray(a)[i, j]


def square(v, n, dtype=None):
    out = np.zeros((n, n), dtype=dtype or np.asarray(v).dtype)
    i, j = tri(n)
    out[i, j] = out[j, i] = v
    return out


def quantise(v, shift=None):
    """(llrint(ldexp(v, shift)) as Python ints, the shift): shift None = the largest |code| in [2^30, 2^31)"""
    v = [float(t) for t in np.asarray(v, dtype=np.float64).ravel()]
    top = max((abs(t) for t in v), default=0.0)
    if shift is None:
        shift = 0 if top == 0.0 else 30 - (math.frexp(top)[1] - 1)
        if round(math.ldexp(top, shift)) >= 1 << 31:
            shift -= 1
    return [round(math.ldexp(t, shift)) for t in v], shift      # (round: half to even, as llrint in the default mode)


def rank_codes(v):
    """2 * midrank - (m + 1), ties averaged, -0.0 == +0.0: counted pair by pair"""
    v = [float(t) for t in v]
    return [sum((a > b) - (a < b) for b in v) for a in v]      # (2 (less + (equal + 1) / 2) - (m + 1) = less - greater)


def sigma(seed, stream, p, n):
    return [int(t) for t in compare.hommola_permutation(seed, stream, p, 0, n)]


def dot(x_sq, w, s):
    """sum over j < i of x[s(i)][s(j)] * w[k(i, j)] as a Python int"""
    n = len(x_sq)
    i, j = tri(n)
    s = np.asarray(s)
    xs = np.asarray(x_sq)[s[i], s[j]]
    return sum(int(a) * int(b) for a, b in zip(xs.tolist(), np.asarray(w).tolist()))


def moments(x_sq, y, z=None):
    xv = [int(t) for t in condensed(x_sq)]
    yv = [int(t) for t in y]
    zv = [int(t) for t in z] if z is not None else [0] * len(yv)
    return {"sx": sum(xv), "sy": sum(yv), "sz": sum(zv), "sxx": sum(t * t for t in xv), "syy": sum(t * t for t in yv),
            "szz": sum(t * t for t in zv), "syz": sum(a * b for a, b in zip(yv, zv))}


def records(x_sq, y, z, permutations, seed, stream=0):
    """[(Sxy_p, Sxz_p)] for p = 0 .. permutations (Sxz_p = 0 without z)"""
    out = []
    for p in range(permutations + 1):
        s = sigma(seed, stream, p, len(x_sq))
        out.append((dot(x_sq, y, s), dot(x_sq, z, s) if z is not None else 0))
    return out


def simple_test(x_sq, y, permutations, seed, stream=0):
    """(r, n_ge, n_le, n_abs_ge) of the simple test by a plain loop: the counts compare the integers m Sxy_p - Sx Sy"""
    M = moments(x_sq, y)
    m = len(y)
    c = [m * sxy - M["sx"] * M["sy"] for sxy, _ in records(x_sq, y, None, permutations, seed, stream)]
    den = (m * M["sxx"] - M["sx"] ** 2) * (m * M["syy"] - M["sy"] ** 2)
    r = c[0] / math.sqrt(den) if den > 0 else float("nan")
    return (r, sum(v >= c[0] for v in c[1:]), sum(v <= c[0] for v in c[1:]), sum(abs(v) >= abs(c[0]) for v in c[1:]))


def p_value(count, permutations):
    return (count + 1) / (permutations + 1)
