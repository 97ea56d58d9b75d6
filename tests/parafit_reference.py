"""ParaFit by the textbook route, in numpy: principal coordinates of both centred matrices by numpy.linalg.eigh, the
fourth-corner matrix D = C^T A B, its squared Frobenius norm, and ParaFitLink1 by recomputing the norm with one link
removed (Legendre, Desdevises & Bazin 2002).  Nothing here uses the Gram identity that the library computes by, except
gram(), the float64 statement of that identity, against which the eigh route's own rounding is measured -- and
integers(), the exact restatement over the int32 codes for the bit-level checks.  No library call except the keyed
permutation, which has its own tests.

A link is (f, s): a position of the held side F and one of the shuffled side S.  Permutation p >= 1 relabels the links
of every F position i through sigma = hommola_permutation(seed, stream[i], p, 0, n_s): (f, s) becomes (f, sigma[s])."""
import numpy as np

from suchtree_amd import compare


def centre(d, transform="sqrt"):
    """G = -1/2 J D2 J of a square distance matrix: D2 = d ("sqrt": its square root is embedded) or d * d ("none")"""
    d = np.asarray(d, dtype=np.float64)
    d2 = d if transform == "sqrt" else d * d
    n = len(d2)
    J = np.eye(n) - np.full((n, n), 1.0 / n)
    g = -0.5 * J @ d2 @ J
    return (g + g.T) / 2


def coordinates(g):
    """(coordinates V sqrt|w|, sign of w) of the axes of g whose eigenvalue is not negligible"""
    w, v = np.linalg.eigh(g)
    keep = np.abs(w) > 1e-12 * np.abs(w).max()
    return v[:, keep] * np.sqrt(np.abs(w[keep])), np.sign(w[keep])


def relabel(links, streams, n_s, seed, p):
    """the S position of every link under permutation p"""
    links = np.asarray(links)
    out = links[:, 1].copy()
    if p:
        for f in np.unique(links[:, 0]).tolist():
            sigma = np.asarray(compare.hommola_permutation(seed, int(streams[f]), p, 0, n_s))
            mine = links[:, 0] == f
            out[mine] = sigma[links[mine, 1]]
    return out


def _norm(D, sf, ss):
    """the squared Frobenius norm of D, every axis pair weighted by the signs of its two eigenvalues"""
    return float((ss[:, None] * sf[None, :] * D * D).sum())


def eigh_route(g_f, g_s, link_f, link_s):
    """(trace, Link1 of every link) by the definition: D = C^T A B over the links, Link1(l) = trace - trace without link l"""
    B, sf = coordinates(g_f)
    C, ss = coordinates(g_s)
    D = C[link_s].T @ B[link_f]
    trace = _norm(D, sf, ss)
    link = np.array([trace - _norm(D - np.outer(C[s], B[f]), sf, ss) for f, s in zip(link_f, link_s)])
    return trace, link


def gram(g_f, g_s, link_f, link_s):
    """the same two in float64 by the Gram identity: T[l][k] = g_f[f_l][f_k] g_s[s_l][s_k]"""
    T = g_f[np.ix_(link_f, link_f)] * g_s[np.ix_(link_s, link_s)]
    return float(T.sum()), 2 * T.sum(axis=1) - np.diag(T)


def integers(q_f, q_s, link_f, link_s):
    """(trace, [Link1], [row sum]) as Python ints over the int32 codes"""
    T = q_f[np.ix_(link_f, link_f)].astype(np.int64) * q_s[np.ix_(link_s, link_s)].astype(np.int64)      # (each below 2^62)
    hi, lo = (T >> 31).sum(axis=1).tolist(), (T & 0x7FFFFFFF).sum(axis=1).tolist()
    rows = [(h << 31) + l for h, l in zip(hi, lo)]
    return sum(rows), [2 * r - int(d) for r, d in zip(rows, np.diag(T).tolist())], rows


def run(q_f, q_s, links, streams, permutations, seed):
    """(traces [permutations + 1], Link1 rows [permutations + 1][L], n_ge of the trace, n_ge of every link) over the codes"""
    links = np.asarray(links)
    traces, rows = [], []
    for p in range(permutations + 1):
        t, link, _ = integers(q_f, q_s, links[:, 0], relabel(links, streams, len(q_s), seed, p))
        traces.append(t)
        rows.append(link)
    n_ge = sum(t >= traces[0] for t in traces[1:])
    link_n_ge = [sum(r[l] >= rows[0][l] for r in rows[1:]) for l in range(len(links))]
    return traces, rows, n_ge, link_n_ge
