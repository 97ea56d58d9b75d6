"""A float64 numpy brute force of the between-set dispersion definitions (include/suchtree_hip.h,
st_beta_dispersion_host), for tests/test_beta_dispersion_host.py and tests/test_gpu_beta_dispersion.py: nothing here
calls the library's reduction.  Sums are math.fsum over the float32 entries, the correctly rounded sum."""
import math

import numpy as np


def direction(D, sigma, s_r, s_c, exclude):
    """(cross_sum, nearest_sum, z) of direction r -> c: positions ``s_r`` / ``s_c`` of the universe relabelled by
    ``sigma`` over the matrix ``D``; z = the elements of r with no included entry."""
    s_r, s_c = np.asarray(s_r, dtype=np.int64), np.asarray(s_c, dtype=np.int64)
    if len(s_r) == 0:
        return 0.0, 0.0, 0
    if len(s_c) == 0:
        return 0.0, 0.0, len(s_r)
    sub = np.asarray(D)[np.ix_(sigma[s_r], sigma[s_c])].astype(np.float64)
    keep = np.ones(sub.shape, dtype=bool) if not exclude else s_r[:, None] != s_c[None, :]
    rows = keep.any(axis=1)
    with np.errstate(invalid="ignore"):
        mins = np.where(keep, sub, np.inf).min(axis=1)[rows]
    return math.fsum(sub[keep]), math.fsum(mins), int(np.count_nonzero(~rows))


def beta(D, sigma, a, b, exclude):
    """(beta_mpd, beta_mntd) of the position sets a and b: picante's comdist / comdistnt, unweighted."""
    c_ab, n_ab, z_ab = direction(D, sigma, a, b, exclude)
    c_ba, n_ba, z_ba = direction(D, sigma, b, a, exclude)
    e = len(np.intersect1d(a, b)) if exclude else 0
    den_mpd, den_mntd = 2 * (len(a) * len(b) - e), len(a) + len(b) - z_ab - z_ba
    return ((c_ab + c_ba) / den_mpd if den_mpd else math.nan), ((n_ab + n_ba) / den_mntd if den_mntd else math.nan)


def pairs(n_sets, begin=0, count=None):
    """[(i, j)] of triangle indices [begin, begin + count): k = i (i - 1) / 2 + j, j < i."""
    out = [(i, j) for i in range(n_sets) for j in range(i)]
    return out[begin:] if count is None else out[begin:begin + count]


def null_columns(observed, null):
    """{suffix: value} of one statistic against its null draws, by the definitions of compare.SetBetaDispersion."""
    draws = null[~np.isnan(null)]
    mean = draws.mean() if len(draws) else math.nan
    sd = draws.std(ddof=1) if len(draws) >= 2 else math.nan
    if len(draws) >= 2 and draws.min() == draws.max():
        mean, sd = draws[0], 0.0
    n_le, n_ge = int(np.count_nonzero(draws <= observed)), int(np.count_nonzero(draws >= observed))
    p = len(null) + 1
    return {"_null_mean": mean, "_null_sd": sd, "_ses": (observed - mean) / sd if sd > 0 else math.nan, "_n_le": n_le, "_n_ge": n_ge,
            "_p_le": math.nan if math.isnan(observed) else (n_le + 1) / p, "_p_ge": math.nan if math.isnan(observed) else (n_ge + 1) / p}
