"""The within-set dispersion sums (include/suchtree_hip.h, st_dispersion_matrix) by a straightforward O(k^2) loop, for
tests/test_dispersion_host.py and tests/fuzz_analyses.py: nothing here calls the library's reduction.  Sums are math.fsum
over the float32 entries, the correctly rounded sum."""
import math


def plain(D, q):
    """(pair_sum, nearest_sum) of the relabelled positions q by the O(k^2) loop, in math.fsum."""
    k = len(q)
    if k < 2:
        return 0.0, 0.0
    sums, mins = [], []
    for i in range(k):
        vals = [float(D[q[i], q[j]]) for j in range(k) if j != i]
        sums.append(math.fsum(vals))
        m = math.inf
        for v in vals:      # the stated rule: v < m ? v : m
            m = v if v < m else m
        mins.append(m)
    return math.fsum(sums), math.fsum(mins)
