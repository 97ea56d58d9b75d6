"""The within-group sums of st_group_sums_codes written straight from the definition (include/suchtree_hip.h), in Python
ints and loops over pairs: the reference tests/test_group_tests_host.py and the fuzz compare the library with."""
from suchtree_amd import _capi


def group_sums(y, group, n_groups, permutations, seed=0, stream=0):
    """[[sum over j < i with group[sigma_p(i)] == group[sigma_p(j)] == h of y[i (i - 1) / 2 + j] for h] for p]"""
    y = [int(v) for v in y]
    group = [int(g) for g in group]
    n = len(group)
    rows = []
    for p in range(int(permutations) + 1):
        sigma = _capi.hommola_permutation(seed, stream, p, 0, n).tolist()
        if p == 0:
            assert sigma == list(range(n))
        row = [0] * n_groups
        for i in range(n):
            gi = group[sigma[i]]
            for j in range(i):
                if group[sigma[j]] == gi:
                    row[gi] += y[i * (i - 1) // 2 + j]
        rows.append(row)
    return rows
