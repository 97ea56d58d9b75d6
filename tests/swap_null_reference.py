"""The swap null's chain restated in plain Python integers (include/suchtree_hip.h, st_swap_null_tables), for
tests/test_swap_null_host.py and tests/test_gpu_swap_null.py: the stream hash, the draw of a trial, the serial chain, the
enumeration of a margin class and the chi-square of chains against the uniform distribution on it."""
import itertools

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def perm_stream(seed, node, p, side):
    h0 = mix(seed + (node + 1) * GOLDEN)
    return mix(h0 + (2 * p + side) * GOLDEN)


def chain(rows, p, iterations, seed, stream):
    """(rows of chain p as sorted lists, accepted) from the observed ``rows`` (lists of increasing positions)."""
    col = [c for r in rows for c in r]
    row_of = [i for i, r in enumerate(rows) for _ in r]
    member = [set(r) for r in rows]
    L, accepted = len(col), 0
    if p >= 1 and L >= 2:
        h1 = perm_stream(seed, stream, p, 1)
        for t in range(iterations):
            e1 = (mix(h1 + (2 * t + 1) * GOLDEN) * L) >> 64
            e2 = (mix(h1 + (2 * t + 2) * GOLDEN) * L) >> 64
            r1, r2, b, d = row_of[e1], row_of[e2], col[e1], col[e2]
            if r1 != r2 and b != d and d not in member[r1] and b not in member[r2]:
                member[r1].remove(b)
                member[r1].add(d)
                member[r2].remove(d)
                member[r2].add(b)
                col[e1], col[e2] = d, b
                accepted += 1
    return [sorted(m) for m in member], accepted


def table_row(rows, p, iterations, seed, stream):
    """(the flat table row, accepted) of chain p"""
    out, accepted = chain(rows, p, iterations, seed, stream)
    return [c for r in out for c in r], accepted


def margin_class(rows, n_cols):
    """every 0/1 matrix with the row sums and column sums of ``rows``, as tuples of row tuples"""
    degree = [0] * n_cols
    for r in rows:
        for c in r:
            degree[c] += 1
    states = []

    def place(i, left, acc):
        if i == len(rows):
            if not any(left):
                states.append(tuple(acc))
            return
        for combo in itertools.combinations([c for c in range(n_cols) if left[c] > 0], len(rows[i])):
            for c in combo:
                left[c] -= 1
            place(i + 1, left, acc + [combo])
            for c in combo:
                left[c] += 1

    place(0, degree, [])
    return states


def chi_square(rows, n_cols, chains, iterations, seed, stream):
    """(chi-square of the end states of chains p = 1 .. chains against the uniform distribution on the margin class, the
    number of states, the fraction of trials accepted)"""
    states = margin_class(rows, n_cols)
    count = dict.fromkeys(states, 0)
    accepted = 0
    for p in range(1, chains + 1):
        out, a = chain(rows, p, iterations, seed, stream)
        count[tuple(tuple(r) for r in out)] += 1      # (a state outside the class is a KeyError)
        accepted += a
    expect = chains / len(states)
    return sum((v - expect) ** 2 / expect for v in count.values()), len(states), accepted / (chains * iterations)
