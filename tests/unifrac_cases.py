"""Shared inputs of tests/test_unifrac_host.py and tests/test_gpu_unifrac.py: seeded random binary trees over n leaves in
depth-first order with integer node depths, the position sets of the edge cases, and the brute-force definition of the
union sum -- the sum of depth(v) - depth(parent(v)) over the nodes v with a member below them, the root's own depth
(its parent counts as 0) included.  Edge lengths are non-negative (the minimum over adjacent MRCA depths finds the MRCA
only then); the root's depth is negative, so that many depths are."""
import numpy as np

SIZES = (0, 1, 2, 31, 32, 33, 63, 64, 65)


def random_tree(n, seed):
    """(parent, depth, leaf_node): node ids in creation order, node 0 the root; leaf_node[k] is the node of leaf k, the
    leaves in depth-first order."""
    rng = np.random.default_rng(seed)
    parent, depth, leaf_node = [-1], [-int(rng.integers(1000, 5000))], [0] * n
    stack = [(0, 0, n)]
    while stack:
        node, lo, k = stack.pop()
        if k == 1:
            leaf_node[lo] = node
            continue
        a = int(rng.integers(1, k))
        for lo2, k2 in ((lo, a), (lo + a, k - a)):
            parent.append(node)
            depth.append(depth[node] + int(rng.integers(0, 1000)))
            stack.append((len(parent) - 1, lo2, k2))
    return np.array(parent), np.array(depth, dtype=np.int64), np.array(leaf_node)


def depths(parent, depth, leaf_node):
    """(d, h): the depth of every leaf and of the MRCA of every two adjacent leaves."""
    n = len(leaf_node)
    h = np.zeros(max(n - 1, 0), dtype=np.int64)
    for k in range(n - 1):
        seen, v = set(), leaf_node[k]
        while v != -1:
            seen.add(v)
            v = parent[v]
        v = leaf_node[k + 1]
        while v not in seen:
            v = parent[v]
        h[k] = depth[v]
    return depth[leaf_node].copy(), h


def node_masks(parent, leaf_node, sets):
    """(len(sets), nodes) bool: node v has a member of the set below it (or is one)."""
    out = np.zeros((len(sets), len(parent)), dtype=bool)
    for r, s in enumerate(sets):
        for p in s:
            v = leaf_node[p]
            while v != -1 and not out[r, v]:
                out[r, v] = True
                v = parent[v]
    return out


def brute_force(parent, depth, leaf_node, sets):
    """(pd, union): PD of every set and the union sum of every pair in triangle order, by the definition."""
    edge = depth - np.where(parent >= 0, depth[np.maximum(parent, 0)], 0)
    masks = node_masks(parent, leaf_node, sets)
    pd = masks @ edge
    union = np.array([(masks[i] | masks[j]) @ edge for i in range(len(sets)) for j in range(i)], dtype=np.int64)
    return pd.astype(np.int64), union


def edge_sets(n, seed):
    """The sets of a universe of n positions: one random set per size that fits, the whole universe, an identical, a nested
    and two disjoint sets, sets that hold position 0 and n - 1, adjacent positions, and for every table level l pairs of
    positions 2^l - 1, 2^l and 2^l + 1 apart at both ends of the universe."""
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(n, k, replace=False)) for k in SIZES if k <= n]
    big = max(sets, key=len)
    sets += [np.arange(n), big.copy(), big[: len(big) // 2], np.arange(0, n, 2), np.arange(1, n, 2), np.array([0, n - 1][: min(n, 2)])]
    if n >= 2:
        sets += [np.array([0, 1]), np.array([n - 2, n - 1]), np.array([n // 2 - 1, n // 2])]
    gap = 1
    while gap - 1 <= n - 1:
        for g in (gap - 1, gap, gap + 1):
            if 1 <= g <= n - 1:
                sets += [np.array([0, g]), np.array([n - 1 - g, n - 1])]
        gap *= 2
    return [np.unique(s).astype(np.int64) for s in sets]


def case(n):
    """(parent, depth, leaf_node, d, h, sets) of universe size n."""
    parent, depth, leaf_node = random_tree(n, 1000 + n)
    d, h = depths(parent, depth, leaf_node)
    return parent, depth, leaf_node, d, h, edge_sets(n, 2000 + n)
