"""Brute-force reference of the clade matching (st_clade_ranges, st_clade_match), with Python sets over ``get_leaves``,
straight from the definitions of include/suchtree_hip.h.  A leaf is named by its index in the call's leaf list, so sets of
the two trees compare directly.  Shared by the host and the GPU tests; small trees only (every clade is a set)."""
import numpy as np

from suchtree_amd import synth
from suchtree_amd.suchtree import SuchTree


def depth_first_positions(tree, ids):
    """position[k] of list index k: the listed leaves depth-first, children in increasing id order."""
    index = {int(v): k for k, v in enumerate(ids)}
    position, stack = {}, [tree.root_node]
    while stack:
        v = stack.pop()
        if tree.is_leaf(v):
            if v in index:
                position[index[v]] = len(position)
        else:
            stack.extend(sorted(tree.get_children(v), reverse=True))
    return position


def induced_clades(tree, ids, rooted):
    """[(node, frozenset of list indices)] of the eligible induced clades, in get_internal_nodes() order."""
    index = {int(v): k for k, v in enumerate(ids)}
    m = len(ids)
    under = lambda v: frozenset(index[int(x)] for x in ([v] if tree.is_leaf(v) else tree.get_leaves(v)) if int(x) in index)  # noqa: E731
    kept = []
    for v in tree.get_internal_nodes():
        mine = under(int(v))
        if len(mine) < 2 or any(len(under(int(c))) == len(mine) for c in tree.get_children(int(v))):
            continue
        kept.append((int(v), mine))
    if rooted:
        return [(v, s) for v, s in kept if 2 <= len(s) <= m - 1]
    eligible = [(v, s) for v, s in kept if 2 <= len(s) <= m - 2]
    position = depth_first_positions(tree, ids)
    last = [k for k, p in position.items() if p == m - 1][0]
    everything, sets = frozenset(range(m)), {s for _, s in eligible}
    # of a clade and its complement, both eligible, the one that ends the depth-first order ([k, m)) goes
    return [(v, s) for v, s in eligible if not (last in s and everything - s in sets)]


def match(rows, candidates, m, rooted):
    """(distance, match index, intersection) per row against every candidate: the least (delta, index)."""
    out = []
    for _, a in rows:
        best = None
        for index, (_, b) in enumerate(candidates):
            i = len(a & b)
            d = len(a) + len(b) - 2 * i
            delta = d if rooted else min(d, m - d)
            if best is None or (delta, index) < best[:2]:
                best = (delta, index, i)
        out.append(best if best is not None else (-1, -1, 0))
    return out


def compare(tree_a, ids_a, tree_b, ids_b, rooted):
    """What SuchTree.compare_clades reports, from the definitions: a dict of lists and scalars."""
    m = len(ids_a)
    rows, cands = induced_clades(tree_a, ids_a, rooted), induced_clades(tree_b, ids_b, rooted)
    got = match(rows, cands, m, rooted)
    p = [len(a) if rooted else min(len(a), m - len(a)) for _, a in rows]
    transfer = [min(g[0], q - 1) if g[1] >= 0 else q - 1 for g, q in zip(got, p)]
    exact = sum(1 for g in got if g[0] == 0)
    return {"nodes": [v for v, _ in rows], "n_leaves": [len(a) for _, a in rows], "match": [cands[g[1]][0] if g[1] >= 0 else -1 for g in got],
            "distance": [g[0] for g in got], "intersection": [g[2] for g in got], "transfer": transfer,
            "support": [1 - t / (q - 1) for t, q in zip(transfer, p)], "exact": exact, "n_a": len(rows), "n_b": len(cands),
            "rf": len(rows) + len(cands) - 2 * exact}


def ranges(tree, ids, rooted):
    """(lo, hi, node) arrays of the eligible induced clades as position ranges (every induced clade is one range)."""
    position = depth_first_positions(tree, ids)
    lo, hi, node = [], [], []
    for v, s in induced_clades(tree, ids, rooted):
        where = sorted(position[k] for k in s)
        assert where == list(range(where[0], where[0] + len(where)))
        lo.append(where[0])
        hi.append(where[-1] + 1)
        node.append(v)
    return np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32), np.array(node, dtype=np.int32)


def random_tree(n_leaves, seed):
    """A seeded random binary SuchTree whose leaves are named L0, L1, ... in id order (no GPU is touched)."""
    parent, distance = synth.random_binary_tree(n_leaves, seed=seed)
    return SuchTree((parent, distance, ["L%d" % k for k in range(n_leaves)]))


def shuffled_tree(n_leaves, seed, label_seed):
    """The same kind of tree with the names L0 ... dealt to the leaves in a seeded random order."""
    parent, distance = synth.random_binary_tree(n_leaves, seed=seed)
    names = ["L%d" % k for k in np.random.default_rng(label_seed).permutation(n_leaves)]
    return SuchTree((parent, distance, names))


def pair_arrays(tree_a, tree_b, rooted, names=None):
    """(m, pos_b, a_lo, a_hi, b_lo, b_hi) of two SuchTrees over their shared leaves, through the library's range builder."""
    from suchtree_amd import compare as cmp
    if names is None:
        _, ids_a, ids_b = tree_a.shared_leaves(tree_b)
    else:
        ids_a, ids_b = tree_a._name_ids(names), tree_b._name_ids(names)
    side_a, side_b = cmp.clade_side(tree_a._flat, ids_a, rooted), cmp.clade_side(tree_b._flat, ids_b, rooted)
    m = len(ids_a)
    where_b = np.empty(m, dtype=np.int32)
    where_b[side_b[0]] = np.arange(m, dtype=np.int32)
    return m, where_b[side_a[0]], side_a[2], side_a[3], side_b[2], side_b[3]
