"""The set oracle of the tree-set comparison (st_rf_tasks, compare.tree_set), independent of Day's method: a clade is a
frozenset of common-leaf indices read off a parent array, unrooted as the side without common leaf 0, and the shared
clades of two trees, their Robinson-Foulds distance and the number of trees that hold a clade are set operations.  Small
trees only (m <= 129).  The trees come from the helpers of clade_match_reference.py and from parent arrays written out
here (a caterpillar, a complete tree, a tree with polytomies, a star); the library's side of a case is its own range
builder (``_capi.clade_ranges``) on the same arrays."""
import numpy as np

from clade_match_reference import random_tree, shuffled_tree
from suchtree_amd import _capi, synth


def clade_sets(parent, ids, rooted):
    """The eligible induced clades of the tree ``parent`` over the listed leaves ``ids`` (common leaf k is node ids[k]) as
    a set of frozensets of common-leaf indices; unrooted, of a set and its complement the one without index 0."""
    parent = np.asarray(parent)
    m, index = len(ids), {int(v): k for k, v in enumerate(ids)}
    under = [set() for _ in parent]
    children = [[] for _ in parent]
    for v, p in enumerate(parent):
        if p >= 0:
            children[int(p)].append(v)
    order, stack = [], [int(np.flatnonzero(parent == -1)[0])]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(children[v])
    for v in reversed(order):
        if not children[v] and v in index:
            under[v].add(index[v])
        for c in children[v]:
            under[v] |= under[c]
    everything, out = frozenset(range(m)), set()
    for v in order:
        s = frozenset(under[v])
        if not children[v] or len(s) < 2 or any(len(under[c]) == len(s) for c in children[v]):
            continue
        if rooted:
            if len(s) <= m - 1:
                out.add(s)
        elif len(s) <= m - 2:
            out.add(everything - s if 0 in s else s)
    return out


def relabel(sets, a, rooted):
    """The clades of tree j seen from tree i under the alignment ``a`` (common leaf k of i meets common leaf a[k] of j)."""
    back = {int(v): k for k, v in enumerate(a)}
    m = len(back)
    out = set()
    for s in sets:
        t = frozenset(back[x] for x in s)
        out.add(frozenset(range(m)) - t if not rooted and 0 in t else t)
    return out


def shared(sets_i, sets_j, a=None, rooted=False):
    return len(sets_i & (sets_j if a is None else relabel(sets_j, a, rooted)))


def frequencies(all_sets):
    """{clade: number of trees of the set that hold it}"""
    out = {}
    for sets in all_sets:
        for s in sets:
            out[s] = out.get(s, 0) + 1
    return out


def _dealt(parent, m, seed):
    """(parent, ids): the common leaves dealt to the leaves of an in-order tree (the even ids) in a seeded random order"""
    return np.asarray(parent, dtype=np.int32), (np.random.default_rng(seed).permutation(m) * 2).astype(np.int64)


def polytomy_tree(m, seed):
    """A seeded random tree whose internal edges are collapsed with probability 1/2: nodes of up to m children."""
    parent, _ = synth.random_binary_tree(m, seed=seed)
    parent = np.asarray(parent).copy()
    rng = np.random.default_rng(seed + 1)
    internal = np.flatnonzero(np.bincount(parent[parent >= 0], minlength=len(parent)) > 0)
    gone = np.array([v for v in internal if parent[v] >= 0 and rng.random() < 0.5], dtype=np.int64)
    dead = np.zeros(len(parent), dtype=bool)
    dead[gone] = True
    for v in range(len(parent)):
        p = parent[v]
        while p >= 0 and dead[p]:
            p = parent[p]
        parent[v] = p
    new_id = np.cumsum(~dead) - 1
    kept = np.flatnonzero(~dead)
    out = np.array([-1 if parent[v] < 0 else new_id[parent[v]] for v in kept], dtype=np.int32)
    leaves = np.random.default_rng(seed + 2).permutation(m) * 2      # (the leaves of the binary tree are its even ids)
    return out, new_id[leaves].astype(np.int64)


def star_tree(m):
    """One root, m leaves: no clade at all."""
    return np.array([-1] + [0] * m, dtype=np.int32), np.arange(1, m + 1, dtype=np.int64)


def tree_set(m, seed):
    """[(parent, ids)] of six trees over m common leaves: a random tree, an identical copy of it, a caterpillar, a complete
    (balanced) tree and a tree with polytomies, the common leaves dealt to each in another order, and a star."""
    names = ["L%d" % k for k in range(m)]
    a = random_tree(m, seed)
    b = shuffled_tree(m, seed + 1, seed + 2)
    first = (np.asarray(a._flat.parent, dtype=np.int32), a._name_ids(names))
    return [first, (first[0].copy(), first[1].copy()), _dealt(synth.caterpillar_tree(m)[0], m, seed + 3),
            _dealt(synth.complete_tree(m)[0], m, seed + 4), polytomy_tree(m, seed + 5), star_tree(m),
            (np.asarray(b._flat.parent, dtype=np.int32), b._name_ids(names))]


def library_sides(trees, rooted):
    """(where, offsets, lo, hi, sides) of st_rf_tasks for ``trees`` through the library's range builder"""
    m = len(trees[0][1])
    sides = [_capi.clade_ranges(parent, ids, rooted) for parent, ids in trees]
    where = np.empty((len(trees), m), dtype=np.int32)
    for t, side in enumerate(sides):
        where[t, side[0]] = np.arange(m, dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s[1]) for s in sides])]).astype(np.int64)
    lo = np.concatenate([s[2] for s in sides]).astype(np.int32)
    hi = np.concatenate([s[3] for s in sides]).astype(np.int32)
    return where, offsets, lo, hi, sides


def side_sets(side, rooted):
    """The clades of one library side (order, node, lo, hi) as the oracle's canonical frozensets, in list order"""
    order, _, lo, hi = side
    m = len(order)
    out = []
    for l, h in zip(lo, hi):
        s = frozenset(int(x) for x in order[l:h])
        out.append(frozenset(range(m)) - s if not rooted and 0 in s else s)
    return out


def triangle(n):
    return [(i, j) for i in range(n) for j in range(i)]
