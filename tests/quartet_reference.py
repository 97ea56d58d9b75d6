"""References for the quartet comparison, independent of the library: no GPU, no suchtree_amd code.

colex_quartets       every 4-subset of range(m) in colexicographic order, built from its own prefixes in numpy
unrank_exact         the four positions of quartet k, in Python integers with math.comb, searched downward
py_draw              the seeded draw of quartet k among m leaves (quartet_plan.h: quartet_draw), in Python integers
mrca_matrices        depth and id of the MRCA of every two leaves of a list, by walking parents
leaf_classes         the class of quartets of distinct leaves in a rooted tree of any arity and numbering, by the
                     four-point rule over MRCA depths -- not the pick rule over MRCA ids that the library implements
perfect_classes / caterpillar_classes / star_classes     the same classes in closed form, for counts too large to walk
perfect_tree / caterpillar / star / random_general_tree   (parent, dist, leaf_ids) of trees in a numbering of their own
table_of             the 4 x 4 table of two class arrays
"""
import math

import numpy as np

M64 = (1 << 64) - 1


# ---- which quartet is quartet k -------------------------------------------------------------------------------------
def _extend(prefixes, m, r):
    """The r-subsets of range(m) in colexicographic order from the (r-1)-subsets in that order: those whose largest
    member is p are the first C(p, r-1) of the (r-1)-subsets, each with p appended, for p = 0 .. m-1 in turn."""
    counts = np.array([math.comb(p, r - 1) for p in range(m)], dtype=np.int64)
    top = np.repeat(np.arange(m, dtype=np.int64), counts)
    first = np.repeat(np.cumsum(counts) - counts, counts)
    return np.column_stack([prefixes[np.arange(len(top), dtype=np.int64) - first], top])


def colex_quartets(m):
    """int64 (C(m,4), 4): every 4-subset p0 < p1 < p2 < p3 of range(m), ordered by p3, then p2, then p1, then p0."""
    sets = np.arange(m, dtype=np.int64).reshape(-1, 1)
    for r in (2, 3, 4):
        sets = _extend(sets, m, r)
    return sets.reshape(-1, 4)


def unrank_exact(k):
    """[p0, p1, p2, p3] of quartet k in colexicographic order: p3 the largest p with C(p,4) <= k, and so on down."""
    out = []
    for r in (4, 3, 2, 1):
        p = int(round((math.factorial(r) * k) ** (1.0 / r))) + r
        while math.comb(p, r) <= k:      # (make sure of the over-estimate, whatever the floating-point root gave)
            p += 1
        while math.comb(p, r) > k:
            p -= 1
        out.append(p)
        k -= math.comb(p, r)
    return out[::-1]


def py_mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_draw(seed, k, m):
    """The four distinct positions of sampled quartet k, in draw order: draw j is a rank among the m - j positions not
    yet chosen, the high 64 bits of mix(seed + (4 k + j + 1) * golden) * (m - j)."""
    chosen, out = [], []
    for j in range(4):
        u = py_mix((seed + (4 * k + j + 1) * 0x9E3779B97F4A7C15) & M64)
        p = (u * (m - j)) >> 64
        for q in sorted(chosen):
            if p >= q:
                p += 1
        chosen.append(p)
        out.append(p)
    return out


# ---- the class of a quartet -----------------------------------------------------------------------------------------
def node_depths(parent):
    """Edges between each node and the root, by walking parents."""
    parent = np.asarray(parent, dtype=np.int64)
    depth = np.full(len(parent), -1, dtype=np.int64)
    for v in range(len(parent)):
        path = []
        while v >= 0 and depth[v] < 0:
            path.append(v)
            v = parent[v]
        d = depth[v] if v >= 0 else -1
        for u in reversed(path):
            d += 1
            depth[u] = d
    return depth


def mrca_matrices(parent, ids):
    """(D, M), both (m, m) int64: depth and id of the MRCA of ids[i] and ids[j].  Every leaf's path to the root is
    walked once; the MRCA of i and j is the first node on j's path that lies on i's."""
    parent = np.asarray(parent, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    depth = node_depths(parent)
    paths = np.full((len(ids), int(depth[ids].max()) + 1 if len(ids) else 1), -1, dtype=np.int64)
    for i, v in enumerate(ids):
        k = 0
        while v >= 0:
            paths[i, k] = v
            v = parent[v]
            k += 1
    D = np.zeros((len(ids), len(ids)), dtype=np.int64)
    M = np.zeros((len(ids), len(ids)), dtype=np.int64)
    on_path = np.zeros(len(parent) + 1, dtype=bool)      # (the last entry stands for the -1 padding)
    rows = np.arange(len(ids))
    for i in range(len(ids)):
        mine = paths[i][paths[i] >= 0]
        on_path[mine] = True
        M[i] = paths[rows, np.argmax(on_path[paths], axis=1)]
        D[i] = depth[M[i]]
        on_path[mine] = False
    return D, M


def classes_of_depths(ab, cd, ac, bd, ad, bc):
    """0 = ab|cd, 1 = ac|bd, 2 = ad|bc where that pairing's sum of MRCA depths is strictly the largest of the three
    (the pairing the tree's inner edge separates), 3 where none is."""
    s0, s1, s2 = ab + cd, ac + bd, ad + bc
    return np.where((s0 > s1) & (s0 > s2), 0, np.where((s1 > s0) & (s1 > s2), 1, np.where((s2 > s0) & (s2 > s1), 2, 3)))


def leaf_classes(parent, ids, positions, D=None):
    """The class of quartet (ids[p0], ids[p1], ids[p2], ids[p3]) for every row of ``positions`` (distinct leaves), in
    the rooted tree ``parent`` of any arity and numbering.  ``D``: mrca_matrices(parent, ids)[0], where it is at hand."""
    if D is None:
        D = mrca_matrices(parent, ids)[0]
    a, b, c, d = np.asarray(positions, dtype=np.int64).T
    return classes_of_depths(D[a, b], D[c, d], D[a, c], D[b, d], D[a, d], D[b, c])


def _bit_length(v):
    """Of int64 values in [0, 2^53): v = f * 2^e with 0.5 <= f < 1 has e bits; frexp gives e = 0 for v = 0."""
    return np.frexp(v.astype(np.float64))[1].astype(np.int64)


def perfect_classes(levels, leaves):
    """Classes of the rows of ``leaves`` (n, 4): each entry is a leaf of the perfect binary tree of 2^levels leaves,
    counted from the left.  The MRCA of leaves i and j lies at depth levels - bit_length(i xor j)."""
    a, b, c, d = np.asarray(leaves, dtype=np.int64).T
    D = lambda i, j: levels - _bit_length(i ^ j)      # noqa: E731
    return classes_of_depths(D(a, b), D(c, d), D(a, c), D(b, d), D(a, d), D(b, c))


def caterpillar_classes(positions):
    """A caterpillar whose leaves are listed in depth order (either way): the two ends of a sorted quartet that lie on
    the same side of the other two are sisters, (p0, p1) or (p2, p3) -- ab|cd, class 0, for every sorted row."""
    p = np.asarray(positions)
    assert (p[:, 1:] > p[:, :-1]).all()
    return np.zeros(len(p), dtype=np.int64)


def star_classes(positions):
    """A star: every MRCA is the root, no pairing stands out."""
    return np.full(len(positions), 3, dtype=np.int64)


def table_of(cx, cy):
    return np.bincount(4 * np.asarray(cx, dtype=np.int64) + np.asarray(cy, dtype=np.int64), minlength=16).reshape(4, 4)


# ---- trees ----------------------------------------------------------------------------------------------------------
def _lengths(parent, seed):
    dist = np.random.default_rng(seed).uniform(0.01, 2.0, len(parent)).astype(np.float32)
    dist[np.asarray(parent) < 0] = -1.0
    return dist


def star(n_leaves):
    """Node 0 is the root, nodes 1 .. n_leaves its children."""
    parent = np.zeros(n_leaves + 1, dtype=np.int32)
    parent[0] = -1
    return parent, _lengths(parent, n_leaves), np.arange(1, n_leaves + 1, dtype=np.int64)


def perfect_tree(levels):
    """Heap numbering: the children of node k are 2k + 1 and 2k + 2; leaf i from the left is node 2^levels - 1 + i."""
    n = (1 << (levels + 1)) - 1
    parent = ((np.arange(n, dtype=np.int64) - 1) // 2).astype(np.int32)
    parent[0] = -1
    return parent, _lengths(parent, levels), np.arange(1 << levels, dtype=np.int64) + (1 << levels) - 1


def caterpillar(n_leaves):
    """Backbone nodes 0 (the root) .. n_leaves - 2, node k + 1 below node k; leaf i hangs from backbone node
    min(i, n_leaves - 2): the leaves are listed from the shallowest to the two deepest."""
    spine = n_leaves - 1
    parent = np.empty(spine + n_leaves, dtype=np.int32)
    parent[:spine] = np.arange(spine) - 1
    parent[spine:] = np.minimum(np.arange(n_leaves), spine - 1)
    return parent, _lengths(parent, n_leaves), np.arange(n_leaves, dtype=np.int64) + spine


def random_general_tree(n_leaves, seed, max_arity=5):
    """(parent int32, dist float32, leaf_ids int64) of a random rooted tree whose inner nodes have 2 to ``max_arity``
    children, numbered by a random permutation, its leaves listed in random order: what a caller of the C ABI other than
    the facade may hand over.  Top down: a node over s > 1 leaves gets k = 2 .. min(max_arity, s) children, the s leaves
    dealt among them at random cut points."""
    rng = np.random.default_rng(seed)
    parent, leaves = [-1], []
    todo = [(0, n_leaves)]
    while todo:
        node, s = todo.pop()
        if s == 1:
            leaves.append(node)
            continue
        k = int(rng.integers(2, min(max_arity, s) + 1))
        cuts = np.sort(rng.choice(np.arange(1, s), k - 1, replace=False))
        for part in np.diff(np.concatenate([[0], cuts, [s]])):
            parent.append(node)
            todo.append((len(parent) - 1, int(part)))
    n = len(parent)
    label = rng.permutation(n)                                   # node v of the construction gets id label[v]
    out = np.empty(n, dtype=np.int32)
    built = np.asarray(parent, dtype=np.int64)
    out[label] = np.where(built < 0, -1, label[np.maximum(built, 0)])
    dist = rng.uniform(0.01, 2.0, n).astype(np.float32)
    dist[out < 0] = -1.0
    return out, dist, rng.permutation(label[np.asarray(leaves, dtype=np.int64)]).astype(np.int64)
