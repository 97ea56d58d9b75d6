"""A numpy restatement of the definitions of the per-clade Hommola test (include/suchtree_hip.h: st_hommola_clades_host),
written from the definitions and not from the package: the depth-first leaf orders, the layout of the links, the
permutation sigma of (seed, node, p, side, n) and the relabelled id rows whose st_compare_rows_host record every row of
the GPU path must equal."""
import numpy as np

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(z):
    """The splitmix64 finalizer on a Python int."""
    z &= MASK
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & MASK
    z ^= z >> 31
    return z


def mix_array(z):
    """The same on a uint64 array (numpy's unsigned arithmetic wraps mod 2^64)."""
    z = z.astype(np.uint64)
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def permutation(seed, node, p, side, n):
    """sigma: a link at universe position i is relabelled to position sigma[i]; p = 0 is the identity."""
    if p == 0:
        return np.arange(n, dtype=np.int64)
    h0 = mix(seed + (node + 1) * G)
    h1 = mix(h0 + (2 * p + side) * G)
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        w = (mix_array(np.uint64(h1) + (i + np.uint64(1)) * np.uint64(G)) & np.uint64(0xFFFFFFFFFFFF0000)) | i
    return (np.sort(w) & np.uint64(0xFFFF)).astype(np.int64)


def depth_first_leaves(parent, root=None):
    """(leaves in depth-first order with children in increasing id order, begin, count): every node's leaves are
    leaves[begin[v]: begin[v] + count[v]]; from ``root`` (default: the tree's root) down."""
    parent = np.asarray(parent)
    n = len(parent)
    kids = [[] for _ in range(n)]
    top = None
    for v in range(n):
        if parent[v] < 0:
            top = v
        else:
            kids[parent[v]].append(v)
    root = top if root is None else int(root)
    begin, count = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    leaves, stack = [], [(root, 0)]
    while stack:
        v, k = stack.pop()
        if k == 0:
            begin[v] = len(leaves)
            if not kids[v]:
                leaves.append(v)
        if k < len(kids[v]):
            stack.append((v, k + 1))
            stack.append((kids[v][k], 0))
        else:
            count[v] = len(leaves) - begin[v]
    return np.array(leaves, dtype=np.int64), begin, count


class Layout:
    """The universes, the links in layout order and every clade's ranges, for links given in rank order as (clade-tree
    leaf id, other-tree leaf id)."""

    def __init__(self, parent_clade, parent_other, ids_clade, ids_other, other_root=None):
        self.univ_c, self.leaf_begin, self.leaf_count = depth_first_leaves(parent_clade)
        self.univ_o, _, _ = depth_first_leaves(parent_other, other_root)
        where_c = {int(v): i for i, v in enumerate(self.univ_c)}
        where_o = {int(v): i for i, v in enumerate(self.univ_o)}
        pos_c = np.array([where_c[int(v)] for v in ids_clade], dtype=np.int64)
        self.order = np.argsort(pos_c, kind="stable")      # by clade leaf, rank order within a leaf
        self.pos_c = pos_c[self.order]
        self.pos_o = np.array([where_o[int(v)] for v in np.asarray(ids_other)[self.order]], dtype=np.int64)

    def links(self, node):
        """(link_begin, link_count) of a clade."""
        lo = int(np.searchsorted(self.pos_c, self.leaf_begin[node], side="left"))
        hi = int(np.searchsorted(self.pos_c, self.leaf_begin[node] + self.leaf_count[node], side="left"))
        return lo, hi - lo

    def rows(self, node, permutations, seed):
        """(ids_other, ids_clade): int64 (permutations + 1, links) id rows of clade ``node``, row p relabelled by
        permutation p -- over the clade's own leaf range on the clade side (side 0), over the whole other universe on
        the other side (side 1)."""
        lo, n = self.links(node)
        b, m = int(self.leaf_begin[node]), int(self.leaf_count[node])
        pc, po = self.pos_c[lo:lo + n], self.pos_o[lo:lo + n]
        ids_o = np.empty((permutations + 1, n), dtype=np.int64)
        ids_c = np.empty((permutations + 1, n), dtype=np.int64)
        for p in range(permutations + 1):
            ids_c[p] = self.univ_c[b + permutation(seed, int(node), p, 0, m)[pc - b]]
            ids_o[p] = self.univ_o[permutation(seed, int(node), p, 1, len(self.univ_o))[po]]
        return ids_o, ids_c
