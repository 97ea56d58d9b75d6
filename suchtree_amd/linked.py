"""SuchLinkedTrees: two trees and the links between their leaves.

Host-side mirror of the parts of the reference's ``SuchLinkedTrees``
(/root/reference/SuchTree/MuchTree.pyx:2525-3208) that feed or call the bulk
distance path: the link table and link list (:2560-2874), subsetting
(:2876-2898), ``linked_distances`` (:2900-2934) and the adjacency / Laplacian
assembly (:3081-3145).  The O(L^2) pair enumeration of ``linked_distances``
never exists in memory here: the kernels derive each pair from its index
(``st_triangle_host``).  ``sample_linked_distances`` keeps the reference's algorithm and
stop rule with numpy's generator in place of its xorshift64*; the igraph export is out of scope.
"""
from typing import Dict

import numpy as np

from . import _capi
from .suchtree import SuchTree, int_arg, seed_arg


class SuchLinkedTrees:
    def __init__(self, tree_a, tree_b, link_matrix):
        # trees: Newick path / string / URL, or existing SuchTree objects (pyx:2592-2609)
        if isinstance(tree_a, str):
            self._tree_a = SuchTree(tree_a)
        elif type(tree_a) == SuchTree:
            self._tree_a = tree_a
        else:
            raise Exception("unknown input for tree", type(tree_a))
        if isinstance(tree_b, str):
            self._tree_b = SuchTree(tree_b)
        elif type(tree_b) == SuchTree:
            self._tree_b = tree_b
        else:
            raise Exception("unknown input for tree", type(tree_b))
        A, B = self._tree_a, self._tree_b

        # the link matrix (a pandas DataFrame: rows = TreeA leaves, columns = TreeB leaves)
        if not link_matrix.shape == (A.num_leaves, B.num_leaves):
            raise Exception("link_matrix shape must match tree leaf counts")
        if not set(link_matrix.axes[0]) == set(A.leaves.keys()):
            raise Exception("axis[0] does not match TreeA leaf names")
        if not set(link_matrix.axes[1]) == set(B.leaves.keys()):
            raise Exception("axis[1] does not match TreeB leaf names")

        self._row_ids = np.array(list(A.leaves.values()))
        self._col_ids = np.array(list(B.leaves.values()))
        self._row_names = list(A.leaves.keys())
        self._col_names = list(B.leaves.keys())
        self._n_rows = A.num_leaves
        self._n_cols = B.num_leaves

        # reverse map for row ids (pyx:2629-2632)
        self._row_map = np.zeros(A.size, dtype=int)
        for n, i in enumerate(self._row_ids):
            self._row_map[i] = n
        # leaf id -> link-table column (the reference stores it in the leaf's right_child, pyx:1993-2003)
        self._col_of_leaf_b = {int(leaf): i for i, leaf in enumerate(self._col_ids)}
        self._row_of_leaf_a = {int(leaf): i for i, leaf in enumerate(self._row_ids)}
        for i, leaf in enumerate(self._col_ids):      # TreeB's leaves know their columns (pyx:2639)
            B.link_leaf(int(leaf), i)

        # the link table: per TreeB column (in TreeB leaf order) the linked TreeA leaf ids, in the
        # row order of the DataFrame (pyx:2637-2653)
        values = link_matrix.T.reindex(self._col_names)
        row_leaf = np.array([A.leaves[name] for name in values.columns], dtype=np.int64)
        mask = values.to_numpy() > 0
        self._table = [row_leaf[mask[i]] for i in range(self._n_cols)]
        self._n_links = int(sum(len(c) for c in self._table))

        # by default, the subset is the whole table (pyx:2655-2666)
        self._subset_a_root = A.root_node
        self._subset_b_root = B.root_node
        self._subset_a_size = len(self._row_ids)
        self._subset_b_size = len(self._col_ids)
        self._subset_rows = np.array(range(self._subset_a_size))
        self._subset_columns = np.array(range(self._subset_b_size))
        self._subset_a_leafs = self._row_ids
        self._subset_b_leafs = self._col_ids
        self._np_linklist = np.ndarray((self._n_links, 2), dtype=int)
        self._subset_n_links = 0
        self._seed = int(np.random.randint(0xFFFFFFFFFFFFFFFF >> 1))      # xorshift64* state (pyx:2572)
        self._build_linklist()

    # ------------------------------------------------------------ properties
    TreeA = property(lambda self: self._tree_a)
    TreeB = property(lambda self: self._tree_b)
    n_links = property(lambda self: self._n_links)
    n_cols = property(lambda self: self._n_cols)
    n_rows = property(lambda self: self._n_rows)
    col_ids = property(lambda self: self._col_ids)
    row_ids = property(lambda self: self._row_ids)
    col_names = property(lambda self: self._col_names)
    row_names = property(lambda self: self._row_names)
    subset_columns = property(lambda self: self._subset_columns)
    subset_rows = property(lambda self: self._subset_rows)
    subset_a_leafs = property(lambda self: self._subset_a_leafs)
    subset_b_leafs = property(lambda self: self._subset_b_leafs)
    subset_a_size = property(lambda self: self._subset_a_size)
    subset_b_size = property(lambda self: self._subset_b_size)
    subset_a_root = property(lambda self: self._subset_a_root)
    subset_b_root = property(lambda self: self._subset_b_root)
    subset_n_links = property(lambda self: self._subset_n_links)

    @property
    def linklist(self) -> np.ndarray:
        """(n_links, 2) array: column 0 = TreeB leaf id, column 1 = TreeA leaf id (pyx:2838-2874)."""
        return self._np_linklist[: self._subset_n_links, :]

    @property
    def linkmatrix(self) -> np.ndarray:
        """Boolean link matrix of the current subset (pyx:2812-2836)."""
        table = np.zeros((self._subset_a_size, self._subset_b_size), dtype=bool)
        in_a = set(int(x) for x in self._subset_a_leafs)
        for col in self._subset_columns:
            for m in self._table[col]:
                if int(m) in in_a:
                    table[self._row_map[m], col] = True
        return table

    def _build_linklist(self) -> None:
        """pyx:2846-2874: columns in subset order; within a column the table order, kept when the
        TreeA leaf is in the current row subset."""
        in_a = set(int(x) for x in self._subset_a_leafs)
        k = 0
        for col in self._subset_columns:
            for m in self._table[col]:
                if int(m) in in_a:
                    self._np_linklist[k, 0] = self._col_ids[col]
                    self._np_linklist[k, 1] = m
                    k += 1
        self._subset_n_links = k

    def get_column_leafs(self, col, as_row_ids=False) -> np.ndarray:
        col_id = self._col_names.index(col) if isinstance(col, str) else col
        if col_id > self._n_cols:
            raise Exception("col_id out of bounds", col_id)
        column = np.array(self._table[col_id], dtype=int)
        return self._row_map[column] if as_row_ids else column

    def get_column_links(self, col) -> np.ndarray:
        col_id = self._col_names.index(col) if isinstance(col, str) else col
        if col_id > self._n_cols:
            raise Exception("col_id out of bounds", col_id)
        column = np.zeros(self._n_rows, dtype=bool)
        column[self._row_map[np.array(self._table[col_id], dtype=int)]] = True
        return column

    # ------------------------------------------------------------- subsetting
    @staticmethod
    def _leaves_below(tree: SuchTree, node_id: int) -> np.ndarray:
        """Breadth-first leaf order of the reference's get_leaves (pyx:427-462)."""
        left, right = tree._flat.left, tree._flat.right
        to_visit = [int(node_id)]
        out = []
        for cur in to_visit:
            if left[cur] == -1:
                out.append(cur)
            else:
                to_visit.append(int(left[cur]))
                to_visit.append(int(right[cur]))
        return np.array(out, dtype=int)

    def subset_b(self, node_id) -> None:
        """Subset the link matrix to leaves descended from node_id in TreeB (pyx:2876-2886)."""
        if node_id > self._tree_b.size or node_id < 0:
            raise Exception("Node ID out of bounds.", node_id)
        self._subset_b_leafs = self._leaves_below(self._tree_b, node_id)
        self._subset_columns = np.array([self._col_of_leaf_b[int(x)] for x in self._subset_b_leafs], dtype=int)
        self._subset_b_size = len(self._subset_columns)
        self._subset_b_root = node_id
        self._build_linklist()

    def subset_a(self, node_id) -> None:
        """Subset the link matrix to leaves descended from node_id in TreeA (pyx:2888-2898)."""
        if node_id > self._tree_a.size or node_id < 0:
            raise Exception("Node ID out of bounds.", node_id)
        self._subset_a_leafs = self._leaves_below(self._tree_a, node_id)
        self._subset_rows = np.array([self._row_of_leaf_a[int(x)] for x in self._subset_a_leafs], dtype=int)
        self._subset_a_size = len(self._subset_rows)
        self._subset_a_root = node_id
        self._build_linklist()

    # ----------------------------------------------------- the distance caller
    def linked_distances(self) -> Dict[str, object]:
        """Distances in both trees for all pairs of links (pyx:2900-2934).

        Pair k = i(i-1)/2 + j (j < i) is (link j, link i): in TreeA the leaves
        ``(linklist[j,1], linklist[i,1])``, in TreeB ``(linklist[j,0], linklist[i,0])``.
        The id arrays are returned like the reference does, but the distances do not
        depend on them being materialised: each tree's kernel launch generates its pairs
        from the link-list column.
        """
        ll = np.ascontiguousarray(self.linklist, dtype=np.int64)
        L = ll.shape[0]
        size = (L * (L - 1)) // 2
        d_a, _ = self._tree_a._device_tree().triangle_host(ll[:, 1])
        d_b, _ = self._tree_b._device_tree().triangle_host(ll[:, 0])
        rows, cols = np.tril_indices(L, -1)
        ids_a = np.stack([ll[cols, 1], ll[rows, 1]], axis=1)
        ids_b = np.stack([ll[cols, 0], ll[rows, 0]], axis=1)
        return {"TreeA": d_a, "TreeB": d_b, "ids_A": ids_a, "ids_B": ids_b,
                "n_pairs": size, "n_samples": size, "deviation_a": None, "deviation_b": None}

    def linked_distances_summary(self, bins=None, range=None, spearman=False, kendall=False):
        """:meth:`linked_distances` reduced on the GPU: a :class:`~suchtree_amd.compare.DistanceComparison` of the same
        pairs with x = the TreeA column, y = the TreeB column (ids from ``linklist[:,1]`` / ``linklist[:,0]``), under the
        current ``subset_a`` / ``subset_b``.  No distance vector is materialised.  ``bins`` / ``range`` as in
        ``numpy.histogram2d`` (``range=None`` with integer bins costs a second pass).  ``spearman=True`` adds Spearman's rs
        of all pairs and its exact rank sums, ``kendall=True`` Kendall's tau-b and its exact counts (16 bytes of device
        memory per pair), as in :meth:`SuchTree.compare_distances`.  An extension: the reference
        has no counterpart (its notebooks correlate the two columns of linked_distances on the host)."""
        from . import compare
        ll = np.ascontiguousarray(self.linklist, dtype=np.int64)
        ids_a, ids_b = np.ascontiguousarray(ll[:, 1]), np.ascontiguousarray(ll[:, 0])
        dev_a, dev_b = self._tree_a._device_tree(), self._tree_b._device_tree()
        return compare.run(dev_a, dev_b, "triangle", (ids_a, ids_b), bins, range, int(ll.shape[0]), spearman, kendall)

    @staticmethod
    def _breadth_first(tree: SuchTree, node_id: int, leaves: bool) -> np.ndarray:
        """The leaves (:meth:`_leaves_below`) or the internal nodes (``get_internal_nodes``) below a node, breadth-first,
        one numpy step per level."""
        left, right = tree._flat.left, tree._flat.right
        level, out = np.array([int(node_id)], dtype=np.int64), []
        while level.size:
            leaf = left[level] == -1
            out.append(level[leaf] if leaves else level[~leaf])
            inner = level[~leaf]
            level = np.stack([left[inner], right[inner]], axis=1).ravel().astype(np.int64)
        return np.concatenate(out)

    @classmethod
    def _leaf_order(cls, tree: SuchTree, node_id: int) -> np.ndarray:
        return cls._breadth_first(tree, node_id, True)

    def _flat_table(self):
        """The link table as (TreeA leaf ids, column start offsets), built once."""
        if getattr(self, "_table_flat", None) is None:
            lens = np.array([len(c) for c in self._table], dtype=np.int64)
            start = np.zeros(len(lens) + 1, dtype=np.int64)
            np.cumsum(lens, out=start[1:])
            ids = np.concatenate([np.asarray(c, dtype=np.int64) for c in self._table]) if self._n_links else np.empty(0, np.int64)
            self._table_flat = (ids, start)
        return self._table_flat

    def _links_in_order(self, columns, a_leaves):
        """(TreeA ids, TreeB ids) of the links of ``columns`` (in that order; table order within a column) whose TreeA
        leaf is in ``a_leaves``: the link list _build_linklist would build, without touching the subset state."""
        ids, start = self._flat_table()
        columns = np.asarray(columns, dtype=np.int64)
        lens = start[columns + 1] - start[columns]
        total = int(lens.sum())
        first = np.repeat(start[columns] - np.concatenate(([0], np.cumsum(lens)[:-1])), lens)
        pos = first + np.arange(total, dtype=np.int64)
        a = ids[pos]
        b = np.repeat(self._col_ids[columns].astype(np.int64), lens)
        keep = np.zeros(self._tree_a.size, dtype=bool)
        keep[np.asarray(a_leaves, dtype=np.int64)] = True
        k = keep[a]
        return a[k], b[k]

    def linked_distances_by_clade(self, tree="B", min_leaves=0, min_links=2, max_links=None, chunk_pairs=0):
        """:meth:`linked_distances_summary` for every clade of one tree at once, in one pass over the pairs on the GPU.

        ``tree="B"``: one row per internal node c of TreeB, equal to what ``subset_b(c); linked_distances_summary()``
        gives under the current ``subset_a``; ``tree="A"``: the mirror, the clades of TreeA under the current
        ``subset_b``.  x is TreeA and y TreeB in both cases.  Rows follow ``get_internal_nodes()`` (breadth-first from
        the root) and are kept when ``n_leaves >= min_leaves``, ``n_links >= min_links`` and, unless ``max_links`` is
        None, ``n_links <= max_links`` -- the per-clade loop of the reference's SuchLinkedTrees notebook with its filters
        (``subset_b_size``, ``subset_n_links``).  A cap also saves work: only clades within it are evaluated.

        Each clade's per-pair values are bit-identical to its ``linked_distances()``: pair (link j, link i) of the clade
        is evaluated with the link of lower rank first, the rank being the position in the link list of the tree's
        root.  The subset state and ``linklist`` are the same after the call as before it.  Returns a
        :class:`~suchtree_amd.compare.CladeComparisons`; its ``pvalue`` column is NaN when scipy is not installed.
        ``chunk_pairs`` (a multiple of 8192, 0 = default) only sets the device chunk; results do not depend on it.
        An extension: the reference has no counterpart.
        """
        from . import compare
        if tree not in ("A", "B"):
            raise ValueError("tree must be 'A' or 'B'")
        A, B = self._tree_a, self._tree_b
        if tree == "B":
            col_of = np.full(B.size, -1, dtype=np.int64)
            col_of[self._col_ids.astype(np.int64)] = np.arange(len(self._col_ids))
            cols = col_of[self._leaf_order(B, B.root_node)]
            ids_a, ids_b = self._links_in_order(cols, self._subset_a_leafs)
            clade, other, ids_clade, ids_other = B, A, ids_b, ids_a
        else:
            ids_a, ids_b = self._links_in_order(self._subset_columns, self._leaf_order(A, A.root_node))
            clade, other, ids_clade, ids_other = A, B, ids_a, ids_b
        parent = np.ascontiguousarray(clade._flat.parent, dtype=np.int32)
        dev_o, dev_c = other._device_tree(), clade._device_tree()
        m, count = dev_o.compare_clades_host(dev_c, parent, ids_other, ids_clade, max_links=max_links, chunk_pairs=chunk_pairs)
        leaves = self._leaf_counts(clade)
        nodes = self._breadth_first(clade, clade.root_node, False)      # (get_internal_nodes() order)
        keep = (leaves[nodes] >= min_leaves) & (count[nodes] >= min_links) & (m["n"][nodes] >= 0)
        if max_links is not None:
            keep &= count[nodes] <= max_links
        nodes = nodes[keep]
        r = m[nodes]
        # x = the other tree in the call: for tree="A" that is TreeB, so the columns swap back
        sx, sy = ("x", "y") if tree == "B" else ("y", "x")
        sums = {"shift_x": r["shift_" + sx], "shift_y": r["shift_" + sy], "sx": r["s" + sx], "sy": r["s" + sy],
                "sxx": r["s" + sx + sx], "syy": r["s" + sy + sy], "sxy": r["sxy"]}
        return compare.CladeComparisons(nodes, leaves[nodes], count[nodes], sums, r["min_" + sx], r["max_" + sx], r["min_" + sy],
                                        r["max_" + sy], tree=tree)

    _HOMMOLA_IDS = 1 << 23      # ids per tree per library call: bounds the host memory of the rows

    def hommola_cospeciation(self, permutations=999, seed=None):
        """Hommola et al.'s (2009) permutation test of cospeciation on the current subset, with the semantics of
        scikit-bio's ``hommola_cospeciation`` (interaction matrix = ``linkmatrix``, distance matrices over
        ``subset_a_leafs`` / ``subset_b_leafs``, leaves without links included).

        Pearson's r over all pairs of links (x = TreeA, y = TreeB, the pairs of :meth:`linked_distances` in its
        orientation), then the r of ``permutations`` relabellings: per permutation, drawn in order from
        ``numpy.random.default_rng(seed)``, mp = a permutation of the TreeB leaves, then mh = one of the TreeA leaves,
        and every link's leaves are replaced by their images.  ``p_value`` = (count(perm_stats >= r) + 1) /
        (permutations + 1), NaN permuted r not counted; an observed r that is NaN (a constant column) gives a NaN p and
        NaN ``perm_stats`` without evaluating a permutation.  ``seed=None`` draws a seed and reports it.

        All rows are evaluated on the GPU in batched passes (st_compare_rows_host).  Each row's result depends on its
        links alone, so ``perm_stats[:k]`` is the same for any ``permutations >= k`` and the same seed, bit for bit.
        ValueError for fewer than 3 links or leaves, or a ``permutations`` that is not a non-negative integer.  The
        subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.HommolaResult`; ``r, p, stats = result`` works as with scikit-bio.
        An extension: the reference has no counterpart (its notebook samples instead).
        """
        import math
        from . import compare
        permutations = int_arg("permutations", permutations)
        ll = np.ascontiguousarray(self.linklist, dtype=np.int64)
        L = int(ll.shape[0])
        if L < 3:
            raise ValueError("Hommola's test needs at least 3 links; the subset has %d" % L)
        u_a = np.asarray(self._subset_a_leafs, dtype=np.int64)
        u_b = np.asarray(self._subset_b_leafs, dtype=np.int64)
        if len(u_a) < 3 or len(u_b) < 3:
            raise ValueError("Hommola's test needs at least 3 leaves in each tree; the subset has %d and %d" % (len(u_a), len(u_b)))
        if seed is None:
            seed = np.random.SeedSequence().entropy
        seed = int(seed)
        where_a = np.full(self._tree_a.size, -1, dtype=np.int64)
        where_a[u_a] = np.arange(len(u_a))
        where_b = np.full(self._tree_b.size, -1, dtype=np.int64)
        where_b[u_b] = np.arange(len(u_b))
        rows = compare.hommola_rows(u_a, u_b, where_a[ll[:, 1]], where_b[ll[:, 0]], permutations, seed,
                                    max(1, self._HOMMOLA_IDS // L))
        dev_a, dev_b = self._tree_a._device_tree(), self._tree_b._device_tree()
        m0 = dev_a.compare_rows_host(dev_b, *next(rows))[0]
        observed = compare.DistanceComparison.from_sums(*(m0[k] for k in _capi.PAIR_MOMENTS.names), n_leaves=L)
        perm_stats = np.full(permutations, np.nan)
        if not math.isnan(observed.pearson_r):
            done = 0
            for ids_a, ids_b in rows:
                m = dev_a.compare_rows_host(dev_b, ids_a, ids_b)
                perm_stats[done:done + len(m)] = compare.row_stats(m["n"], *(m[k] for k in compare._SUMS))[5]
                done += len(m)
        return compare.HommolaResult(observed.pearson_r, compare.hommola_pvalue(observed.pearson_r, perm_stats), perm_stats,
                                     observed, L, permutations, seed)

    _HOMMOLA_GROUP_ROWS = 1 << 21      # rows of st_pair_moments per library call of hommola_by_clade: bounds its host memory

    @staticmethod
    def _depth_first_leaves(tree: SuchTree):
        """(leaves, begin, count): the tree's leaves in depth-first order, children in increasing id order, and every
        node's range [begin, begin + count) of that order (st_clade_plan over one link per leaf)."""
        left = np.asarray(tree._flat.left)
        leaf_ids = np.flatnonzero(left == -1).astype(np.int64)
        plan = _capi.clade_plan(tree._flat.parent, leaf_ids)
        return leaf_ids[plan["perm"]], plan["begin"], plan["count"]

    def hommola_by_clade(self, tree="B", permutations=999, seed=None, nodes=None, min_leaves=3, min_links=3, max_links=None,
                         max_leaves=4096, keep_stats=False, chunk_blocks=0):
        """:meth:`hommola_cospeciation` for every clade of one tree at once, in one pass on the GPU.

        ``tree="B"``: one row per internal node c of TreeB under the current ``subset_a``, Hommola's test with scikit-bio's
        semantics on what ``subset_b(c)`` would select -- the links under c, the clade's leaves (linked or not) on the
        clade side, the current subset leaves of the other tree on the other side; ``tree="A"`` is the mirror.  x is TreeA
        and y TreeB in both cases.  Rows follow ``get_internal_nodes()`` order and are kept as in
        :meth:`linked_distances_by_clade` (``min_leaves``, ``min_links``, ``max_links``; fewer than 3 leaves or links never
        make a row); ``nodes=`` restricts them to the listed clade ids.  Clades of more than ``max_leaves`` leaves (at
        most 16384) are not evaluated and are listed in ``skipped_nodes``: the whole-tree test stays with
        :meth:`hommola_cospeciation`.

        ``corr_coeff`` is the r that :meth:`linked_distances_by_clade` reports for the clade, from a pass of its own.
        Each clade's distances are then computed once, as a matrix, and every permutation only relabels the links'
        positions in it.  Permutation p >= 1 of clade c on side s is ``compare.hommola_permutation(seed, c, p, s, n)`` over the
        side's leaves in depth-first order (children in increasing id order); it is generated on the GPU, and differs
        from the numpy draws of :meth:`hommola_cospeciation` with the same seed.  A clade's rows depend on (seed, c, its
        links, the two leaf sets) alone -- not on the other clades, ``nodes``, the filters or ``chunk_blocks`` -- and
        ``perm_stats[:, :k]`` is the same for any ``permutations >= k``.  ``seed=None`` draws a seed and reports it.
        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.CladeHommola`.  An extension: the reference has no counterpart (its
        notebook loops ``subset_b`` over the clades and keeps ``pearsonr``'s parametric p).
        """
        from . import compare
        if tree not in ("A", "B"):
            raise ValueError("tree must be 'A' or 'B'")
        permutations = int_arg("permutations", permutations)
        limit = _capi.HOMMOLA_MAX_UNIVERSE
        max_leaves = int_arg("max_leaves", max_leaves, limit)
        seed = seed_arg(seed)
        A, B = self._tree_a, self._tree_b
        if tree == "B":
            col_of = np.full(B.size, -1, dtype=np.int64)
            col_of[self._col_ids.astype(np.int64)] = np.arange(len(self._col_ids))
            ids_a, ids_b = self._links_in_order(col_of[self._leaf_order(B, B.root_node)], self._subset_a_leafs)
            clade, other, ids_clade, ids_other, other_root = B, A, ids_b, ids_a, self._subset_a_root
        else:
            ids_a, ids_b = self._links_in_order(self._subset_columns, self._leaf_order(A, A.root_node))
            clade, other, ids_clade, ids_other, other_root = A, B, ids_a, ids_b, self._subset_b_root
        univ_c, leaf_begin, leaves = self._depth_first_leaves(clade)
        o_leaves, o_begin, o_count = self._depth_first_leaves(other)
        univ_o = o_leaves[o_begin[other_root]: o_begin[other_root] + o_count[other_root]]
        if len(univ_o) < 3:
            raise ValueError("Hommola's test needs at least 3 leaves in each tree; the other tree's subset has %d" % len(univ_o))
        if len(univ_o) > limit:
            raise ValueError("the other tree's subset has %d leaves: at most %d (subset it first)" % (len(univ_o), limit))
        # the links laid out so that every clade's are one range; their positions in the two universes
        plan = _capi.clade_plan(clade._flat.parent, ids_clade)
        where_c = np.full(clade.size, -1, dtype=np.int64)
        where_c[univ_c] = np.arange(len(univ_c))
        where_o = np.full(other.size, -1, dtype=np.int64)
        where_o[univ_o] = np.arange(len(univ_o))
        pos_c = where_c[ids_clade[plan["perm"]]].astype(np.int32)
        pos_o = where_o[ids_other[plan["perm"]]].astype(np.int32)
        link_begin, count = plan["begin"], plan["count"]
        # rows
        rows = self._breadth_first(clade, clade.root_node, False)      # (get_internal_nodes() order)
        if nodes is not None:
            wanted = np.atleast_1d(np.asarray(nodes, dtype=np.int64))
            left = np.asarray(clade._flat.left)
            for v in wanted:
                if v < 0 or v >= clade.size or left[v] == -1:
                    raise ValueError("node %d is not an internal node of Tree%s" % (v, tree))
            rows = rows[np.isin(rows, wanted)]
        keep = (leaves[rows] >= max(int(min_leaves), 3)) & (count[rows] >= max(int(min_links), 3))
        if max_links is not None:
            keep &= count[rows] <= max_links
        rows = rows[keep]
        skipped = rows[leaves[rows] > max_leaves]
        rows = rows[leaves[rows] <= max_leaves]
        n = len(rows)
        # Groups of whole maximal clades -- within max_leaves, the parent not -- of about _HOMMOLA_GROUP_ROWS rows and at most
        # 16384 leaves: a call's clade-side universe is the leaf ranges of its maximal clades, one behind the other, and its
        # links are theirs.  (A clade's permutations run over its own leaf range, so the cut changes no result.)
        parent = np.asarray(clade._flat.parent)
        fits = leaves <= max_leaves
        top = np.flatnonzero(fits & ((parent < 0) | ~fits[np.maximum(parent, 0)]))
        top = top[np.argsort(leaf_begin[top])]
        owner = np.searchsorted(leaf_begin[top], leaf_begin[rows], side="right") - 1
        order = np.argsort(owner, kind="stable")
        n_ge, n_nan = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        stats = np.full((n, permutations), np.nan) if keep_stats else None
        dev_o, dev_c = other._device_tree(), clade._device_tree()
        # The observed r is the clade's r of linked_distances_by_clade: every pair with the link of lower rank first, as
        # subset_b(c) orders it.  (The permuted rows take a pair's links in layout order, and float32 distances are not
        # symmetric in their last bit: row 0 of the library call differs from this r at about 1e-8.)
        observed = np.zeros(n, dtype=_capi.PAIR_MOMENTS)
        if n:
            parent32 = np.ascontiguousarray(clade._flat.parent, dtype=np.int32)
            observed = dev_o.compare_clades_host(dev_c, parent32, ids_other, ids_clade, max_links=int(count[rows].max()))[0][rows]
        corr = compare.row_stats(observed["n"], *(observed[k] for k in compare._SUMS))[5]
        per_group = max(1, self._HOMMOLA_GROUP_ROWS // (permutations + 1))
        at = 0
        while at < n:
            end, span = at, 0
            while end < n:      # one more maximal clade with all its rows, while it fits
                o = owner[order[end]]
                stop = end
                while stop < n and owner[order[stop]] == o:
                    stop += 1
                if end > at and (stop - at > per_group or span + leaves[top[o]] > limit):
                    break
                end, span = stop, span + int(leaves[top[o]])
            idx = order[at:end]
            at = end
            v = rows[idx]
            tops = top[np.unique(owner[idx])]      # (by leaf_begin)
            leaf_off = np.concatenate(([0], np.cumsum(leaves[tops])[:-1])) - leaf_begin[tops]      # new position - old, per maximal clade
            link_off = np.concatenate(([0], np.cumsum(count[tops])[:-1])) - link_begin[tops]
            of = np.searchsorted(leaf_begin[tops], leaf_begin[v], side="right") - 1
            clades = np.zeros(len(v), dtype=_capi.HOMMOLA_CLADE)
            clades["node"], clades["leaf_begin"], clades["leaf_count"] = v, leaf_begin[v] + leaf_off[of], leaves[v]
            clades["link_begin"], clades["link_count"] = link_begin[v] + link_off[of], count[v]
            leaf_at = np.concatenate([np.arange(leaf_begin[t], leaf_begin[t] + leaves[t]) for t in tops])
            link_at = np.concatenate([np.arange(link_begin[t], link_begin[t] + count[t]) for t in tops])
            shift = np.repeat(leaf_off, count[tops]).astype(np.int32)
            m = dev_o.hommola_clades_host(dev_c, univ_o, univ_c[leaf_at], pos_o[link_at], pos_c[link_at] + shift, clades, permutations, seed,
                                          chunk_blocks)
            r = compare.row_stats(m["n"][:, 1:], *(m[k][:, 1:] for k in compare._SUMS))[5]
            with np.errstate(invalid="ignore"):
                n_ge[idx] = np.count_nonzero(r >= corr[idx, None], axis=1)
            n_nan[idx] = np.count_nonzero(np.isnan(r), axis=1)
            if keep_stats:
                stats[idx] = r
        if tree == "A":      # x = the other tree in the call: for tree="A" that is TreeB, so the columns swap back
            swapped = observed.copy()
            for a, b in (("shift_x", "shift_y"), ("sx", "sy"), ("sxx", "syy"), ("min_x", "min_y"), ("max_x", "max_y")):
                swapped[a], swapped[b] = observed[b], observed[a]
            observed = swapped
        return compare.CladeHommola(rows, leaves[rows], count[rows], observed, n_ge, n_nan, stats, permutations, seed, tree, skipped)

    def partner_dispersion(self, of="A", permutations=999, seed=None, pool="subset", min_partners=2, max_partners=None, keep_null=False,
                           null="taxa.labels", iterations=None):
        """Phylogenetic specificity: for each leaf, are its partners in the other tree close relatives of one another?

        ``of="A"``: one row per TreeA leaf of the current ``subset_a`` (in ``subset_a_leafs`` order) with at least
        ``min_partners`` -- and, unless ``max_partners`` is None, at most that many -- linked TreeB leaves inside the
        current ``subset_b``; the distances are TreeB's.  ``of="B"`` is the mirror.  Each row holds the MPD and MNTD of
        the leaf's partners and their standardised effect sizes against the null that shuffles the partner tree's leaf
        labels (:meth:`SuchTree.dispersion`, picante's ``ses.mpd`` / ``ses.mntd`` with ``null.model = "taxa.labels"``;
        NRI = -``mpd_ses``, NTI = -``mntd_ses``, ``mpd_p`` / ``mntd_p`` small for clustered partners).  ``pool`` is the
        universe whose labels are shuffled: ``"subset"`` = every leaf of the partner tree's current subset, ``"linked"`` =
        only those with a link in the current subset.  One shuffle serves every row: a row's null draws are uniform
        k-subsets of the universe, and the rows share the shuffles.  The shuffles are those of ``SuchTree.dispersion``
        with ``stream`` = the partner tree's subset root.  A universe of more than 16384 leaves is a ValueError: subset it
        first.  No row, nothing launched.

        ``null="swap"`` standardises against the degree-preserving swap null (:meth:`SuchTree.dispersion`): the link
        matrix is shuffled by chains of ``iterations`` trial swaps that keep every leaf's number of partners on both
        sides, so widespread partner leaves stay widespread in every draw.  The matrix is every leaf of the own subset
        with at least one partner in the universe; ``min_partners`` / ``max_partners`` only choose which rows are
        reported, a reported row's columns do not depend on them, and ``pool`` only bounds the universe (a column without
        links stays empty).  ``iterations=None`` is max(1000, 10 x the links), the library's own default.

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.SetDispersion` with ``leaves`` (the rows' leaf ids) and ``names``.
        An extension: the reference has no counterpart.
        """
        from .suchtree import null_model_arg
        null, iterations = null_model_arg(null, iterations)
        if null == "swap":
            lo = max(int_arg("min_partners", min_partners, optional=True) or 0, 1)
            hi = int_arg("max_partners", max_partners, optional=True)
            reported = []      # the rows of the matrix (one partner and more) that the call reports

            def run_swap(partner, sets, root, universe):
                reported.extend(i for i, s in enumerate(sets) if len(s) >= lo and (hi is None or len(s) <= hi))
                return partner.dispersion(sets, universe=universe, permutations=permutations, seed=seed, stream=root, keep_null=keep_null,
                                          null="swap", iterations=iterations, _report=reported)
            return self._over_partner_rows(of, 1, None, run_swap, pool, _capi.HOMMOLA_MAX_UNIVERSE, reported)

        def run(partner, sets, root, universe):
            return partner.dispersion(sets, universe=universe, permutations=permutations, seed=seed, stream=root, keep_null=keep_null)
        return self._over_partner_rows(of, min_partners, max_partners, run, pool, _capi.HOMMOLA_MAX_UNIVERSE)

    def _over_partner_rows(self, of, min_partners, max_partners, run, pool="subset", pool_limit=None, reported=None):
        """What partner_dispersion, partner_unifrac and partner_beta_dispersion share: the checks of ``of``, ``pool`` and the partner counts, the rows
        (_partner_rows), ``run(partner tree, the rows' partner ids, partner subset root, universe)``, then the result's
        ``leaves`` and ``names``.  With ``pool_limit`` the universe is ``pool`` of the partner tree -- "subset" = every leaf
        of its current subset, "linked" = those with a link in it -- of at most that many leaves; without, it is None."""
        if of not in ("A", "B"):
            raise ValueError("of must be 'A' or 'B'")
        if pool not in ("subset", "linked"):
            raise ValueError("pool must be 'subset' or 'linked'")
        min_partners = int_arg("min_partners", min_partners, optional=True)
        max_partners = int_arg("max_partners", max_partners, optional=True)
        ll = np.ascontiguousarray(self.linklist, dtype=np.int64)
        universe = None
        if pool_limit is not None:
            if pool == "subset":
                universe = np.asarray(self._subset_b_leafs if of == "A" else self._subset_a_leafs, dtype=np.int64)
            else:
                universe = np.unique(ll[:, 0 if of == "A" else 1])
            if len(universe) > pool_limit:      # (before the rows are built)
                raise ValueError("the partner tree's %s has %d leaves: at most %d (subset it first)"
                                 % ("subset" if pool == "subset" else "linked leaves", len(universe), pool_limit))
        own, partner, root, leaves, sets = self._partner_rows(of, min_partners, max_partners, ll)
        out = run(partner, sets, root, universe)
        if reported is not None:      # (the swap null: `run` reports these of the rows it was given)
            leaves = [leaves[i] for i in reported]
        out.leaves = np.asarray(leaves, dtype=np.int64)
        names = own.leaf_nodes
        out.names = [names[int(v)] for v in leaves]
        return out

    def _partner_rows(self, of, min_partners, max_partners, ll=None):
        """(own tree, partner tree, partner subset root, rows' leaf ids, rows' partner ids): the leaves of the current
        subset of tree ``of``, in subset order, with min_partners .. max_partners links inside the other subset.  ``ll``:
        the int64 ``linklist`` where the caller has read it already."""
        if ll is None:
            ll = np.ascontiguousarray(self.linklist, dtype=np.int64)
        if of == "A":
            own, partner, own_ids, partner_ids = self._tree_a, self._tree_b, ll[:, 1], ll[:, 0]
            own_leaves, root = self._subset_a_leafs, self._subset_b_root
        else:
            own, partner, own_ids, partner_ids = self._tree_b, self._tree_a, ll[:, 0], ll[:, 1]
            own_leaves, root = self._subset_b_leafs, self._subset_a_root
        by_leaf = {}      # leaf -> its partners' ids
        if len(ll):
            order = np.argsort(own_ids, kind="stable")
            ids, first, count = np.unique(own_ids[order], return_index=True, return_counts=True)
            by_leaf = {int(v): partner_ids[order[b:b + c]] for v, b, c in zip(ids, first, count)}
        leaves, sets = [], []
        for leaf in np.asarray(own_leaves, dtype=np.int64).tolist():
            partners = by_leaf.get(leaf)
            k = 0 if partners is None else len(partners)
            if k >= max(int(min_partners), 1) and (max_partners is None or k <= max_partners):
                leaves.append(leaf)
                sets.append(partners)
        return own, partner, int(root), leaves, sets

    def partner_unifrac(self, of="A", min_partners=1, max_partners=None, begin=0, count=None, shift=None):
        """How different are two leaves' partners: Faith's PD of every leaf's partner set and unweighted UniFrac between
        every two of them, measured on the partner tree.

        ``of="A"``: one row per TreeA leaf of the current ``subset_a`` (in ``subset_a_leafs`` order) with at least
        ``min_partners`` -- and, unless ``max_partners`` is None, at most that many -- linked TreeB leaves inside the
        current ``subset_b``, the row choice of :meth:`partner_dispersion`; the branch lengths are TreeB's, from its
        current subset root.  ``of="B"`` is the mirror.  ``begin`` / ``count`` / ``shift`` as in :meth:`SuchTree.unifrac`,
        which does the work: a sparse set merge over all row pairs on the GPU, no distance matrix, up to 2^20 partner
        leaves.  Two leaves with the same partners are at distance 0, two with partners in disjoint clades near 1.

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.SetUniFrac` with ``leaves`` (the rows' leaf ids), ``names`` and ``root``.
        An extension: the reference has no counterpart.
        """
        return self._over_partner_rows(of, min_partners, max_partners,
                                       lambda partner, sets, root, _: partner.unifrac(sets, root=root, begin=begin, count=count, shift=shift))

    def partner_beta_dispersion(self, of="A", pool="subset", min_partners=1, max_partners=None, begin=0, count=None, exclude_shared=False,
                                permutations=999, seed=None, keep_null=False):
        """How different are two leaves' partners, by distance: betaMPD and betaMNTD between every two leaves' partner
        sets, measured on the partner tree, with the taxa-labels null (betaNRI = ``beta_mpd_ses``, betaNTI =
        ``beta_mntd_ses``).

        ``of="A"``: one set per TreeA leaf of the current ``subset_a`` (in ``subset_a_leafs`` order) with at least
        ``min_partners`` -- and, unless ``max_partners`` is None, at most that many -- linked TreeB leaves inside the
        current ``subset_b``, the row choice of :meth:`partner_unifrac`; the distances are TreeB's.  ``of="B"`` is the
        mirror.  ``pool`` is the universe whose labels are shuffled, as in :meth:`partner_dispersion`; ``begin`` /
        ``count`` / ``exclude_shared`` / ``permutations`` / ``seed`` / ``keep_null`` as in
        :meth:`SuchTree.beta_dispersion`, which does the work with ``stream`` = the partner tree's subset root.  Two
        leaves with the same partners have ``beta_mntd`` 0.  A universe of more than 16384 leaves is a ValueError:
        subset it first.  No pair, nothing launched.

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.SetBetaDispersion` with ``leaves`` (the sets' leaf ids) and ``names``.
        An extension: the reference has no counterpart.
        """
        def run(partner, sets, root, universe):
            return partner.beta_dispersion(sets, universe=universe, begin=begin, count=count, exclude_shared=exclude_shared,
                                           permutations=permutations, seed=seed, stream=root, keep_null=keep_null)
        return self._over_partner_rows(of, min_partners, max_partners, run, pool, _capi.HOMMOLA_MAX_UNIVERSE)

    def partner_unifrac_null(self, of="A", pool="subset", min_partners=1, max_partners=None, begin=0, count=None, shift=None, permutations=999,
                             seed=None, keep_null=False):
        """Is a leaf's partner set, or the difference between two leaves' partner sets, more than its size explains:
        Faith's PD of every leaf's partners and UniFrac / PhyloSor between every two, standardised against the taxa-labels
        null (``pd_ses`` is picante's ``ses.pd``; ``unifrac_p_ge`` the label-shuffling significance of UniFrac).

        The rows are those of :meth:`partner_unifrac`: ``of="A"``, one set per TreeA leaf of the current ``subset_a`` (in
        ``subset_a_leafs`` order) with ``min_partners`` .. ``max_partners`` linked TreeB leaves inside the current
        ``subset_b``; the branch lengths are TreeB's, from its current subset root.  ``of="B"`` is the mirror.  ``pool`` is
        the universe whose labels are shuffled, as in :meth:`partner_dispersion`, and the shuffles are the same ones: the
        same ``seed`` and ``pool`` relabel the sets exactly as there (``stream`` = the partner tree's subset root).
        ``begin`` / ``count`` / ``shift`` / ``permutations`` / ``seed`` / ``keep_null`` as in :meth:`SuchTree.unifrac_null`,
        which does the work.  A universe of more than 16384 leaves is a ValueError: subset it first.

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.SetUniFracNull` with ``leaves`` (the sets' leaf ids), ``names`` and
        ``root``.  An extension: the reference has no counterpart.
        """
        def run(partner, sets, root, universe):
            return partner.unifrac_null(sets, universe=universe, root=root, begin=begin, count=count, shift=shift, permutations=permutations,
                                        seed=seed, stream=root, keep_null=keep_null)
        return self._over_partner_rows(of, min_partners, max_partners, run, pool, _capi.HOMMOLA_MAX_UNIVERSE)

    PHYLOSYMBIOSIS_MEASURES = ("unifrac", "phylosor", "beta_mpd", "beta_mntd")

    def phylosymbiosis(self, of="A", measure="unifrac", method="pearson", permutations=999, seed=None, alternative="greater", pool="subset",
                       min_partners=1, max_partners=None, exclude_shared=False, control=None, keep_stats=False, device=..., chunk_tasks=0):
        """Phylosymbiosis: do closely related leaves of one tree have similar partners in the other?  The Mantel test of
        the leaves' own tree distance against the distance between their partner sets.

        The rows are those of :meth:`partner_unifrac`: ``of="A"``, one per TreeA leaf of the current ``subset_a`` (in
        ``subset_a_leafs`` order) with ``min_partners`` .. ``max_partners`` linked TreeB leaves inside the current
        ``subset_b``; ``of="B"`` is the mirror.  x is the patristic distance between the row leaves in their own tree
        (:meth:`SuchTree.pairwise_distances`), y the ``measure`` between their partner sets, taken from the observed
        values of :meth:`partner_unifrac` ("unifrac", "phylosor") or :meth:`partner_beta_dispersion` ("beta_mpd",
        "beta_mntd", with ``pool`` and ``exclude_shared``).  ``control`` is an optional third matrix over the same rows
        (square, or condensed in the triangle order) for the partial test.  ``method``, ``permutations``, ``seed``,
        ``alternative`` (here "greater" by default: related leaves, similar partners), ``keep_stats`` and ``chunk_tasks``
        are those of :func:`~suchtree_amd.compare.mantel`, which relabels the row leaves on ``device`` (... = the row
        tree's device; None = only the permutations run on the host: the two matrices still come from the trees'
        kernels, so the call needs a GPU either way).  The call needs 3 to 16384 rows; a NaN in the measure (two
        leaves whose partner sets give a zero denominator) is a ValueError that names the pair.

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.MantelResult` with ``leaves`` (the rows' leaf ids), ``names`` and
        ``measure``.  An extension: the reference has no counterpart.
        """
        from . import compare
        if measure not in self.PHYLOSYMBIOSIS_MEASURES:
            raise ValueError("measure must be one of %s" % (self.PHYLOSYMBIOSIS_MEASURES,))
        if method not in compare.MANTEL_METHODS or alternative not in compare.MANTEL_ALTERNATIVES:
            raise ValueError("method must be one of %s and alternative one of %s" % (compare.MANTEL_METHODS, compare.MANTEL_ALTERNATIVES))
        int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1")
        int_arg("chunk_tasks", chunk_tasks)
        seed = seed_arg(seed)
        own, observed, x, y = self._phylosymbiosis_matrices(of, measure, pool, min_partners, max_partners, exclude_shared, control)
        out = compare.mantel(x, y, control, method=method, permutations=permutations, seed=seed, alternative=alternative, keep_stats=keep_stats,
                             device=own._device if device is ... else device, chunk_tasks=chunk_tasks)
        out.leaves, out.names, out.measure = observed.leaves, observed.names, measure
        return out

    def _phylosymbiosis_matrices(self, of, measure, pool, min_partners, max_partners, exclude_shared, control=None, with_x=True):
        """(the row tree, the observed measure over the partner rows, x: the row leaves' own tree distances -- None
        without ``with_x`` --, y: the ``measure`` between their partner sets) of :meth:`phylosymbiosis`; a NaN in y is its
        ValueError."""
        from . import compare
        by_distance = measure in ("beta_mpd", "beta_mntd")

        def run(partner, sets, root, universe):
            if len(sets) < 3 or len(sets) > _capi.HOMMOLA_MAX_UNIVERSE:      # (before anything is launched)
                raise ValueError("%d rows: 3 to %d" % (len(sets), _capi.HOMMOLA_MAX_UNIVERSE))
            if control is not None and compare.mantel_condensed(control, "control")[1] != len(sets):
                raise ValueError("control is not over the %d rows" % len(sets))
            if by_distance:
                return partner.beta_dispersion(sets, universe=universe, exclude_shared=exclude_shared, permutations=0, seed=0, stream=root)
            return partner.unifrac(sets, root=root)
        observed = self._over_partner_rows(of, min_partners, max_partners, run, pool, _capi.HOMMOLA_MAX_UNIVERSE if by_distance else None)
        y = np.asarray(getattr(observed, measure), dtype=np.float64)
        bad = np.flatnonzero(np.isnan(y))
        if len(bad):
            i, j = observed.pair(int(bad[0]))
            raise ValueError("%s of rows %d and %d (%s, %s) is NaN" % (measure, i, j, observed.names[i], observed.names[j]))
        own = self._tree_a if of == "A" else self._tree_b
        return own, observed, own.pairwise_distances(observed.leaves.tolist()) if with_x else None, y

    def phylosymbiosis_correlogram(self, of="A", measure="unifrac", n_classes=None, breaks=None, cutoff=True, method="pearson", permutations=999,
                                   seed=None, correction="holm", progressive=True, pool="subset", min_partners=1, max_partners=None,
                                   exclude_shared=False, keep_stats=False, device=..., chunk_tasks=0):
        """At which phylogenetic distances does phylosymbiosis sit?  The Mantel correlogram of the distance between the
        leaves' partner sets over the classes of the leaves' own tree distance: among sister species only, across
        genera, or with a change of sign at depth -- what the one r of :meth:`phylosymbiosis` cannot separate.

        The rows, x, y and ``measure`` (with ``pool``, ``min_partners``, ``max_partners`` and ``exclude_shared``) are
        those of :meth:`phylosymbiosis`; a NaN in the measure is the same ValueError.  ``n_classes``, ``breaks``,
        ``cutoff``, ``method``, ``permutations``, ``seed``, ``correction``, ``progressive``, ``keep_stats`` and
        ``chunk_tasks`` are those of :func:`~suchtree_amd.compare.mantel_correlogram`, which files every relabelled pair
        under its distance class in one pass on ``device`` (... = the row tree's device; None = only the permutations
        run on the host: the two matrices still come from the trees' kernels).  A class with a positive ``corr_coeff``
        holds leaves whose partners are more alike than average.

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.MantelCorrelogram`, one row per class, with ``leaves`` (the rows' leaf
        ids), ``names`` and ``measure``.  An extension: the reference has no counterpart.
        """
        from . import compare
        if measure not in self.PHYLOSYMBIOSIS_MEASURES:
            raise ValueError("measure must be one of %s" % (self.PHYLOSYMBIOSIS_MEASURES,))
        if method not in compare.MANTEL_METHODS or correction not in compare.MANTEL_CORRECTIONS:
            raise ValueError("method must be one of %s and correction one of %s" % (compare.MANTEL_METHODS, compare.MANTEL_CORRECTIONS))
        int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1")
        int_arg("chunk_tasks", chunk_tasks)
        seed = seed_arg(seed)
        own, observed, x, y = self._phylosymbiosis_matrices(of, measure, pool, min_partners, max_partners, exclude_shared)
        out = compare.mantel_correlogram(x, y, n_classes=n_classes, breaks=breaks, cutoff=cutoff, method=method, permutations=permutations, seed=seed,
                                         correction=correction, progressive=progressive, keep_stats=keep_stats,
                                         device=own._device if device is ... else device, chunk_tasks=chunk_tasks)
        out.leaves, out.names, out.measure = observed.leaves, observed.names, measure
        return out

    def _dendrogram_rows(self, of, measure, linkage, pool, min_partners, max_partners, exclude_shared):
        """(the row tree, the observed measure, y) of :meth:`partner_dendrogram` and :meth:`phylosymbiosis_topology`"""
        from . import compare
        if measure not in self.PHYLOSYMBIOSIS_MEASURES:
            raise ValueError("measure must be one of %s" % (self.PHYLOSYMBIOSIS_MEASURES,))
        if linkage not in compare.LINKAGE_METHODS:
            raise ValueError("linkage must be one of %s" % (compare.LINKAGE_METHODS,))
        own, observed, _, y = self._phylosymbiosis_matrices(of, measure, pool, min_partners, max_partners, exclude_shared, with_x=False)
        if len(observed.leaves) < 4:
            raise ValueError("%d rows: 4 to %d" % (len(observed.leaves), _capi.LINKAGE_MAX_OBJECTS))
        return own, observed, y

    def partner_dendrogram(self, of="A", measure="unifrac", linkage="average", pool="subset", min_partners=1, max_partners=None,
                           exclude_shared=False, device=...):
        """The dendrogram of the leaves of one tree by the similarity of their partners in the other: the partner-set
        distances of :meth:`phylosymbiosis`, clustered exactly.

        The rows and ``measure`` (with ``pool``, ``min_partners``, ``max_partners`` and ``exclude_shared``) are those of
        :meth:`phylosymbiosis`, a NaN in the measure is the same ValueError; 4 to 16384 rows.  ``linkage`` ("average" =
        UPGMA, "single", "complete") and ``device`` are those of :func:`~suchtree_amd.compare.linkage` (... = the host
        restatement below ``compare.LINKAGE_DEVICE_MIN`` rows, the row tree's device from there; the matrix still comes
        from the trees' kernels, so the call needs a GPU either way).

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.Dendrogram` with ``leaves`` (the rows' leaf ids), ``names`` and
        ``measure``.  An extension: the reference has no counterpart.
        """
        from . import compare
        own, observed, y = self._dendrogram_rows(of, measure, linkage, pool, min_partners, max_partners, exclude_shared)
        if device is ... and len(observed.leaves) >= compare.LINKAGE_DEVICE_MIN:
            device = own._device
        out = compare.linkage(y, linkage, device=device)
        out.leaves, out.names, out.measure = observed.leaves, observed.names, measure
        return out

    def phylosymbiosis_topology(self, of="A", measure="unifrac", linkage="average", rooted=True, min_branch=None, permutations=999, seed=None,
                                stream=0, pool="subset", min_partners=1, max_partners=None, exclude_shared=False, keep_stats=False, device=...):
        """Phylosymbiosis by topology (Brooks et al. 2016): is the dendrogram of the leaves' partner sets
        (:meth:`partner_dendrogram`) closer to the leaves' own tree than chance -- by Robinson-Foulds and by the transfer
        distance, against relabellings of the dendrogram's objects.  :meth:`phylosymbiosis` asks the same of the two
        distance matrices; this asks it of the two branching orders.

        The rows, ``measure``, ``pool``, ``min_partners``, ``max_partners`` and ``exclude_shared`` are those of
        :meth:`phylosymbiosis` (4 to 16384 rows); ``linkage``, ``rooted``, ``min_branch``, ``permutations``, ``seed``,
        ``stream``, ``keep_stats`` and ``device`` those of :meth:`SuchTree.dendrogram_congruence` on the row tree
        (``min_branch=0.0`` leaves out the clades that a broken tie made: leaves with identical partner sets).

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.TopologyTestResult` with ``leaves``, ``names`` and ``measure``.  An
        extension: the reference has no counterpart.
        """
        int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1")
        seed = seed_arg(seed)
        own, observed, y = self._dendrogram_rows(of, measure, linkage, pool, min_partners, max_partners, exclude_shared)
        out = own.dendrogram_congruence(y, observed.leaves, linkage=linkage, rooted=rooted, min_branch=min_branch, permutations=permutations, seed=seed,
                                        stream=stream, keep_stats=keep_stats, device=device)
        out.leaves, out.names, out.measure = observed.leaves, observed.names, measure
        return out

    def parafit(self, permutations=999, seed=None, shuffle="A", transform="sqrt", test_links=True, keep_stats=False):
        """ParaFit (Legendre, Desdevises & Bazin 2002) on the current subset: the global test of cophylogeny, and for every
        link ParaFitLink1 with a permutation test of its own -- which links carry the signal that
        :meth:`hommola_cospeciation` reports for the whole system.

        The links are those of the current subsets (``linklist``), the two distance matrices come from
        :meth:`SuchTree.pairwise_distances` over the subsets' leaves, each in its tree's depth-first order as in
        :meth:`partner_dispersion`.  ``shuffle="A"`` (default) is Legendre's null: for every TreeB leaf separately its
        partners are redrawn among the TreeA leaves of the current subset; ``shuffle="B"`` is the mirror.  With S the
        shuffled side (n_s leaves) and F the held one, permutation p >= 1 relabels the links of the F leaf with id v by
        ``compare.hommola_permutation(seed, v, p, 0, n_s)``; the links of one leaf keep distinct partners, different
        leaves draw independently.  ``transform``, ``test_links``, ``keep_stats`` and the definitions of the statistics
        and of the link test -- Link1_p(l), the statistic of the relabelled link l in the relabelled system, against the
        observed Link1_0(l); not claimed to equal ape's link p-values -- are those of
        :func:`~suchtree_amd.compare.parafit`, which does the work on the shuffled tree's device in one pass over the link
        pairs, in exact integers.  3 to 16384 links and leaves a side, else a ValueError.

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.ParaFitResult` with ``link_a`` / ``link_b`` (leaf ids, in ``linklist``
        order), ``link_names`` ((TreeA name, TreeB name) pairs) and ``shuffle``.  An extension: the reference has no
        counterpart.
        """
        from . import compare
        if shuffle not in ("A", "B"):
            raise ValueError("shuffle must be 'A' or 'B'")
        if transform not in compare.PARAFIT_TRANSFORMS:
            raise ValueError("transform must be one of %s" % (compare.PARAFIT_TRANSFORMS,))
        int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1")
        seed = seed_arg(seed)
        ll = np.ascontiguousarray(self.linklist, dtype=np.int64)
        limit = _capi.HOMMOLA_MAX_UNIVERSE
        if len(ll) < 3 or len(ll) > limit:
            raise ValueError("ParaFit needs 3 to %d links; the subset has %d" % (limit, len(ll)))
        sides = {}
        for name, tree, subset, col in (("A", self._tree_a, self._subset_a_leafs, 1), ("B", self._tree_b, self._subset_b_leafs, 0)):
            inside = np.zeros(tree.size, dtype=bool)
            inside[np.asarray(subset, dtype=np.int64)] = True
            univ = tree._depth_first_leaves()
            univ = univ[inside[univ]]
            if len(univ) < 3 or len(univ) > limit:
                raise ValueError("ParaFit needs 3 to %d leaves in each tree; the subset of Tree%s has %d" % (limit, name, len(univ)))
            where = np.full(tree.size, -1, dtype=np.int64)
            where[univ] = np.arange(len(univ))
            sides[name] = (tree, univ, where[ll[:, col]])
        (tree_s, univ_s, pos_s), (tree_f, univ_f, pos_f) = sides[shuffle], sides["B" if shuffle == "A" else "A"]
        out = compare.parafit(tree_f.pairwise_distances(univ_f.tolist()), tree_s.pairwise_distances(univ_s.tolist()), np.stack([pos_f, pos_s], axis=1),
                              permutations=permutations, seed=seed, shuffle_streams=univ_f, transform=transform, test_links=test_links,
                              keep_stats=keep_stats, device=tree_s._device)
        names_a, names_b = self._tree_a.leaf_nodes, self._tree_b.leaf_nodes
        out.shuffle, out.link_a, out.link_b = shuffle, ll[:, 1].copy(), ll[:, 0].copy()
        out.link_names = [(names_a[int(a)], names_b[int(b)]) for b, a in ll.tolist()]
        return out

    @staticmethod
    def _row_groups(own, leaves, groups):
        """The label of each row leaf of ``leaves`` under ``groups`` (None: in no group): a mapping from leaf name or id
        to a label, or a sequence of node ids of ``own`` whose clades are the groups.  ValueError for clades that overlap."""
        if hasattr(groups, "keys"):
            ids = own.leaves
            by_leaf = {(int(ids[k]) if isinstance(k, str) else int(k)): label for k, label in groups.items()}
        else:
            by_leaf = {}
            for node in groups:
                node = int(node)
                for leaf in own.get_leaves(node).tolist():
                    if leaf in by_leaf:
                        raise ValueError("clades %d and %d overlap: both hold leaf %d (%s)" % (by_leaf[leaf], node, leaf, own.leaf_nodes[leaf]))
                    by_leaf[leaf] = node
        return [by_leaf.get(int(v)) for v in leaves]

    def partner_group_differences(self, of="A", groups=None, measure="unifrac", test="permanova", permutations=999, seed=None, pool="subset",
                                  min_partners=1, max_partners=None, exclude_shared=False, keep_stats=False, device=..., chunk_tasks=0):
        """Do groups of leaves of one tree differ in their partners in the other?  PERMANOVA or ANOSIM of the distance
        between the leaves' partner sets against a grouping of the leaves.

        The rows and the ``measure`` between their partner sets are those of :meth:`phylosymbiosis`.  ``groups`` is a
        mapping from leaf name or leaf id to a label, or a sequence of internal node ids of the row leaves' own tree: a
        row then belongs to the listed clade that contains it, and listed clades that overlap are a ValueError that
        names both.  Rows in no group are left out of the test and listed, as leaf ids, in ``result.dropped``.  A NaN in
        the measure among the kept rows is a ValueError that names the pair.  ``test`` is "permanova" or "anosim";
        ``permutations``, ``seed``, ``keep_stats`` and ``chunk_tasks`` are those of
        :func:`~suchtree_amd.compare.permanova`, which relabels the kept rows on ``device`` (... = the row tree's
        device; None = only the permutations run on the host: the matrix still comes from the trees' kernels).

        The subset state, ``linklist`` and the generator of :meth:`sample_linked_distances` are left as they were.
        Returns a :class:`~suchtree_amd.compare.GroupTestResult` with ``leaves`` (the kept rows' leaf ids), ``names``,
        ``measure`` and ``dropped``.  An extension: the reference has no counterpart.
        """
        from . import compare
        if measure not in self.PHYLOSYMBIOSIS_MEASURES:
            raise ValueError("measure must be one of %s" % (self.PHYLOSYMBIOSIS_MEASURES,))
        if test not in compare.GROUP_TESTS:
            raise ValueError("test must be one of %s" % (compare.GROUP_TESTS,))
        if of not in ("A", "B"):
            raise ValueError("of must be 'A' or 'B'")
        if groups is None:
            raise ValueError("groups: a mapping from leaf to label, or a sequence of node ids")
        int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1")
        int_arg("chunk_tasks", chunk_tasks)
        seed = seed_arg(seed)
        own, _, _, row_leaves, _ = self._partner_rows(of, int_arg("min_partners", min_partners, optional=True),
                                                      int_arg("max_partners", max_partners, optional=True))
        labels = self._row_groups(own, row_leaves, groups)      # (before anything is launched)
        keep = np.array([k for k, g in enumerate(labels) if g is not None], dtype=np.int64)
        grouping = [labels[k] for k in keep.tolist()]
        if len(keep) < 3:
            raise ValueError("%d rows in a group: at least 3" % len(keep))
        compare.group_codes(grouping, len(keep))
        by_distance = measure in ("beta_mpd", "beta_mntd")

        def run(partner, sets, root, universe):
            if len(sets) > _capi.HOMMOLA_MAX_UNIVERSE:
                raise ValueError("%d rows: at most %d" % (len(sets), _capi.HOMMOLA_MAX_UNIVERSE))
            if by_distance:
                return partner.beta_dispersion(sets, universe=universe, exclude_shared=exclude_shared, permutations=0, seed=0, stream=root)
            return partner.unifrac(sets, root=root)
        observed = self._over_partner_rows(of, min_partners, max_partners, run, pool, _capi.HOMMOLA_MAX_UNIVERSE if by_distance else None)
        y = np.asarray(getattr(observed, measure), dtype=np.float64)
        i, j = np.tril_indices(len(keep), -1)
        ki, kj = keep[i], keep[j]      # (keep is increasing: ki > kj)
        sub = y[ki * (ki - 1) // 2 + kj]
        bad = np.flatnonzero(np.isnan(sub))
        if len(bad):
            a, b = int(ki[bad[0]]), int(kj[bad[0]])
            raise ValueError("%s of rows %d and %d (%s, %s) is NaN" % (measure, a, b, observed.names[a], observed.names[b]))
        fn = compare.permanova if test == "permanova" else compare.anosim
        out = fn(sub, grouping, permutations=permutations, seed=seed, keep_stats=keep_stats, device=own._device if device is ... else device,
                 chunk_tasks=chunk_tasks)
        kept = set(keep.tolist())
        out.leaves = observed.leaves[keep]
        out.names = [observed.names[k] for k in keep.tolist()]
        out.dropped = np.array([int(v) for k, v in enumerate(observed.leaves.tolist()) if k not in kept], dtype=np.int64)
        out.measure = measure
        return out

    @staticmethod
    def _leaf_counts(tree: SuchTree) -> np.ndarray:
        """Leaves under every node (st_clade_plan)."""
        return _capi.clade_plan(tree._flat.parent, np.empty(0, dtype=np.int64))["leaves"]

    def sample_linked_distances(self, sigma=0.001, buckets=64, n=4096, maxcycles=100, seed=None):
        """Monte-Carlo form of :meth:`linked_distances` (pyx:2951-3079): cycles of ``buckets`` x ``n`` random link
        pairs, distances in both trees, until the spread of the per-bucket standard deviations falls below ``sigma``
        in both trees (``None`` after ``maxcycles`` cycles).

        The reference's algorithm in the reference's arithmetic: link pairs from its xorshift64* generator
        (``st_link_sample_pairs``; the generator's state lives in the object as it does there and starts at a random
        value -- ``seed=`` sets it, an extension, so that a run can be repeated), the running sums in doubles
        element by element, the four bucket accumulators in C floats, ``pow`` for squares and roots
        (SuchTree/MuchTree.c:65197-65505).  What differs is the batching: one cycle is one launch per tree
        (``buckets * n`` pairs) instead of ``buckets`` calls of ``n`` pairs.
        """
        import math
        if seed is not None:
            self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        ll = np.ascontiguousarray(self.linklist, dtype=np.int64)
        if ll.shape[0] < 1:
            raise ValueError("no links in the current subset")
        buckets, n = int(buckets), int(n)
        sums_a, sums_b = np.zeros(buckets), np.zeros(buckets)
        sumsq_a, sumsq_b = np.zeros(buckets), np.zeros(buckets)
        samples = 0
        all_a, all_b = [], []
        cycles = 0

        def c_pow_half(x):      # C pow(x, 0.5): NaN for negative x, no exception
            return math.pow(x, 0.5) if x >= 0 else float("nan")

        f32 = np.float32
        while True:
            query_a, query_b, self._seed = _capi.link_sample_pairs(self._seed, ll, buckets * n)
            d_a = self._tree_a.distances_bulk(query_a).reshape(buckets, n)
            d_b = self._tree_b.distances_bulk(query_b).reshape(buckets, n)
            all_a.append(d_a.ravel())
            all_b.append(d_b.ravel())
            # sums[i] += d[i, j]; sumsq[i] += pow(d[i, j], 2.0), element by element onto the running values (pyx:3044-3048)
            _capi.bucket_moments(d_a, sums_a, sumsq_a)
            _capi.bucket_moments(d_b, sums_b, sumsq_b)
            samples += n
            dev_a = [c_pow_half(float(sumsq_a[i]) / float(samples) - math.pow(float(sums_a[i]) / float(samples), 2.0)) for i in range(buckets)]
            dev_b = [c_pow_half(float(sumsq_b[i]) / float(samples) - math.pow(float(sums_b[i]) / float(samples), 2.0)) for i in range(buckets)]
            # C floats: x = (float)((double)x + y)
            acc_a = acc_b = sq_a = sq_b = f32(0)
            for i in range(buckets):
                acc_a = f32(float(acc_a) + dev_a[i])
                acc_b = f32(float(acc_b) + dev_b[i])
                sq_a = f32(float(sq_a) + math.pow(dev_a[i], 2.0))
                sq_b = f32(float(sq_b) + math.pow(dev_b[i], 2.0))
            # (float)pow((double)(sq / (float)buckets - powf(acc / (float)buckets, 2.0f)), 0.5)
            mean_a, mean_b = f32(acc_a / f32(buckets)), f32(acc_b / f32(buckets))
            deviation_a = f32(c_pow_half(float(f32(f32(sq_a / f32(buckets)) - f32(mean_a * mean_a)))))
            deviation_b = f32(c_pow_half(float(f32(f32(sq_b / f32(buckets)) - f32(mean_b * mean_b)))))
            cycles += 1
            if deviation_a < sigma and deviation_b < sigma:
                break
            if cycles >= maxcycles:
                return None
        return {"TreeA": np.concatenate(all_a), "TreeB": np.concatenate(all_b),
                "n_pairs": (self._subset_n_links * (self._subset_n_links - 1)) / 2,
                "n_samples": n * buckets * cycles,
                "deviation_a": float(deviation_a), "deviation_b": float(deviation_b)}

    # ------------------------------------------- adjacency / Laplacian assembly
    @staticmethod
    def _tree_adjacency(tree: SuchTree, from_node):
        """SuchTree.adjacency_matrix (pyx:1750-1813) for the subtree below from_node."""
        r = tree.adjacency_matrix(int(from_node))
        return r["adjacency_matrix"], r["node_ids"]

    def _graph_edges(self, deletions=0, additions=0, swaps=0):
        """Edge list (u, v, weight) and size of the two-tree graph of pyx:3081-3131: tree edges
        normalised by each tree's longest edge, link edges at the mean of the two trees' mean
        (non-epsilon) normalised edge lengths; optional random link perturbations as the reference."""
        ta_aj, ta_ids = self._tree_adjacency(self._tree_a, self._subset_a_root)
        tb_aj, tb_ids = self._tree_adjacency(self._tree_b, self._subset_b_root)
        ta_node_ids, tb_node_ids = ta_ids.tolist(), tb_ids.tolist()
        ll = np.array(self.linklist)
        for _ in range(1, deletions):
            ll = np.delete(ll, np.random.randint(len(ll)), axis=0)
        for _ in range(1, swaps):
            x, y = np.random.choice(range(len(ll)), size=2, replace=False)
            ll[x, 1], ll[y, 1] = ll[y, 1], ll[x, 1]
        for _ in range(1, additions):
            a = np.random.choice(list(self._tree_a.leaves.values()))
            b = np.random.choice(list(self._tree_b.leaves.values()))
            ll = np.concatenate((ll, np.array([[b, a]])), axis=0)
        na, nb = ta_aj.shape[0], tb_aj.shape[0]
        a_index = {x: i for i, x in enumerate(ta_node_ids)}
        b_index = {x: i for i, x in enumerate(tb_node_ids)}
        ta_links = [a_index[int(x)] for x in ll[:, 1]]
        tb_links = [b_index[int(x)] + na for x in ll[:, 0]]
        ta_mean = np.mean(ta_aj.flatten()[ta_aj.flatten() > self._tree_a.polytomy_epsilon])
        tb_mean = np.mean(tb_aj.flatten()[tb_aj.flatten() > self._tree_b.polytomy_epsilon])
        link_mean = (ta_mean / ta_aj.max() + tb_mean / tb_aj.max()) / 2.0
        ua, va = np.nonzero(np.triu(ta_aj))
        ub, vb = np.nonzero(np.triu(tb_aj))
        u = np.concatenate([ua, ub + na, np.array(tb_links, dtype=np.int64)])
        v = np.concatenate([va, vb + na, np.array(ta_links, dtype=np.int64)])
        w = np.concatenate([ta_aj[ua, va] / ta_aj.max(), tb_aj[ub, vb] / tb_aj.max(),
                            np.full(len(ta_links), link_mean)])
        return na + nb, u, v, w

    def _matrices(self, deletions, additions, swaps, on_gpu, want_adjacency, want_laplacian):
        n, u, v, w = self._graph_edges(deletions, additions, swaps)
        if on_gpu:
            from . import _capi
            return _capi.graph_matrices(n, u, v, w, device=self._tree_a._device,
                                        want_adjacency=want_adjacency, want_laplacian=want_laplacian)
        aj = np.zeros((n, n))
        aj[u, v] = w
        aj[v, u] = w
        lp = None
        if want_laplacian:
            lp = np.zeros(aj.shape)
            np.fill_diagonal(lp, aj.sum(axis=0))
            lp = lp - aj
        return (aj if want_adjacency else None), lp

    def adjacency(self, deletions=0, additions=0, swaps=0, on_gpu=True) -> np.ndarray:
        """Graph adjacency matrix of both (subsetted) trees plus the link edges (pyx:3081-3131).
        The dense matrix is assembled on the GPU (``st_graph_matrices_host``); ``on_gpu=False``
        assembles it with numpy exactly as the reference does."""
        return self._matrices(deletions, additions, swaps, on_gpu, True, False)[0]

    def laplacian(self, deletions=0, additions=0, swaps=0, on_gpu=True) -> np.ndarray:
        """Graph Laplacian L = D - A of the current subset (pyx:3133-3145)."""
        return self._matrices(deletions, additions, swaps, on_gpu, False, True)[1]

    def spectrum(self, deletions=0, additions=0, swaps=0, on_gpu=True) -> np.ndarray:
        """Eigenvalues of the Laplacian by LAPACK's dsyev, as the reference calls it (pyx:3147-3173: jobz 'N', uplo 'U',
        workspace (4 + 2) N; scipy's LAPACK, the library the reference's `cython_lapack.dsyev` binds); the LAPACK info
        code if the solver fails.  The eigen-solve stays on the host."""
        lp = self.laplacian(deletions=deletions, additions=additions, swaps=swaps, on_gpu=on_gpu)
        try:
            from scipy.linalg.lapack import dsyev
        except ImportError:      # no scipy: numpy's symmetric solver (dsyevd), same values to rounding
            return np.linalg.eigvalsh(lp)
        w, _, info = dsyev(lp, compute_v=0, lower=0, lwork=6 * lp.shape[0])
        return w if info == 0 else info

    def to_igraph(self, deletions=0, additions=0, swaps=0):
        """The current subgraph as a weighted, labelled igraph object (pyx:3175-3198); igraph must be installed."""
        try:
            from igraph import ADJ_UNDIRECTED, Graph
        except ImportError:
            raise Exception("igraph package not installed.")
        g = Graph.Weighted_Adjacency(self.adjacency(deletions=deletions, additions=additions, swaps=swaps).tolist(),
                                     mode=ADJ_UNDIRECTED)
        na = len(list(self._tree_a.get_descendants(self._subset_a_root)))
        nb = len(list(self._tree_b.get_descendants(self._subset_b_root)))
        g.vs["color"] = ["#e1e329ff"] * na + ["#24878dff"] * nb
        g.vs["label"] = ["h" + str(i) for i in range(na)] + ["g" + str(i) for i in range(nb)]
        g.vs["tree"] = [0] * na + [1] * nb
        return g

    def dump_table(self) -> None:
        """Print the link matrix, one line per TreeB column (pyx:3200-3208)."""
        for i in range(self._n_cols):
            print("column", i, ":", ",".join(str(int(x)) for x in self._table[i]))
