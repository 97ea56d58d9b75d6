"""The SuchTree class surface for the bulk distance / MRCA path.

Host-side mirror of the reference's extension type
(/root/reference/SuchTree/MuchTree.pyx:89-2518): same constructor dispatch,
property names (and deprecated aliases), method names, argument conventions,
return types, exceptions and warnings for everything on the hot path; the
reference's navigation methods around it (node tests, lineages, traversals,
bipartitions, RED) come from navigate.py.  All arithmetic happens in
libsuchtree_hip.so on the GPU; nothing here computes a distance or an MRCA on
the CPU, and a missing library or GPU raises ``HipBackendError``.
"""
import math
import os
from itertools import chain
from numbers import Integral
from typing import Dict, List, Tuple, Union
from urllib.parse import urlparse
from warnings import warn

import numpy as np

from . import _capi
from .exceptions import InvalidNodeError, NodeNotFoundError
from .navigate import TreeNavigation
from .newick import EPSILON, FlatTree, flat_tree_from_arrays, flat_tree_from_newick

_NAMES_EXT = False      # not looked for yet


def _names_ext():
    """The optional _names extension (host-side name -> id loop of distances_by_name), or None."""
    global _NAMES_EXT
    if _NAMES_EXT is False:
        try:
            from . import _names
            _NAMES_EXT = _names
        except ImportError:
            try:                                    # not built yet: a one-second gcc job
                from . import build as _build
                _build.build_names_ext()
                from . import _names
                _NAMES_EXT = _names
            except Exception:                       # noqa: BLE001 -- no compiler, read-only tree, ...
                _NAMES_EXT = None
    return _NAMES_EXT


def _deprecation_warning(old_name: str, new_name: str, version: str = "2.0") -> None:
    # wording of MuchTree.pyx:33-42
    warn(
        f"{old_name} is deprecated and will be removed in SuchTree {version}. "
        f"Use {new_name} instead.",
        DeprecationWarning,
        stacklevel=3,
    )


def int_arg(name, v, top=None, top_text=None, optional=False):
    """The argument ``v`` as an int: a non-negative integer (no bool), at most ``top`` where one is given (``top_text``
    words it in the message); None passes where ``optional``.  ValueError otherwise."""
    if v is None and optional:
        return None
    if isinstance(v, bool) or not isinstance(v, Integral) or v < 0 or (top is not None and v > top):
        if top is None:
            raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
        raise ValueError("%s must be an integer from 0 to %s, got %r" % (name, top_text or top, v))
    return int(v)


def _null_args(permutations, seed, stream, chunk_tasks):
    """The arguments of a permutation null (``dispersion``, ``beta_dispersion``, ``unifrac_null``), checked in this order."""
    return (int_arg("permutations", permutations), seed_arg(seed), int_arg("stream", stream, (1 << 31) - 1, "2^31 - 1"),
            int_arg("chunk_tasks", chunk_tasks))


def null_model_arg(null, iterations):
    """The null model of ``dispersion`` / ``partner_dispersion``: "taxa.labels" or "swap"; ``iterations`` (None or a
    non-negative integer) belongs to "swap" alone.  ValueError otherwise."""
    if null not in ("taxa.labels", "swap"):
        raise ValueError("null must be 'taxa.labels' or 'swap', got %r" % (null,))
    if null == "taxa.labels" and iterations is not None:
        raise ValueError("iterations belongs to null='swap': the taxa.labels null has no chain")
    return null, int_arg("iterations", iterations, optional=True)


def _triangle_range(n_rows, begin, count):
    """(begin, count) of pairs [begin, begin + count) of the triangle over ``n_rows`` sets; ``count`` None = up to the last
    pair, which above 2^31 pairs is a ValueError."""
    total = n_rows * (n_rows - 1) // 2
    if count is None and total - begin > 1 << 31:
        raise ValueError("the whole triangle of %d sets is %d pairs, more than 2^31: ask for ranges with begin= and count=" % (n_rows, total))
    return _capi._unifrac_range(n_rows, begin, count, 0)


def seed_arg(seed):
    """A 64-bit seed: the caller's, or a fresh draw where it is None."""
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, np.uint64)[0])
    return int_arg("seed", seed, (1 << 64) - 1, "2^64 - 1")


class SuchTree(TreeNavigation):
    """Immutable phylogenetic tree resident in GPU memory.

    ``tree_input`` follows the reference (MuchTree.pyx:138-155): a URL, a Newick
    string, or a path to a Newick file.  As an extension it may also be a
    :class:`~suchtree_amd.newick.FlatTree` or a ``(parent, distance[, leaf_names])``
    tuple of flat arrays in the reference's in-order numbering.

    ``device``: HIP device index the tree is uploaded to (on first use).
    ``devices``: list of HIP device indices instead: the tree is replicated on all of them and
    the bulk methods taking host arrays (``distances_bulk``, ``pairwise_distances``, ...) deal
    their work over every listed GPU from this one process.
    ``strategy``: ``'auto'`` | ``'canopy'`` | ``'walk'`` kernel family.
    """

    def __init__(self, tree_input, device: int = 0, strategy: str = "auto", devices=None, table_mb=None):
        self._epsilon = EPSILON
        if isinstance(tree_input, FlatTree):
            flat = tree_input
        elif isinstance(tree_input, tuple):
            flat = flat_tree_from_arrays(*tree_input)
        elif isinstance(tree_input, str):
            if urlparse(tree_input).scheme in ("http", "https", "ftp"):
                from urllib.request import urlopen
                with urlopen(tree_input) as fh:
                    text = fh.read().decode("utf-8")
            elif all(["(" in tree_input,
                      ")" in tree_input,
                      tree_input.count("(") == tree_input.count(")"),
                      tree_input.endswith(";")]):
                text = tree_input
            else:
                with open(tree_input) as fh:
                    text = fh.read()
            flat = flat_tree_from_newick(text)
        else:
            raise TypeError("tree_input must be a str, FlatTree or (parent, distance) tuple")
        self._flat = flat
        self._devices = None if devices is None else [int(d) for d in devices]
        if self._devices is not None and not self._devices:
            raise ValueError("devices must not be empty")
        self._device = int(device) if self._devices is None else self._devices[0]
        if strategy not in _capi.STRATEGY:
            raise ValueError("strategy must be one of %s" % sorted(_capi.STRATEGY))
        self._strategy = strategy
        self._table_mb = table_mb      # budget (MiB) of the device tables: _capi.DeviceTree
        self._dev_tree = None

    # ------------------------------------------------------------------ device
    def _device_tree(self) -> "_capi.DeviceTree":
        """Upload on first use; raises HipBackendError without a usable GPU."""
        if self._dev_tree is not None and self._dev_tree._pid != os.getpid():
            # inherited through fork: the handle belongs to the parent's GPU context.  Drop it
            # (without destroying it); the upload below raises the explanatory HipBackendError
            # if the parent had initialised the GPU, which a resident tree implies.
            self._dev_tree = None
        if self._dev_tree is None:
            self._dev_tree = _capi.DeviceTree(self._flat.parent, self._flat.distance,
                                              device=self._device, strategy=self._strategy,
                                              devices=self._devices, table_mb=self._table_mb)
        return self._dev_tree

    def to_device(self) -> "SuchTree":
        """Force the upload now (otherwise it happens at the first query)."""
        self._device_tree()
        return self

    def device_info(self) -> dict:
        """Kernel family, canopy / understory geometry and HBM footprint."""
        return self._device_tree().info()

    def close(self) -> None:
        """Release the GPU copy (it is re-created on the next query)."""
        if self._dev_tree is not None:
            self._dev_tree.close()
            self._dev_tree = None

    # trees travel between processes (spawn / pickle) as their flat arrays; every process uploads
    # its own copy.  The reference's users parallelise with fork pools
    # (docs/examples/SuchTree_examples.md:462-497): that works here as long as the pool forks
    # before the parent's first GPU query (uploads are lazy); a child forked later gets a
    # HipBackendError saying so instead of a hang (see _capi._check_fork).
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_dev_tree"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._dev_tree = None

    def __repr__(self) -> str:
        return "<SuchTree %d nodes, %d leaves, depth %d, device %d%s>" % (
            self.size, self.num_leaves, self.depth, self._device,
            "" if self._dev_tree is None else ", resident")

    # -------------------------------------------------------------- properties
    @property
    def size(self) -> int:
        """The number of nodes in the tree."""
        return self._flat.size

    @property
    def depth(self) -> int:
        """The maximum depth of the tree (nodes on the longest leaf-to-root path)."""
        return self._flat.depth

    @property
    def num_leaves(self) -> int:
        return self._flat.num_leaves

    @property
    def leaves(self) -> Dict[str, int]:
        """Dictionary mapping leaf names to node IDs."""
        return self._flat.leaves

    @property
    def leaf_nodes(self) -> Dict[int, str]:
        """Dictionary mapping leaf node IDs to names."""
        return self._flat.leaf_nodes

    @property
    def root_node(self) -> int:
        return self._flat.root

    @property
    def internal_nodes(self) -> np.ndarray:
        return self._flat.internal_nodes

    @property
    def all_nodes(self) -> np.ndarray:
        return np.concatenate((np.array(list(self.leaves.values())),
                               np.array(list(self.internal_nodes))))

    @property
    def leaf_node_ids(self) -> np.ndarray:
        return np.array(list(self.leaves.values()))

    @property
    def leaf_names(self) -> list:
        return list(self.leaves.keys())

    @property
    def polytomy_epsilon(self) -> float:
        return self._epsilon

    @polytomy_epsilon.setter
    def polytomy_epsilon(self, new_epsilon: float) -> None:
        # like the reference (MuchTree.pyx:298-301) this does not rewrite stored lengths
        self._epsilon = new_epsilon

    # deprecated aliases (MuchTree.pyx:2374-2414)
    @property
    def length(self) -> int:
        _deprecation_warning("length property", "size")
        return self.size

    @property
    def leafs(self) -> dict:
        _deprecation_warning("leafs property", "leaves")
        return self.leaves

    @property
    def leafnodes(self) -> dict:
        _deprecation_warning("leafnodes property", "leaf_nodes")
        return self.leaf_nodes

    @property
    def n_leafs(self) -> int:
        _deprecation_warning("n_leafs property", "num_leaves")
        return self.num_leaves

    @property
    def root(self) -> int:
        _deprecation_warning("root property", "root_node")
        return self.root_node

    @property
    def polytomy_distance(self) -> float:
        _deprecation_warning("polytomy_distance property", "polytomy_epsilon")
        return self.polytomy_epsilon

    @polytomy_distance.setter
    def polytomy_distance(self, value: float) -> None:
        _deprecation_warning("polytomy_distance property", "polytomy_epsilon")
        self.polytomy_epsilon = value

    # ------------------------------------------------------------- validation
    def _validate_node(self, node: Union[int, str]) -> int:
        """MuchTree.pyx:2255-2284."""
        if isinstance(node, str):
            if node not in self.leaves:
                raise NodeNotFoundError(node)
            return self.leaves[node]
        if not isinstance(node, Integral):
            raise TypeError("Node must be int or str, got {t}".format(t=str(type(node))))
        node_id = int(node)
        if node_id < 0 or node_id >= self.size:
            raise InvalidNodeError(node_id, self.size)
        return node_id

    def _validate_node_pair(self, a, b) -> Tuple[int, int]:
        return self._validate_node(a), self._validate_node(b)

    # -------------------------------------------------- cheap harness lookups
    def get_parent(self, node: Union[int, str]) -> int:
        return int(self._flat.parent[self._validate_node(node)])

    def get_children(self, node: Union[int, str]) -> Tuple[int, int]:
        i = self._validate_node(node)
        return int(self._flat.left[i]), int(self._flat.right[i])

    def get_support(self, node: Union[int, str]) -> float:
        return float(self._flat.support[self._validate_node(node)])

    def is_leaf(self, node: Union[int, str]) -> bool:
        return bool(self._flat.left[self._validate_node(node)] == -1)

    def get_ancestors(self, node: Union[int, str]):
        i = self._validate_node(node)
        parent = self._flat.parent
        while True:
            p = int(parent[i])
            if p == -1:
                break
            yield p
            i = p

    # ----------------------------------------------------------- the hot path
    def _coerce_pairs(self, pairs) -> np.ndarray:
        """Input conventions of distances_bulk (MuchTree.pyx:889-894)."""
        if not isinstance(pairs, np.ndarray):
            pairs = np.array(pairs, dtype=np.int64)
        if pairs.ndim != 2 or pairs.shape[1] != 2:
            # (a 1-D array raises IndexError here, exactly like the reference's formatting)
            shape = str((pairs.shape[0], pairs.shape[1]))
            raise ValueError("Expected (n, 2) array, got shape {shape}".format(shape=shape))
        if pairs.dtype != np.int64:
            if not np.issubdtype(pairs.dtype, np.integer):
                raise ValueError("Buffer dtype mismatch, expected 'long' but got '%s'" % pairs.dtype.name)
            # more permissive than the reference (which only takes int64): int32 goes to the
            # library as it is, other integer widths are widened
            if pairs.dtype != np.int32:
                pairs = pairs.astype(np.int64)
        if pairs.shape[0] == 0:
            pairs.max()   # the reference fails here: ValueError (zero-size array to reduction ...)
        return pairs

    def distances_bulk(self, pairs) -> np.ndarray:
        """Patristic distances for an (n, 2) array of node-id pairs.

        Stands in for MuchTree.pyx:872-909 + ``_distances`` (:911-943): float64
        array holding the reference's float32 ordered sums.
        Raises ValueError for a wrong shape, InvalidNodeError for an id outside
        ``[0, size)`` (the id reported follows MuchTree.pyx:897-903).
        """
        pairs = self._coerce_pairs(pairs)
        dist, _ = self._device_tree().distances_host(pairs, want_dist=True, want_mrca=False)
        return dist

    def common_ancestors_bulk(self, pairs) -> np.ndarray:
        """MRCA node ids (int32) for an (n, 2) array of node-id pairs.

        The reference has no bulk MRCA call; this equals a loop over
        ``common_ancestor`` (MuchTree.pyx:1128-1149) and uses the same kernels.
        """
        pairs = self._coerce_pairs(pairs)
        _, mrca = self._device_tree().distances_host(pairs, want_dist=False, want_mrca=True)
        return mrca

    def distances_and_ancestors_bulk(self, pairs) -> Tuple[np.ndarray, np.ndarray]:
        """(distances float64[n], MRCA ids int32[n]) from one kernel launch."""
        pairs = self._coerce_pairs(pairs)
        return self._device_tree().distances_host(pairs, want_dist=True, want_mrca=True)

    def distance(self, a: Union[int, str], b: Union[int, str]) -> float:
        """Patristic distance between two nodes (MuchTree.pyx:852-870, 981-997)."""
        node_a, node_b = self._validate_node_pair(a, b)
        pairs = np.array([[node_a, node_b]], dtype=np.int64)
        dist, _ = self._device_tree().distances_host(pairs, want_dist=True, want_mrca=False)
        return float(dist[0])

    def distances_by_name(self, pairs: List[Tuple[str, str]]) -> List[float]:
        """Distances for (leaf_name, leaf_name) tuples (MuchTree.pyx:945-979)."""
        if not isinstance(pairs, list):
            raise TypeError("pairs must be a list of tuples")
        leaves = self.leaves
        names_ext = _names_ext()
        if names_ext is not None and pairs:
            # fastest path: the lookup loop in C (csrc/names_ext.c); -1 = something unexpected,
            # left to the code below
            ids = np.empty((len(pairs), 2), dtype=np.int64)
            if names_ext.lookup_pairs(pairs, leaves, ids) == 0:
                return self.distances_bulk(ids).tolist()
        try:
            # fast path: the dict lookups run at C speed over the flattened names, no per-element
            # checks (keys are str only, so anything that is not a known leaf name raises here
            # and is diagnosed by the loop below, which owns the error messages)
            if set(map(len, pairs)) - {2}:
                raise ValueError("a pair does not have two elements")
            ids = np.fromiter(map(leaves.__getitem__, chain.from_iterable(pairs)),
                              dtype=np.int64, count=2 * len(pairs))
        except (KeyError, TypeError, ValueError):
            ids = None
        if ids is not None:
            # (an empty list becomes the 1-D empty array of the reference and fails the shape check)
            return self.distances_bulk(ids.reshape(-1, 2) if len(pairs) else ids).tolist()
        node_pairs = []
        for i, (name_a, name_b) in enumerate(pairs):
            if not isinstance(name_a, str) or not isinstance(name_b, str):
                raise TypeError("Pair {i}: both elements must be strings".format(i=str(i)))
            if name_a not in leaves:
                raise NodeNotFoundError(name_a)
            if name_b not in leaves:
                raise NodeNotFoundError(name_b)
            node_pairs.append((leaves[name_a], leaves[name_b]))
        pairs_array = np.array(node_pairs, dtype=np.int64)
        return self.distances_bulk(pairs_array).tolist()

    def _name_ids(self, names) -> np.ndarray:
        """Leaf ids of ``names`` (NodeNotFoundError for an unknown one, as distances_by_name raises)."""
        leaves = self.leaves
        out = np.empty(len(names), dtype=np.int64)
        for i, name in enumerate(names):
            if name not in leaves:
                raise NodeNotFoundError(name)
            out[i] = leaves[name]
        return out

    def shared_leaves(self, other: "SuchTree") -> Tuple[list, np.ndarray, np.ndarray]:
        """(names, ids in self, ids in other) of every leaf name present in both trees, ordered by self's leaf id.
        An extension: the reference has no counterpart."""
        names = [name for name, _ in sorted(self.leaves.items(), key=lambda kv: kv[1]) if name in other.leaves]
        return names, self._name_ids(names), other._name_ids(names)

    def compare_distances(self, other: "SuchTree", leaves=None, pairs=None, bins=None, range=None, spearman=False,
                          kendall=False):
        """Compare this tree's distances with ``other``'s over the same pairs, reduced on the GPU.

        An extension: the reference has no counterpart.  It stands in for the comparison workflow of its docs
        (docs/examples/SuchTree_examples.md, "Comparing the topologies of two large trees": random name pairs,
        ``distances_by_name`` on both trees, then Pearson's r and a joint histogram on the host), but evaluates every
        pair on the GPU and returns only a :class:`~suchtree_amd.compare.DistanceComparison`: x = distances here,
        y = distances in ``other``.  The per-pair values are those of ``distances_bulk``.

        ``leaves`` (all pairs of a leaf list; exclusive with ``pairs``):
          * None: every leaf name present in both trees, ordered by this tree's leaf id (:meth:`shared_leaves`);
          * a list of leaf names, looked up in both trees;
          * a tuple ``(ids_self, ids_other)`` of aligned node-id arrays.
          Pair k = (leaf j, leaf i), k = i(i-1)/2 + j, j < i: the enumeration of ``linked_distances``.
        ``pairs``: a list of ``(name, name)`` tuples, looked up in each tree (unknown names raise as in
        ``distances_by_name``), or a tuple of two aligned (n, 2) node-id arrays.
        ``bins`` / ``range`` follow ``numpy.histogram2d`` (an int, two ints, or two edge arrays); ``bins=None`` skips the
        histogram.  ``range=None`` with integer bins takes numpy's default range, the data's (min, max) widened by 0.5
        where it is empty: that costs a second pass over all pairs (the first finds min and max).  That first pass
        ignores NaN distances (NaN-ignoring min and max), so the range is that of the other values; numpy raises on
        NaN data there instead.  An infinite distance makes the range infinite: ValueError, as in numpy.  The
        histogram leaves NaN and infinite distances out, as numpy does with a given range.
        ``spearman=True`` also ranks every pair on the GPU (two more passes over the pairs and 4 MiB of device counters
        per occupied key bucket, see DistanceComparison): ``spearman_r``, the exact integer rank sums and the distinct
        counts are filled in; at most 2^31 - 1 pairs (ValueError beyond).  Every other field is what it is without it.
        ``kendall=True`` also keeps every pair on the GPU as a 64-bit key, sorts them there and counts: ``kendall_tau``
        (tau-b, as ``scipy.stats.kendalltau``) and the exact integers ``concordant``, ``discordant``, ``ties_x``,
        ``ties_y``, ``ties_xy`` are filled in.  One pass over the pairs and 16 bytes of device memory per pair (all
        1.48e9 pairs of 54,327 leaves: 24 GB; MemoryError when the device cannot give them); at most 2^31 - 1 pairs.
        With ``bins`` or ``spearman=True`` those calls run as they do without it.  Every other field is what it is
        without it.
        Both trees must be on the same GPU (ValueError otherwise); an id out of range raises InvalidNodeError.
        """
        from . import compare
        if leaves is not None and pairs is not None:
            raise ValueError("leaves and pairs are mutually exclusive")
        # (names and ids are resolved before either tree is touched on the GPU)
        if pairs is not None:
            if isinstance(pairs, tuple) and len(pairs) == 2 and all(isinstance(p, np.ndarray) for p in pairs):
                px, py = (np.ascontiguousarray(p, dtype=np.int64) for p in pairs)
            else:
                if not isinstance(pairs, list):
                    raise TypeError("pairs must be a list of (name, name) tuples or a tuple of two (n, 2) id arrays")
                for i, p in enumerate(pairs):
                    if len(p) != 2 or not isinstance(p[0], str) or not isinstance(p[1], str):
                        raise TypeError("Pair {i}: both elements must be strings".format(i=str(i)))
                flat = [name for p in pairs for name in p]
                px = self._name_ids(flat).reshape(-1, 2)
                py = other._name_ids(flat).reshape(-1, 2)
            dx, dy = self._device_tree(), other._device_tree()
            return compare.run(dx, dy, "pairs", (px, py), bins, range, spearman=spearman, kendall=kendall)
        if leaves is None:
            _, ids_x, ids_y = self.shared_leaves(other)
        elif isinstance(leaves, tuple) and len(leaves) == 2:
            ids_x, ids_y = (np.ascontiguousarray(v, dtype=np.int64) for v in leaves)
        else:
            names = list(leaves)
            ids_x, ids_y = self._name_ids(names), other._name_ids(names)
        if ids_x.ndim != 1 or ids_x.shape != ids_y.shape:
            raise ValueError("the two id lists must be 1-D and of equal length")
        dx, dy = self._device_tree(), other._device_tree()
        return compare.run(dx, dy, "triangle", (ids_x, ids_y), bins, range, int(len(ids_x)), spearman, kendall)

    def compare_quartets(self, other: "SuchTree", leaves=None, quartets=None, samples=None, seed=None):
        """Compare this tree's topology with ``other``'s over the same quartets, counted on the GPU.

        An extension: the reference has no counterpart.  It stands in for two ``quartet_topologies_bulk`` calls
        (MuchTree.pyx:1271-1329) and a host-side comparison of their results: the quartets are generated on the GPU,
        classified in both trees and counted there, and only a :class:`~suchtree_amd.compare.QuartetComparison` -- a
        4 x 4 table of counts -- comes back.  A quartet's class in a tree is what ``quartet_topologies_bulk`` reports
        for it: which of b, c, d ends up beside a.

        ``leaves`` (as in :meth:`compare_distances`; exclusive with ``quartets``): None = every leaf name present in both
        trees, a list of leaf names, or a tuple ``(ids_self, ids_other)`` of aligned node-id arrays.
        ``samples=None`` compares all C(m,4) quartets of the m leaves (``distance`` is then the normalised quartet
        distance): at most 2^36 of them and at most 65536 leaves, ValueError beyond -- give ``samples=``.
        ``samples=n`` draws n quartets of distinct leaves, uniformly; quartet k depends on (seed, k, m) alone
        (:func:`~suchtree_amd.compare.quartet_positions` returns them).  ``seed=None`` takes a seed from
        ``numpy.random.default_rng()``; the result reports it.  Fewer than four leaves with ``samples > 0``: ValueError.
        ``quartets``: a list of 4-tuples of leaf names, looked up in each tree, or a tuple of two aligned (n, 4)
        node-id arrays (repeated ids and internal nodes are allowed: such rows may fall in class 3).
        Both trees must be on the same GPU (ValueError otherwise); an id out of range raises InvalidNodeError.
        """
        from . import compare
        if quartets is not None and (leaves is not None or samples is not None):
            raise ValueError("quartets is exclusive with leaves and samples")
        # (names and ids are resolved before either tree is touched on the GPU)
        if quartets is not None:
            if isinstance(quartets, tuple) and len(quartets) == 2 and all(isinstance(q, np.ndarray) for q in quartets):
                qx, qy = (np.ascontiguousarray(q, dtype=np.int64) for q in quartets)
            else:
                if not isinstance(quartets, list):
                    raise TypeError("quartets must be a list of 4-tuples of names or a tuple of two (n, 4) id arrays")
                for i, q in enumerate(quartets):
                    if len(q) != 4 or not all(isinstance(name, str) for name in q):
                        raise TypeError("Quartet {i}: all four elements must be strings".format(i=str(i)))
                flat = [name for q in quartets for name in q]
                qx = self._name_ids(flat).reshape(-1, 4)
                qy = other._name_ids(flat).reshape(-1, 4)
            table = self._device_tree().compare_quartets_host(other._device_tree(), qx, qy)
            return compare.QuartetComparison.from_table(table, mode="given")
        if leaves is None:
            _, ids_x, ids_y = self.shared_leaves(other)
        elif isinstance(leaves, tuple) and len(leaves) == 2:
            ids_x, ids_y = (np.ascontiguousarray(v, dtype=np.int64) for v in leaves)
        else:
            names = list(leaves)
            ids_x, ids_y = self._name_ids(names), other._name_ids(names)
        if ids_x.ndim != 1 or ids_x.shape != ids_y.shape:
            raise ValueError("the two id lists must be 1-D and of equal length")
        m = int(len(ids_x))
        if samples is None:
            total = math.comb(m, 4)
            if m > _capi.QUARTET_MAX_LEAVES_ALL or total > compare.QUARTET_MAX_ALL:
                raise ValueError("all quartets of %d leaves are %d, more than 2^36: draw a sample with samples=" % (m, total))
            mode, count, seed = "all", total, None
        else:
            count = int(samples)
            if count < 0:
                raise ValueError("samples must not be negative")
            if m < 4 and count > 0:
                raise ValueError("a quartet needs four leaves, the list has %d" % m)
            if seed is None:
                seed = int(np.random.default_rng().integers(0, 1 << 63))
            mode, seed = "sample", int(seed)
        table = self._device_tree().compare_quartets_leaves_host(other._device_tree(), ids_x, ids_y, mode=mode, seed=seed or 0,
                                                                 k_count=count)
        return compare.QuartetComparison.from_table(table, n_leaves=m, mode=mode, seed=seed)

    def _shared_ids(self, other, leaves):
        """(ids in self, ids in other) of a ``leaves`` argument as :meth:`compare_distances` reads it."""
        if leaves is None:
            _, ids_x, ids_y = self.shared_leaves(other)
        elif isinstance(leaves, tuple) and len(leaves) == 2:
            ids_x, ids_y = (np.ascontiguousarray(v, dtype=np.int64) for v in leaves)
        else:
            names = list(leaves)
            ids_x, ids_y = self._name_ids(names), other._name_ids(names)
        if ids_x.ndim != 1 or ids_x.shape != ids_y.shape:
            raise ValueError("the two id lists must be 1-D and of equal length")
        return ids_x, ids_y

    def compare_clades(self, other: "SuchTree", leaves=None, rooted=False, nodes=None, min_branch=None, device=..., chunk_rows=0):
        """Which clades of this tree are also in ``other``, and how close is the best match where they are not: every
        induced clade of this tree (A) against every induced clade of ``other`` (B), matched on the GPU.

        An extension: the reference offers only ``bipartitions()``, a generator of Python sets (MuchTree.pyx:1151-1200).
        Returns a :class:`~suchtree_amd.compare.CladeMatches`: per clade of A the closest clade of B, the leaves to move
        between them (``distance``), the transfer distance and support of Lemoine et al. 2018, and over all clades the
        Robinson-Foulds distance ``rf``.

        ``leaves`` as in :meth:`compare_distances`: None = every leaf name present in both trees, a list of leaf names,
        or a tuple ``(ids_self, ids_other)`` of aligned leaf-id arrays; 4 to 262144 leaves, each once (ValueError).  Other
        leaves collapse away: a clade is a node that is the MRCA of two or more listed leaves, taken as the set of
        listed leaves under it.  ``rooted=False`` (the default: most such trees are arbitrarily rooted) reads clades as
        bipartitions -- a set and its complement are the same, clades of m - 1 leaves are left out and the root's two
        children count once; ``rooted=True`` compares the sets themselves, up to m - 1 leaves.
        ``nodes=`` restricts the rows to the listed clades of this tree; the candidates and ``rf`` still use all of them.
        ``min_branch=x`` leaves out of both lists every clade whose branch -- the path from its node up to the next node
        that joins more listed leaves, summed in float64 -- is x or shorter: ``min_branch=tree.polytomy_epsilon`` keeps the
        epsilon branches that resolve a polytomy from counting as clades.
        ``device``: by default the tree's device; None runs the host restatement (one thread, no GPU): the same integers.
        Neither tree is uploaded: the call needs their parent arrays alone.
        """
        from . import compare
        ids_x, ids_y = self._shared_ids(other, leaves)
        return compare.match_clades(self._flat, ids_x, other._flat, ids_y, bool(rooted), nodes, min_branch,
                                    self._device if device is ... else device, int_arg("chunk_rows", chunk_rows))

    def transfer_support(self, replicates, leaves=None, rooted=False, min_branch=None, device=...):
        """The transfer bootstrap expectation (Lemoine et al. 2018) of every clade of this tree over replicate trees, the
        support measure made for trees of 10^4 to 10^5 leaves, with Felsenstein's count beside it.

        ``replicates`` is an iterable of :class:`SuchTree` objects, Newick texts or paths to Newick files; texts and paths
        are parsed into flat arrays only, nothing of a replicate goes to the GPU but its clade ranges.  ``leaves``: None =
        every leaf of this tree, else a collection of leaf names; a replicate that lacks one is a ValueError that names
        it.  ``rooted``, ``min_branch`` and ``device`` as in :meth:`compare_clades`, which is what every replicate gets:
        replicate r's contribution depends on (this tree, replicate r, the leaf list) alone.  Returns a
        :class:`~suchtree_amd.compare.TransferSupport`.  An extension: the reference has no counterpart.
        """
        from . import compare
        names = [name for name, _ in sorted(self.leaves.items(), key=lambda kv: kv[1])] if leaves is None else list(leaves)
        ids = self._name_ids(names)
        device = self._device if device is ... else device
        if len(ids) < 4:
            raise ValueError("%d listed leaves: at least 4" % len(ids))
        side = compare.clade_side(self._flat, ids, bool(rooted), min_branch)
        out = compare.TransferSupport(len(ids), bool(rooted), side)
        for r, rep in enumerate(replicates):
            flat = compare.read_flat_tree(rep)
            if flat is None:
                raise TypeError("replicate %d must be a SuchTree, a Newick text or a path" % r)
            where = flat.leaves
            for name in names:
                if name not in where:
                    raise ValueError("replicate %d has no leaf %r" % (r, name))
            ids_r = np.fromiter((where[name] for name in names), dtype=np.int64, count=len(names))
            out.add(compare.match_clades(self._flat, ids, flat, ids_r, bool(rooted), None, min_branch, device, side_a=side))
        return out

    _DISPERSION_GROUP_ROWS = 1 << 22      # records per library call of dispersion: bounds its host memory (16 bytes each)

    def _depth_first_leaves(self) -> np.ndarray:
        """The leaf ids in depth-first order, children in increasing id order (st_clade_plan over one link per leaf)."""
        leaf_ids = np.flatnonzero(np.asarray(self._flat.left) == -1).astype(np.int64)
        return leaf_ids[_capi.clade_plan(self._flat.parent, leaf_ids)["perm"]]

    def _leaf_ids(self, leaves, what) -> np.ndarray:
        """Leaf ids of a collection of leaf names or leaf ids (ValueError for an id that is no leaf)."""
        left = self._flat.left
        if isinstance(leaves, np.ndarray) and leaves.dtype.kind in "iu":      # an id array: checked at once
            ids = leaves.astype(np.int64).ravel()
            ok = (ids >= 0) & (ids < self.size)
            ok[ok] = np.asarray(left)[ids[ok]] == -1
            if not ok.all():
                raise ValueError("%s: %r is not a leaf of this tree" % (what, int(ids[~ok][0])))
            return ids
        leaves = list(leaves)
        out = np.empty(len(leaves), dtype=np.int64)
        for i, v in enumerate(leaves):
            if isinstance(v, str):
                if v not in self.leaves:
                    raise NodeNotFoundError(v)
                out[i] = self.leaves[v]
            else:
                if isinstance(v, bool) or not isinstance(v, Integral) or not 0 <= v < self.size or left[int(v)] != -1:
                    raise ValueError("%s: %r is not a leaf of this tree" % (what, v))
                out[i] = int(v)
        return out

    def _position_table(self, univ, rows):
        """(set_pos int32, offsets int64): every set of ``rows`` (leaf ids, all of them in ``univ``) as increasing positions
        of ``univ``, one set behind the other; set r is set_pos[offsets[r]:offsets[r + 1]]."""
        where = np.full(self.size, -1, dtype=np.int64)
        where[univ] = np.arange(len(univ))
        pos = [np.sort(where[ids]).astype(np.int32) for ids in rows]
        offsets = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(np.array([len(p) for p in pos], dtype=np.int64), out=offsets[1:])
        return (np.concatenate(pos) if pos else np.empty(0, dtype=np.int32)), offsets

    def _universe_and_sets(self, sets, universe):
        """What dispersion and beta_dispersion share: (the universe's leaf ids depth-first, every set's leaf ids), with their
        ValueErrors -- a universe outside 3 .. 16384 leaves, a member outside it, a repeated member."""
        univ = self._depth_first_leaves()
        if universe is not None:
            inside = np.zeros(self.size, dtype=bool)
            inside[self._leaf_ids(universe, "universe")] = True
            univ = univ[inside[univ]]
        limit = _capi.HOMMOLA_MAX_UNIVERSE
        if len(univ) < 3:
            raise ValueError("the universe has %d leaves: at least 3" % len(univ))
        if len(univ) > limit:
            raise ValueError("the universe has %d leaves: at most %d (subset it first)" % (len(univ), limit))
        inside = np.zeros(self.size, dtype=bool)
        inside[univ] = True
        rows = []
        for r, members in enumerate(sets):
            ids = self._leaf_ids(members, "set %d" % r)
            if not inside[ids].all():
                raise ValueError("set %d: a member outside the universe" % r)
            if len(np.unique(ids)) != len(ids):
                raise ValueError("set %d: a repeated member" % r)
            rows.append(ids)
        return univ, rows

    def dispersion(self, sets, universe=None, permutations=999, seed=None, stream=0, keep_null=False, chunk_tasks=0, null="taxa.labels",
                   iterations=None, _report=None):
        """How closely related are the members of each set of leaves: MPD and MNTD with a permutation null, on the GPU.

        ``sets`` is an iterable of collections of leaf names or leaf ids.  For each, ``mpd`` is the mean pairwise distance
        among its members and ``mntd`` the mean distance from a member to its nearest other member, in float64 over the
        float32 distances of ``distances_bulk``.  Both are standardised against the null that shuffles the leaf labels of
        ``universe`` (a collection of leaves; None = all leaves of the tree; 3 to 16384 leaves), picante's ``ses.mpd`` /
        ``ses.mntd`` with ``null.model = "taxa.labels"``: NRI = -``mpd_ses``, NTI = -``mntd_ses``.  One shuffle serves
        every set of the call: a set's null draws are uniform k-subsets of the universe, and the sets share the
        shuffles.  Every member must be in the universe; a repeated member is a ValueError.

        The universe's distances are computed once, as a matrix on the GPU, and every (set, permutation) is reduced
        there.  Shuffle p >= 1 is ``compare.hommola_permutation(seed, stream, p, 0, n)`` over the universe in depth-first
        order (children in increasing id order); a set's columns depend on (seed, ``stream``, the universe, the set)
        alone -- not on the other sets or ``chunk_tasks`` -- and null column p is the same for any ``permutations`` >= p.
        ``seed=None`` draws a seed and reports it.  ``keep_null=True`` keeps the (sets, permutations) null draws.

        ``null="swap"`` standardises against the degree-preserving swap null instead (picante's ``independentswap`` /
        ``trialswap``, the fixed-fixed null of bipartite networks): the sets are the rows of a 0/1 matrix over the
        universe, and null draw p is that matrix after a chain of ``iterations`` trial swaps
        (:func:`~suchtree_amd.compare.swap_null_tables`), which keeps every set's size *and* the number of sets each leaf
        belongs to.  A clustered set that is only the signature of a few widespread leaves is not significant under it.
        ``iterations=None`` is max(1000, 10 x the links of the matrix) trials, the library's own default (picante's is
        1000 swaps); with the default null it must stay None.  All sets of the call form one matrix, so a set's null
        columns depend on the other sets; they do not depend on ``chunk_tasks``, and column p is the same for any
        ``permutations`` >= p.  ``swap_accepted`` of the result holds the swaps each chain made.

        Returns a :class:`~suchtree_amd.compare.SetDispersion`.  An extension: the reference has no counterpart.
        """
        from . import compare
        null, iterations = null_model_arg(null, iterations)
        permutations, seed, stream, chunk_tasks = _null_args(permutations, seed, stream, chunk_tasks)
        univ, rows = self._universe_and_sets(sets, universe)
        set_pos, offsets = self._position_table(univ, rows)
        k = np.diff(offsets)
        if null == "swap":      # one matrix, one call: the chains run over every row, `_report` (partner_dispersion) picks the rows kept
            keep = np.arange(len(rows)) if _report is None else np.asarray(_report, dtype=np.int64)
            iterations = _capi.swap_iterations(iterations, len(set_pos))
            out = compare.SetDispersion(len(keep), permutations, seed, len(univ), keep_null, null, iterations)
            if len(keep):      # (no row to report: nothing is launched, and the tree stays where it is)
                rec, out.swap_accepted = self._device_tree().partner_dispersion_swap_host(univ, (set_pos, offsets), permutations, seed, iterations,
                                                                                         stream, chunk_tasks)
                out.fill(0, k[keep], rec[keep])
            return out
        out = compare.SetDispersion(len(rows), permutations, seed, len(univ), keep_null)
        per_group = max(1, self._DISPERSION_GROUP_ROWS // (permutations + 1))
        for at in range(0, len(rows), per_group):      # (no sets: nothing is launched, and the tree stays where it is)
            end = min(at + per_group, len(rows))
            part = (set_pos[offsets[at]:offsets[end]], offsets[at:end + 1] - offsets[at])
            rec = self._device_tree().partner_dispersion_host(univ, part, permutations, seed, stream, chunk_tasks)
            out.fill(at, k[at:end], rec)      # (each group is reduced before the next)
        return out

    def beta_dispersion(self, sets, universe=None, begin=0, count=None, exclude_shared=False, permutations=999, seed=None, stream=0,
                        keep_null=False, chunk_tasks=0):
        """How far apart are the members of every two sets of leaves: betaMPD and betaMNTD with a permutation null, on the GPU.

        ``sets`` and ``universe`` are those of :meth:`dispersion`, with the same checks; sets of no or one member are
        allowed.  For a pair of sets, ``beta_mpd`` is the mean distance between a member of one and a member of the other
        and ``beta_mntd`` the mean, over the members of both, of the distance to the nearest member of the other set
        (picante's ``comdist`` / ``comdistnt``, unweighted), in float64 over the float32 distances of ``distances_bulk``;
        ``exclude_shared=True`` does not compare a member with itself in the other set (``exclude.conspecifics``).  Both
        are standardised against the null of :meth:`dispersion`, which shuffles the universe's leaf labels: betaNRI is
        ``beta_mpd_ses``, betaNTI ``beta_mntd_ses``.

        The pairs are ``[begin, begin + count)`` of the triangle k = i (i - 1) / 2 + j, j < i; ``count=None`` means the
        whole triangle, which above 2^31 pairs is a ValueError: ask for ranges.  The shuffles, ``seed``, ``stream``,
        ``keep_null`` and ``chunk_tasks`` are those of :meth:`dispersion`: a pair's columns depend on (seed, ``stream``, the
        universe, its two sets, ``exclude_shared``) alone.  Returns a :class:`~suchtree_amd.compare.SetBetaDispersion`.  An
        extension: the reference has no counterpart.
        """
        from . import compare
        permutations, seed, stream, chunk_tasks = _null_args(permutations, seed, stream, chunk_tasks)
        begin, count = int_arg("begin", begin), int_arg("count", count, optional=True)
        univ, rows = self._universe_and_sets(sets, universe)
        begin, count = _triangle_range(len(rows), begin, count)
        set_pos, offsets = self._position_table(univ, rows)
        k = np.diff(offsets)
        out = compare.SetBetaDispersion(len(rows), begin, count, permutations, seed, len(univ), exclude_shared, keep_null)
        per_group = max(1, self._DISPERSION_GROUP_ROWS // (2 * (permutations + 1)))
        bits = compare.set_bit_rows(set_pos, offsets, len(univ)) if count else None
        for at in range(0, count, per_group):      # (no pairs: nothing is launched, and the tree stays where it is)
            n = min(per_group, count - at)
            rec = self._device_tree().beta_dispersion_host(univ, (set_pos, offsets), begin + at, n, exclude_shared, permutations, seed, stream,
                                                           chunk_tasks)
            i, j = compare.SetUniFrac._rows(begin + at + np.arange(n, dtype=np.int64))
            out.fill(at, k[i], k[j], compare.shared_counts(bits, i, j), rec)      # (each group is reduced before the next)
        return out

    def mantel(self, y, leaves, z=None, method="pearson", permutations=999, seed=None, alternative="two-sided", stream=0, keep_stats=False,
               chunk_tasks=0):
        """The Mantel test of this tree's distances against another distance matrix over the same objects, on the GPU.

        ``leaves`` (leaf names or leaf ids, at least 3, at most 16384, none repeated) are the objects in the order of
        ``y``'s rows; x is the tree's own distance matrix over them (:meth:`pairwise_distances`), and it is x that the
        permutations relabel.  ``y``, ``z`` (the partial test given a third matrix) and every other argument are those of
        :func:`~suchtree_amd.compare.mantel`, which does the work on this tree's device.  Returns a
        :class:`~suchtree_amd.compare.MantelResult`.  An extension: the reference has no counterpart.
        """
        from . import compare
        ids = self._leaf_ids(leaves, "leaves")
        if len(np.unique(ids)) != len(ids):
            raise ValueError("leaves: a repeated leaf")
        if len(ids) < 3 or len(ids) > _capi.HOMMOLA_MAX_UNIVERSE:
            raise ValueError("%d leaves: 3 to %d" % (len(ids), _capi.HOMMOLA_MAX_UNIVERSE))
        for name, a in (("y", y), ("z", z)):      # (before the tree goes to its device)
            if a is not None and compare.mantel_condensed(a, name)[1] != len(ids):
                raise ValueError("%s is not over the %d leaves" % (name, len(ids)))
        return compare.mantel(self.pairwise_distances(ids.tolist()), y, z, method=method, permutations=permutations, seed=seed, alternative=alternative,
                              stream=stream, keep_stats=keep_stats, device=self._device, chunk_tasks=chunk_tasks)

    def mantel_correlogram(self, y, leaves, n_classes=None, breaks=None, cutoff=True, method="pearson", permutations=999, seed=None, stream=0,
                           correction="holm", progressive=True, keep_stats=False, device=..., chunk_tasks=0):
        """The Mantel correlogram of another distance matrix over the classes of this tree's distances, on the GPU: at
        which depths of the tree are the objects' y values alike.

        ``leaves`` (leaf names or leaf ids, at least 3, at most 16384, none repeated) are the objects in the order of
        ``y``'s rows; x is the tree's own distance matrix over them (:meth:`pairwise_distances`), as in :meth:`mantel`,
        and its classes are what the permutations relabel.  Every other argument is that of
        :func:`~suchtree_amd.compare.mantel_correlogram`, which does the work on ``device`` (... = this tree's device;
        None = only the permutations run on the host: x still comes from the tree's kernels).  Returns a
        :class:`~suchtree_amd.compare.MantelCorrelogram` with ``leaves`` (leaf ids) and ``names``.  An extension: the
        reference has no counterpart.
        """
        from . import compare
        ids = self._leaf_ids(leaves, "leaves")
        if len(np.unique(ids)) != len(ids):
            raise ValueError("leaves: a repeated leaf")
        if len(ids) < 3 or len(ids) > _capi.HOMMOLA_MAX_UNIVERSE:
            raise ValueError("%d leaves: 3 to %d" % (len(ids), _capi.HOMMOLA_MAX_UNIVERSE))
        if compare.mantel_condensed(y, "y")[1] != len(ids):      # (before the tree goes to its device)
            raise ValueError("y is not over the %d leaves" % len(ids))
        out = compare.mantel_correlogram(self.pairwise_distances(ids.tolist()), y, n_classes=n_classes, breaks=breaks, cutoff=cutoff, method=method,
                                         permutations=permutations, seed=seed, stream=stream, correction=correction, progressive=progressive,
                                         keep_stats=keep_stats, device=self._device if device is ... else device, chunk_tasks=chunk_tasks)
        out.leaves, out.names = ids.copy(), [self.leaf_nodes[int(v)] for v in ids.tolist()]
        return out

    def dendrogram_congruence(self, y, leaves, linkage="average", rooted=True, min_branch=None, permutations=999, seed=None, stream=0,
                              keep_stats=False, device=...):
        """Does the dendrogram of another distance matrix over the same objects share this tree's topology?  The
        topology test of phylosymbiosis (Brooks et al. 2016): ``y`` is clustered exactly (UPGMA by default) and the
        dendrogram is matched against this tree by Robinson-Foulds and the transfer distance, against relabellings of
        the dendrogram's objects.

        ``leaves`` (leaf names or leaf ids, 4 to 16384, none repeated) are the objects in the order of ``y``'s rows.
        ``y`` (square symmetric or condensed in the triangle order; or a :class:`~suchtree_amd.compare.Dendrogram`),
        ``linkage``, ``rooted``, ``min_branch``, ``permutations``, ``seed``, ``stream`` and ``keep_stats`` are those of
        :func:`~suchtree_amd.compare.dendrogram_congruence`, which does the work: ``device`` ... = the clade matches on
        this tree's device and the linkage where :func:`~suchtree_amd.compare.linkage` puts it by n; None = all of it
        on the host, without a GPU; an index = all of it there.  The same integers either way: the tree is not
        uploaded, the call needs its parent array and branch lengths alone.  Returns a
        :class:`~suchtree_amd.compare.TopologyTestResult` with ``leaves`` (leaf ids) and ``names``.  An extension: the
        reference has no counterpart.
        """
        from . import compare
        ids = self._leaf_ids(leaves, "leaves")
        if len(np.unique(ids)) != len(ids):
            raise ValueError("leaves: a repeated leaf")
        out = compare.dendrogram_congruence(self._flat, ids, y, linkage=linkage, rooted=rooted, min_branch=min_branch, permutations=permutations,
                                            seed=seed, stream=stream, keep_stats=keep_stats, device=device, match_device=self._device)
        out.leaves, out.names = ids.copy(), [self.leaf_nodes[int(v)] for v in ids.tolist()]
        return out

    def unifrac(self, sets, root=None, begin=0, count=None, shift=None, chunk_pairs=0):
        """How different are every two sets of leaves, measured on this tree: Faith's PD and unweighted UniFrac, on the GPU.

        ``sets`` is an iterable of collections of leaf names or leaf ids; a repeated member is a ValueError, and every
        member must lie under ``root`` (a node id; None = the tree's root).  PD of a set is the branch length that joins
        ``root`` to its members; for a pair of sets the call also sums the branch length of their union, from which
        ``shared``, ``unifrac`` and ``phylosor`` follow (:class:`~suchtree_amd.compare.SetUniFrac`).  The universe is the
        union of all members in depth-first order (up to 2^20 leaves): no distance matrix is built.

        The pairs are ``[begin, begin + count)`` of the triangle k = i (i - 1) / 2 + j, j < i; ``count=None`` means the
        whole triangle, which above 2^31 pairs is a ValueError: ask for ranges.  The sums are exact integers over depths
        quantised to 2^-``shift`` (None = chosen from the largest depth): a row's ``pd_q`` and a pair's ``union_q`` depend
        on (root, the sets, shift) alone, so pass ``shift=`` to keep several calls on one scale.  ``shift=`` takes 0 to
        256: on a tree with a depth of 2^40 or more the automatic shift is negative and cannot be passed back; calls over
        the same sets and root choose the same automatic shift there.  An extension: the
        reference has no counterpart.
        """
        from . import compare
        begin, count = int_arg("begin", begin), int_arg("count", count, optional=True)
        shift, chunk_pairs = int_arg("shift", shift, optional=True), int_arg("chunk_pairs", chunk_pairs)
        root = self.root_node if root is None else self._validate_node(root)
        leaf_ids = np.flatnonzero(np.asarray(self._flat.left) == -1).astype(np.int64)
        plan = _capi.clade_plan(self._flat.parent, leaf_ids)      # (one link per leaf: _depth_first_leaves, and every node's range of it)
        order = leaf_ids[plan["perm"]]
        rows, member = [], np.zeros(self.size, dtype=bool)
        for r, members in enumerate(sets):
            ids = self._leaf_ids(members, "set %d" % r)
            if len(np.unique(ids)) != len(ids):
                raise ValueError("set %d: a repeated member" % r)
            rows.append(ids)
            member[ids] = True
        univ = order[member[order]]
        inside = np.zeros(self.size, dtype=bool)      # the leaves under root are one range of the depth-first order
        inside[order[int(plan["begin"][root]):int(plan["begin"][root]) + int(plan["count"][root])]] = True
        if not inside[univ].all():
            raise ValueError("leaf %d does not lie under node %d" % (int(univ[~inside[univ]][0]), root))
        if len(univ) > _capi.UNIFRAC_MAX_UNIVERSE:
            raise ValueError("the sets hold %d distinct leaves: at most %d" % (len(univ), _capi.UNIFRAC_MAX_UNIVERSE))
        begin, count = _triangle_range(len(rows), begin, count)
        if not len(univ):      # (no member at all: nothing is launched, and the tree stays where it is)
            out = compare.SetUniFrac(len(rows), begin, shift or 0, np.zeros(len(rows), dtype=np.int64), np.zeros(count, dtype=np.int64), root)
        else:
            pd_q, union_q, used, _, _ = self._device_tree().unifrac_host(root, univ, self._position_table(univ, rows), begin, count, shift,
                                                                         chunk_pairs)
            out = compare.SetUniFrac(len(rows), begin, used, pd_q, union_q, root)
        return out

    def unifrac_null(self, sets, universe=None, root=None, begin=0, count=None, shift=None, permutations=999, seed=None, stream=0,
                     keep_null=False, chunk_tasks=0):
        """Faith's PD of every set of leaves and the UniFrac and PhyloSor of every two, standardised against a permutation
        null, on the GPU: picante's ``ses.pd`` and the label-shuffling significance of UniFrac.

        ``sets`` and the sums are those of :meth:`unifrac`; the null is that of :meth:`dispersion`.  The universe is the
        leaves under ``root`` (a node id; None = the tree's root), restricted to ``universe`` where given (a collection of
        leaves), 3 to 16384 leaves in depth-first order; every member must be in it and a repeated member is a ValueError.
        Shuffle p >= 1 is ``compare.hommola_permutation(seed, stream, p, 0, n)`` over the universe: set r becomes the
        images of its members, and its PD and every pair's union sum are taken again, as exact integers over the depths
        quantised to 2^-``shift`` (None = chosen from the largest depth of the universe).  One shuffle serves every set
        of the call.  A set's and a pair's columns depend on (seed, ``stream``, root, the universe, shift, the one or
        two sets) alone -- not on the other sets, the range or ``chunk_tasks`` -- and null column p is the same for any
        ``permutations`` >= p; the observed values are those of :meth:`unifrac` at the same ``shift``.

        The pairs are ``[begin, begin + count)`` of the triangle, as in :meth:`unifrac`.  ``seed=None`` draws a seed and
        reports it; ``keep_null=True`` keeps the draws.  Returns a :class:`~suchtree_amd.compare.SetUniFracNull`.  An
        extension: the reference has no counterpart.
        """
        from . import compare
        permutations, seed, stream, chunk_tasks = _null_args(permutations, seed, stream, chunk_tasks)
        begin, count = int_arg("begin", begin), int_arg("count", count, optional=True)
        shift = int_arg("shift", shift, optional=True)
        root = self.root_node if root is None else self._validate_node(root)
        if root != self.root_node:      # the leaves under root are one range of the depth-first order
            leaf_ids = np.flatnonzero(np.asarray(self._flat.left) == -1).astype(np.int64)
            plan = _capi.clade_plan(self._flat.parent, leaf_ids)
            under = leaf_ids[plan["perm"]][int(plan["begin"][root]):int(plan["begin"][root]) + int(plan["count"][root])]
            if universe is not None:
                inside = np.zeros(self.size, dtype=bool)
                inside[self._leaf_ids(universe, "universe")] = True
                under = under[inside[under]]
            universe = under
        univ, rows = self._universe_and_sets(sets, universe)
        begin, count = _triangle_range(len(rows), begin, count)
        table = self._position_table(univ, rows)
        if not rows:      # (no sets: nothing is launched, and the tree stays where it is)
            return compare.SetUniFracNull(0, begin, count, shift or 0, permutations, seed, len(univ), keep_null, root)
        # PD of every set first (it fixes the shift), then the pairs a group at a time: a group's int64 block is bounded
        pd_q, _, used = self._device_tree().unifrac_null_host(root, univ, table, 0, 0, shift, permutations, seed, stream, chunk_tasks, union=False)
        out = compare.SetUniFracNull(len(rows), begin, count, used, permutations, seed, len(univ), keep_null, root)
        out.fill_sets(np.diff(table[1]), pd_q)
        shift = used if used >= 0 else None      # (a negative automatic shift cannot be passed: it is chosen again, the same)
        per_group = max(1, 2 * self._DISPERSION_GROUP_ROWS // (permutations + 1))
        for at in range(0, count, per_group):
            n = min(per_group, count - at)
            _, union_q, _ = self._device_tree().unifrac_null_host(root, univ, table, begin + at, n, shift, permutations, seed, stream,
                                                                  chunk_tasks, pd=False)
            out.fill_pairs(at, union_q)      # (each group is reduced before the next)
        return out

    def common_ancestor(self, a: Union[int, str], b: Union[int, str]) -> int:
        """Most recent common ancestor of two nodes (MuchTree.pyx:1128-1149)."""
        node_a, node_b = self._validate_node_pair(a, b)
        pairs = np.array([[node_a, node_b]], dtype=np.int64)
        _, mrca = self._device_tree().distances_host(pairs, want_dist=False, want_mrca=True)
        return int(mrca[0])

    # ------------------------------------------- callers of the path (all-pairs, kNN)
    def _node_ids(self, nodes) -> np.ndarray:
        if nodes is None:
            return self.leaf_node_ids
        return np.array([self._validate_node(node) for node in nodes])

    def pairwise_distances(self, nodes: List[Union[int, str]] = None) -> np.ndarray:
        """Symmetric matrix of all pairwise distances (MuchTree.pyx:1084-1124).

        The reference materialises the n(n-1)/2 pairs as a Python list, calls
        ``distances_bulk`` and scatters the result into the matrix in a Python loop.  Here the
        whole (n, n) matrix is generated on the device (``st_grid_host``, symmetric grid) and
        streamed straight into the result array: entry [i, j] with i < j is d(ids[i], ids[j])
        in that argument order, exactly as the reference computes it, entry [j, i] is the same
        value, the diagonal is d(x, x) = 0.
        """
        node_ids = self._node_ids(nodes)
        n = len(node_ids)
        distance_matrix = np.zeros((n, n), dtype=float)
        if n > 1:
            ids = np.asarray(node_ids, dtype=np.int64)
            self._device_tree().grid_host(ids, ids, symmetric=True, out_dist=distance_matrix.reshape(-1))
        return distance_matrix

    def distance_matrix(self, nodes: list = None) -> dict:
        """MuchTree.pyx:1919-1956."""
        if nodes is None:
            node_ids = self.leaf_node_ids
            node_names = [self.leaf_nodes[nid] for nid in node_ids]
        else:
            node_ids = np.array([self._validate_node(node) for node in nodes])
            node_names = [self.leaf_nodes[int(i)] if self.is_leaf(int(i)) else f"node_{i}" for i in node_ids]
        return {"distance_matrix": self.pairwise_distances(nodes), "node_ids": node_ids,
                "node_names": node_names}

    def nearest_neighbors(self, node: Union[int, str], k: int = 1, from_nodes: list = None) -> list:
        """k nearest neighbours of a node (MuchTree.pyx:1032-1082)."""
        if k <= 0:
            raise ValueError("k must be positive")
        query_node_id = self._validate_node(node)
        if from_nodes is None:
            if self.is_leaf(query_node_id):
                from_node_ids = [nid for nid in self.leaf_node_ids if nid != query_node_id]
            else:
                from_node_ids = self.leaf_node_ids
            from_nodes_orig = [self.leaf_nodes[nid] for nid in from_node_ids]
        else:
            from_node_ids = [self._validate_node(n) for n in from_nodes]
            from_nodes_orig = from_nodes.copy()
        if len(from_node_ids) == 0:
            # the reference hands np.array([], dtype=int64) to distances_bulk here, whose shape check
            # raises (pyx:1072, 892-894): same call, same exception
            self.distances_bulk(np.array([], dtype=np.int64))
        cands = np.asarray(from_node_ids, dtype=np.int64)
        dev = self._device_tree()
        if k <= dev.KNN_MAX_K:
            # distances and the selection of the k smallest both happen on the GPU (st_knn_host);
            # ties go to the candidate listed first (the reference's argsort leaves them unspecified)
            idx, dist = dev.knn_host(np.array([query_node_id], dtype=np.int64), cands, k)
            return [(from_nodes_orig[int(i)], d) for i, d in zip(idx[0], dist[0]) if i >= 0]
        distances, _ = dev.grid_host(np.array([query_node_id], dtype=np.int64), cands)
        sorted_indices = np.argsort(distances, kind="stable")
        return [(from_nodes_orig[i], distances[i]) for i in sorted_indices[:k]]

    def nearest_neighbors_bulk(self, nodes, k: int = 1, from_nodes: list = None):
        """``nearest_neighbors`` for many query nodes in one call (no reference counterpart):
        returns ``(neighbor_ids int64 (q, k), distances float64 (q, k))``, neighbours ascending
        by distance, -1 / NaN where a query has fewer than k candidates.  With the default
        candidate set (all leaves) a leaf query is not its own neighbour, as in
        ``nearest_neighbors`` (MuchTree.pyx:1058-1062)."""
        if k <= 0:
            raise ValueError("k must be positive")
        queries = np.array([self._validate_node(n) for n in nodes], dtype=np.int64)
        if from_nodes is None:
            cands, skip_self = np.asarray(self.leaf_node_ids, dtype=np.int64), True
        else:
            cands, skip_self = np.array([self._validate_node(n) for n in from_nodes], dtype=np.int64), False
        dev = self._device_tree()
        if k > dev.KNN_MAX_K:
            raise ValueError("k must be at most %d" % dev.KNN_MAX_K)
        idx, dist = dev.knn_host(queries, cands, k, skip_self=skip_self)
        ids = np.where(idx >= 0, cands[np.maximum(idx, 0)], -1) if len(cands) else idx
        return ids, dist

    # --------------------------------------------------- quartet topologies (MRCA caller)
    def quartet_topologies_bulk(self, quartets) -> np.ndarray:
        """(n, 4) node ids re-ordered so columns (0,1) and (2,3) are sisters (MuchTree.pyx:1271-1376)."""
        if not isinstance(quartets, np.ndarray):
            quartets = np.array(quartets, dtype=np.int64)
        if quartets.ndim != 2 or quartets.shape[1] != 4:
            raise ValueError(f"Expected (n, 4) array, got shape {quartets.shape}")
        if quartets.dtype != np.int64:
            if not np.issubdtype(quartets.dtype, np.integer):
                raise ValueError("Buffer dtype mismatch, expected 'long' but got '%s'" % quartets.dtype.name)
            quartets = quartets.astype(np.int64)
        if quartets.shape[0] == 0:
            quartets.max()
        return self._device_tree().quartets_host(quartets)

    def quartet_topology(self, a, b, c, d) -> frozenset:
        """Topology of one quartet as a frozenset of two sister-pair frozensets (MuchTree.pyx:1202-1248)."""
        nodes = [a, b, c, d]
        node_ids = [self._validate_node(node) for node in nodes]
        has_strings = any(isinstance(node, str) for node in nodes)
        w, x, y, z = (int(v) for v in self.quartet_topologies_bulk(np.array([node_ids], dtype=np.int64))[0])
        if has_strings:
            ln = self.leaf_nodes
            return frozenset((frozenset((ln[w], ln[x])), frozenset((ln[y], ln[z]))))
        return frozenset((frozenset((w, x)), frozenset((y, z))))

    def quartet_topologies_by_name(self, quartets) -> list:
        """MuchTree.pyx:1378-1422."""
        quartet_ids = []
        for i, (a, b, c, d) in enumerate(quartets):
            if not all(isinstance(name, str) for name in (a, b, c, d)):
                raise TypeError(f"Quartet {i}: all elements must be strings")
            try:
                quartet_ids.append([self.leaves[a], self.leaves[b], self.leaves[c], self.leaves[d]])
            except KeyError as e:
                raise NodeNotFoundError(str(e).strip("'"))
        topologies = self.quartet_topologies_bulk(np.array(quartet_ids, dtype=np.int64))
        ln = self.leaf_nodes
        return [frozenset((frozenset((ln[a], ln[b])), frozenset((ln[c], ln[d]))))
                for a, b, c, d in topologies.tolist()]

    # deprecated wrappers (MuchTree.pyx:2447-2459)
    def distances(self, pairs):
        _deprecation_warning("distances()", "distances_bulk()")
        return self.distances_bulk(pairs)

    def mrca(self, a: Union[int, str], b: Union[int, str]) -> int:
        _deprecation_warning("mrca()", "common_ancestor()")
        return self.common_ancestor(a, b)

    def get_quartet_topology(self, a, b, c, d):
        _deprecation_warning("get_quartet_topology()", "quartet_topology()")
        return self.quartet_topology(a, b, c, d)

    def quartet_topologies(self, quartets):
        _deprecation_warning("quartet_topologies()", "quartet_topologies_bulk()")
        return self.quartet_topologies_bulk(quartets)
