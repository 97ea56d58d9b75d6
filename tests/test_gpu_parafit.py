"""ParaFit on the GPU: the device's totals, link records and counts equal the host restatement (device = -1, itself
checked against tests/parafit_reference.py in tests/test_parafit_host.py) bit for bit -- on both kernel forms, at every
alignment of a staged row, on the three sort classes, with rows above 32 KiB and at the 64 KiB limit, under chunk cuts,
at the 128-bit carries -- and the facade gives the same values as the host route on the golden systems."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare
from test_parafit_host import codes_case, library

pytestmark = pytest.mark.gpu


def _same(q_f, q_s, links, streams, perms, seed=17, chunk=0, bare=True):
    host = library(q_f, q_s, links, streams, perms, seed, -1)
    got = library(q_f, q_s, links, streams, perms, seed, 0, chunk)
    assert got == host
    traces, rows, n_ge = got
    # the counts recomputed from the kept rows
    assert n_ge == [sum(r[l] >= rows[0][l] for r in rows[1:]) for l in range(len(links))]
    if not bare:      # (the largest matrices: one device call)
        return got
    # without the kept rows: the same totals, observations and counts
    total, obs, count, _ = _capi.parafit_codes(q_f, q_s, links[:, 0], links[:, 1], streams, perms, seed, 0, chunk)
    assert (_capi.parafit_ints(total), _capi.parafit_ints(obs), count.tolist()) == (traces, rows[0], n_ge)
    return got


@pytest.mark.parametrize("shape", [(3, 3, 3), (64, 64, 64), (5, 64, 63)])
def test_wave_form(shape):
    _same(*codes_case(*shape, seed=shape[2]), perms=9)


@pytest.mark.parametrize("shape", [(40, 3, 65), (30, 65, 257), (30, 66, 257), (30, 67, 257), (30, 257, 257), (3000, 64, 131)])
def test_row_form_at_every_row_alignment_and_a_tail(shape):
    """n_s = 65, 66, 67, 257: row r of g_s starts at every residue mod 4 words; L = 257 and 131 are no multiple of 4;
    (40, 3, 65) and (3000, 64, 131) take the row form with a wave-sized S side"""
    if shape[0] == 3000:      # (a cheap symmetric matrix at a large F side: most F leaves have no link)
        rng = np.random.default_rng(5)
        a = rng.integers(-(1 << 31), 1 << 31, 3000, dtype=np.int64).astype(np.int32)
        _, q_s, links, streams = codes_case(200, shape[1], shape[2], seed=9)
        links[:, 0] = np.sort(rng.choice(3000, shape[2], replace=False))
        _same(a[:, None] ^ a[None, :], q_s, links, np.arange(3000), perms=2)
        return
    _same(*codes_case(*shape, seed=shape[1]), perms=3)


@pytest.mark.parametrize("n_s, L", [(2049, 70), (8200, 65), (16384, 65)])
def test_large_sort_class_and_long_rows(n_s, L):
    """n_s = 2049: the large sort class; 8200: a staged row above 32 KiB; 16384: the largest row, 64 KiB, one permutation"""
    rng = np.random.default_rng(n_s)
    a = rng.integers(-(1 << 31), 1 << 31, n_s, dtype=np.int64).astype(np.int32)
    q_f, _, _, streams = codes_case(12, 8, 10, seed=2)
    cells = np.sort(rng.choice(12 * n_s, L, replace=False))
    links = np.stack([cells // n_s, cells % n_s], axis=1)
    _same(q_f, a[:, None] ^ a[None, :], links, streams, perms=1 if n_s == 16384 else 2, bare=n_s < 8000)


@pytest.mark.parametrize("chunk", [1, 7, 100])
def test_chunks_cut_inside_a_permutation_and_a_block(chunk):
    case = codes_case(30, 70, 65, seed=4)
    whole = _same(*case, perms=5)
    assert _same(*case, perms=5, chunk=chunk) == whole      # (chunk_tasks also bounds the block: 1, 6 and 6 permutations)
    wave = codes_case(9, 20, 33, seed=4)
    assert _same(*wave, perms=11, chunk=chunk) == _same(*wave, perms=11)


def test_carries_past_64_bits_both_signs():
    top = (1 << 31) - 1
    q_f, q_s, links, streams = codes_case(20, 66, 257, 3, top=top)
    for sign in (1, -1):
        _same(sign * q_f, q_s, links, streams, perms=2)
    ones_f, ones_s = np.full((20, 20), top, dtype=np.int32), np.full((66, 66), top, dtype=np.int32)
    for sign in (1, -1):
        traces, rows, n_ge = _same(sign * ones_f, ones_s, links, streams, perms=1)
        assert traces == [sign * 257 * 257 * top * top] * 2 and rows[1] == [sign * (2 * 257 - 1) * top * top] * 257 and n_ge == [1] * 257


@pytest.mark.parametrize("n_s, L", [(20, 12), (90, 80)])
def test_links_of_one_f_leaf_keep_distinct_images(n_s, L):
    """g_f all ones, g_s diagonal with entry i + 1 at position i, every link on one F leaf: link l's statistic is
    (2 c - 1) (r + 1) with r its image and c the links that share it -- distinct values up to n_s mean distinct images"""
    rng = np.random.default_rng(L)
    links = np.stack([np.full(L, 1), np.sort(rng.choice(n_s, L, replace=False))], axis=1)
    q_s = np.diag(np.arange(1, n_s + 1)).astype(np.int32)
    _, rows, _ = _same(np.ones((3, 3), dtype=np.int32), q_s, links, np.array([5, 6, 7]), perms=6)
    assert rows[0] == (links[:, 1] + 1).tolist()
    for row in rows[1:]:
        assert len(set(row)) == L and 1 <= min(row) and max(row) <= n_s and row != rows[0]


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), pd.read_csv(d + "/links.csv", index_col=0))


@pytest.mark.parametrize("shuffle", ["A", "B"])
@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
def test_facade_agrees_with_the_host_route(which, shuffle):
    slt = _slt(which)
    before = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist), slt.subset_a_root, slt.subset_b_root)
    got = slt.parafit(permutations=99, seed=13, shuffle=shuffle, keep_stats=True)
    after = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist), slt.subset_a_root, slt.subset_b_root)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    ll = np.asarray(slt.linklist, dtype=np.int64)
    assert got.shuffle == shuffle and got.link_a.tolist() == ll[:, 1].tolist() and got.link_b.tolist() == ll[:, 0].tolist() and got.n_links == len(ll)
    assert got.link_names[0] == (slt.TreeA.leaf_nodes[int(ll[0, 1])], slt.TreeB.leaf_nodes[int(ll[0, 0])])
    # the same call assembled by hand, on the host: the S and F leaves depth-first, the F leaf ids as streams
    tree_s, tree_f, col_s, col_f = (slt.TreeA, slt.TreeB, 1, 0) if shuffle == "A" else (slt.TreeB, slt.TreeA, 0, 1)
    univ_s, univ_f = tree_s._depth_first_leaves(), tree_f._depth_first_leaves()
    pos = lambda univ, ids: np.array([univ.tolist().index(v) for v in ids.tolist()])      # noqa: E731
    links = np.stack([pos(univ_f, ll[:, col_f]), pos(univ_s, ll[:, col_s])], axis=1)
    host = compare.parafit(tree_f.pairwise_distances(univ_f.tolist()), tree_s.pairwise_distances(univ_s.tolist()), links, permutations=99, seed=13,
                           shuffle_streams=univ_f, keep_stats=True, device=None)
    for k in ("statistic", "p_value", "n_ge", "trace_q", "perm_trace_q", "shift_f", "shift_s", "link_stat_q"):
        assert getattr(got, k) == getattr(host, k), k
    for k in ("link_stat", "link_n_ge", "link_p", "perm_stats", "perm_link_stats"):
        assert getattr(got, k).tobytes() == getattr(host, k).tobytes(), k
    assert got.p_value == (got.n_ge + 1) / 100 and got.link_p.tolist() == [(c + 1) / 100 for c in got.link_n_ge.tolist()]
    # a prefix in `permutations`, and the other transform runs through the same path
    short = slt.parafit(permutations=9, seed=13, shuffle=shuffle, keep_stats=True)
    assert short.perm_trace_q == got.perm_trace_q[:9] and short.perm_link_stats.tobytes() == got.perm_link_stats[:9].tobytes()
    other = slt.parafit(permutations=9, seed=13, shuffle=shuffle, transform="none")
    assert other.transform == "none" and other.trace_q != got.trace_q
