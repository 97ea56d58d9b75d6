"""ParaFit without a GPU: the host restatement behind st_parafit_codes (device = -1) against the integer restatement of
tests/parafit_reference.py with ==, the float statistics against the textbook eigh route within a derived bound, the
prefix property, chunking, a system whose every relabelling is the observation, the argument errors in the contract's
order, the golden systems through compare.parafit with both sides shuffled, and the plan and restatement under the
address / undefined-behaviour sanitizers in a program of their own.

The facade SuchLinkedTrees.parafit takes its matrices from the trees' distance kernels, so its values are checked in
tests/test_gpu_parafit.py; here its argument errors are, which are raised before anything is uploaded."""
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import parafit_reference as ref
from conftest import ROOT, golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare


def codes_case(n_f, n_s, L, seed, top=None):
    """(q_f, q_s, links sorted by (f, s), stream ids): random symmetric int32 codes -- every one +-top where given -- and
    L distinct links"""
    rng = np.random.default_rng(seed)

    def sym(n):
        if top is None:
            a = rng.integers(-(1 << 31), 1 << 31, (n, n), dtype=np.int64)
        else:
            a = np.where(rng.integers(0, 2, (n, n)) == 1, top, -top)
        return (np.tril(a) + np.tril(a, -1).T).astype(np.int32)
    cells = np.sort(rng.choice(n_f * n_s, L, replace=False))
    return sym(n_f), sym(n_s), np.stack([cells // n_s, cells % n_s], axis=1), rng.permutation(n_f) + 11


def library(q_f, q_s, links, streams, perms, seed, device=-1, chunk=0):
    total, obs, n_ge, every = _capi.parafit_codes(q_f, q_s, links[:, 0], links[:, 1], streams, perms, seed, device, chunk, keep=True)
    rows = _capi.parafit_ints(every)
    assert _capi.parafit_ints(obs) == rows[0]
    return _capi.parafit_ints(total), rows, n_ge.tolist()


@pytest.mark.parametrize("shape", [(3, 3, 3), (64, 64, 64), (5, 64, 63), (40, 3, 65), (9, 70, 40), (30, 66, 257)])
def test_integers_equal_the_reference(shape):
    q_f, q_s, links, streams = codes_case(*shape, seed=sum(shape))
    perms = 3 if shape[2] > 100 else 6
    traces, rows, _, link_n_ge = ref.run(q_f, q_s, links, streams, perms, 17)
    got = library(q_f, q_s, links, streams, perms, 17)
    assert got == (traces, rows, link_n_ge)
    # chunk_tasks changes the plan, never a value
    for chunk in (1, 2, shape[2] + 1):
        assert library(q_f, q_s, links, streams, perms, 17, chunk=chunk) == got


def test_carry_past_64_bits():
    top = (1 << 31) - 1
    q_f, q_s, links, streams = codes_case(20, 66, 257, 3, top=top)
    for sign in (1, -1):
        traces, rows, n_ge = library(sign * q_f, q_s, links, streams, 2, 5)
        want = ref.run(sign * q_f, q_s, links, streams, 2, 5)
        assert (traces, rows, n_ge) == (want[0], want[1], want[3])
    ones = np.full((20, 20), top, dtype=np.int32)      # every term +(2^31 - 1)^2: the largest sums there are at this L
    traces, rows, n_ge = library(ones, np.full((66, 66), top, dtype=np.int32), links, streams, 1, 5)
    assert traces == [257 * 257 * top * top] * 2 and traces[0] > 1 << 64 and rows[1] == [(2 * 257 - 1) * top * top] * 257 and n_ge == [1] * 257


def _patristic(tree, leaf_ids):
    """float64 distances between the leaves, from the flat arrays on the host"""
    parent, dist = np.asarray(tree._flat.parent), np.asarray(tree._flat.distance, dtype=np.float64)
    paths = []
    for v in leaf_ids:
        v, path, d = int(v), {}, 0.0
        while v != -1:
            path[v] = d
            d += dist[v]
            v = int(parent[v])
        paths.append(path)
    n = len(leaf_ids)
    D = np.zeros((n, n))
    for a in range(n):
        for b in range(a):
            D[a, b] = D[b, a] = min(paths[a][v] + paths[b][v] for v in paths[a] if v in paths[b])
    return D


def golden_system(which):
    """(d_a, d_b, links as (a position, b position)) of a golden system: both trees' leaves in id order"""
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    ta, tb = SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1])
    table = pd.read_csv(d + "/links.csv", index_col=0)
    ids_a, ids_b = sorted(ta.leaves.values()), sorted(tb.leaves.values())
    links = [(ids_a.index(ta.leaves[a]), ids_b.index(tb.leaves[b])) for a in table.index for b in table.columns if table.loc[a, b] > 0]
    return _patristic(ta, ids_a), _patristic(tb, ids_b), np.array(links)


@pytest.fixture(scope="module")
def systems():
    out = {which: golden_system(which) for which in ("gopher_louse", "fish_worm")}
    rng = np.random.default_rng(4)
    pts_a, pts_b = rng.random((30, 4)), rng.random((25, 3))
    euclid = lambda p: np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))      # noqa: E731
    cells = rng.choice(30 * 25, 60, replace=False)
    out["random"] = (euclid(pts_a), euclid(pts_b), np.stack([cells // 25, cells % 25], axis=1))
    return out


def bounds(g_f, g_s, links):
    """(bound of the trace, bound of a link statistic): what the fixed point may cost -- every code is within half a unit
    of its value and the largest code of a matrix is at least 2^30, so a product of two is within max|g_f| max|g_s| 2^-30
    (and a second-order 2^-62) of the exact one; the trace has L^2 terms, a link statistic 2 L - 1 -- plus the eigh
    reference's own rounding, measured inside the reference as the gap between its eigh and its float64 Gram route."""
    L = len(links)
    term = np.abs(g_f).max() * np.abs(g_s).max() * (2.0 ** -30 + 2.0 ** -62)
    t_e, l_e = ref.eigh_route(g_f, g_s, links[:, 0], links[:, 1])
    t_g, l_g = ref.gram(g_f, g_s, links[:, 0], links[:, 1])
    return L * L * term + abs(t_e - t_g), 2 * L * term + np.abs(l_e - l_g).max()


@pytest.mark.parametrize("transform", ["sqrt", "none"])
@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm", "random"])
def test_statistics_against_the_eigh_route(systems, which, transform):
    d_a, d_b, links = systems[which]
    for d_f, d_s, lk in ((d_b, d_a, links[:, ::-1]), (d_a, d_b, links)):      # (shuffle A: TreeB held; shuffle B)
        g_f, g_s = ref.centre(d_f, transform), ref.centre(d_s, transform)
        if transform == "sqrt":      # (the square root of a tree metric is Euclidean: no negative axis)
            assert min(np.linalg.eigvalsh(g_f).min(), np.linalg.eigvalsh(g_s).min()) > -1e-9 * np.abs(g_f).max()
        got = compare.parafit(d_f, d_s, lk, permutations=4, seed=6, transform=transform, keep_stats=True, device=None)
        streams = np.arange(len(d_f))
        for p in range(5):
            r = ref.relabel(lk, streams, len(d_s), 6, p)
            b_trace, b_link = bounds(g_f, g_s, np.stack([lk[:, 0], r], axis=1))      # (the reference's rounding under this relabelling)
            trace, link = ref.eigh_route(g_f, g_s, lk[:, 0], r)
            mine = (got.statistic, got.link_stat) if p == 0 else (got.perm_stats[p - 1], got.perm_link_stats[p - 1])
            gap_t, gap_l = abs(mine[0] - trace), np.abs(mine[1] - link).max()
            print(which, transform, p, "trace gap %.3g of %.3g, link gap %.3g of %.3g" % (gap_t, b_trace, gap_l, b_link))
            assert gap_t <= b_trace and gap_l <= b_link
        # the codes behind the floats are the library's own centring and fixed point
        q_f, s_f = _capi.mantel_quantise(compare.parafit_centre(compare.mantel_condensed(d_f)[0], len(d_f), transform))
        q_s, s_s = _capi.mantel_quantise(compare.parafit_centre(compare.mantel_condensed(d_s)[0], len(d_s), transform))
        assert (q_f == q_f.T).all() and (s_f, s_s) == (got.shift_f, got.shift_s)
        order = np.lexsort((lk[:, 1], lk[:, 0]))
        traces, rows, n_ge, link_n_ge = ref.run(q_f, q_s, lk[order], streams, 4, 6)
        assert got.trace_q == traces[0] and got.n_ge == n_ge and got.p_value == (n_ge + 1) / 5
        assert [got.link_stat_q[k] for k in order] == rows[0] and got.link_n_ge[order].tolist() == link_n_ge
        assert got.link_p.tolist() == [(c + 1) / 5 for c in got.link_n_ge.tolist()]
        assert got.statistic == float(traces[0]) * 2.0 ** -(s_f + s_s)


def test_prefix_chunks_forms_and_result(systems):
    d_a, d_b, links = systems["gopher_louse"]
    kw = dict(seed=21, keep_stats=True, device=None)
    long, short = compare.parafit(d_b, d_a, links[:, ::-1], permutations=30, **kw), compare.parafit(d_b, d_a, links[:, ::-1], permutations=7, **kw)
    assert long.perm_stats[:7].tobytes() == short.perm_stats.tobytes() and long.perm_link_stats[:7].tobytes() == short.perm_link_stats.tobytes()
    assert long.perm_trace_q[:7] == short.perm_trace_q and (long.statistic, long.link_stat_q) == (short.statistic, short.link_stat_q)
    for chunk in (1, 5, 1000):
        other = compare.parafit(d_b, d_a, links[:, ::-1], permutations=30, chunk_tasks=chunk, **kw)
        assert other.perm_link_stats.tobytes() == long.perm_link_stats.tobytes() and other.link_n_ge.tolist() == long.link_n_ge.tolist()
        assert other.perm_trace_q == long.perm_trace_q and other.n_ge == long.n_ge
    # condensed input, a shuffled link order: the same values, link by link
    rng = np.random.default_rng(0)
    mix = rng.permutation(len(links))
    i, j = np.tril_indices(len(d_b), -1)
    other = compare.parafit(d_b[i, j], d_a, links[mix][:, ::-1], permutations=30, **kw)
    assert other.trace_q == long.trace_q and other.link_stat_q == [long.link_stat_q[k] for k in mix] and other.n_ge == long.n_ge
    assert other.link_n_ge.tolist() == long.link_n_ge[mix].tolist() and other.perm_link_stats.tobytes() == long.perm_link_stats[:, mix].tobytes()
    # the result object
    stat, p, n = long
    assert (stat, p, n) == (long.statistic, long.p_value, len(links)) and len(long) == n and long.transform == "sqrt" and long.shuffle is None
    row = long.row(3)
    assert row["link_f"] == links[3, 1] and row["link_s"] == links[3, 0] and row["link_stat_q"] == long.link_stat_q[3] and row["link_p"] == long.link_p[3]
    frame = long.to_dataframe()
    assert len(frame) == n and frame["link_n_ge"].tolist() == long.link_n_ge.tolist()
    bare = compare.parafit(d_b, d_a, links[:, ::-1], permutations=7, seed=21, test_links=False, device=None)
    assert bare.link_p is None and bare.link_n_ge is None and bare.perm_stats is None and bare.link_stat_q == long.link_stat_q
    # other streams, other draws; the same streams, the same
    moved = compare.parafit(d_b, d_a, links[:, ::-1], permutations=7, shuffle_streams=np.arange(len(d_b)) + 1, **kw)
    assert moved.trace_q == short.trace_q and moved.perm_trace_q != short.perm_trace_q
    same = compare.parafit(d_b, d_a, links[:, ::-1], permutations=7, shuffle_streams=np.arange(len(d_b)), **kw)
    assert same.perm_trace_q == short.perm_trace_q


def test_every_f_leaf_linked_to_all_s_leaves(systems):
    """every relabelling maps the links onto themselves: all statistics tie with the observation and are counted"""
    d_a, d_b, _ = systems["random"]
    links = np.array([(f, s) for f in (0, 3, 4, 9) for s in range(len(d_b))])
    got = compare.parafit(d_a, d_b, links, permutations=19, seed=2, keep_stats=True, device=None)
    assert got.n_ge == 19 and got.p_value == 1.0 and got.perm_trace_q == [got.trace_q] * 19
    # Link1_p(l) is the statistic of the link that l was relabelled to -- another link of the same system -- so under
    # every permutation the statistics of one F leaf's links are the observed ones in another order, and link_p is 1
    # for the link with the smallest observed statistic of its leaf
    for f in (0, 3, 4, 9):
        mine = links[:, 0] == f
        for row in got.perm_link_stats:
            assert sorted(row[mine].tolist()) == sorted(got.link_stat[mine].tolist())
        assert got.link_p[mine][np.argmin(got.link_stat[mine])] == 1.0
    # all S leaves alike: every link statistic ties as well
    flat = np.ones_like(d_b) - np.eye(len(d_b))
    got = compare.parafit(d_a, flat, links, permutations=19, seed=2, device=None)
    assert got.p_value == 1.0 and got.link_n_ge.tolist() == [19] * len(links) and got.link_p.tolist() == [1.0] * len(links)


def test_links_of_one_f_leaf_keep_distinct_images():
    q_f, q_s, links, streams = codes_case(4, 9, 20, 8)
    for p in range(1, 6):
        r = ref.relabel(links, streams, 9, 3, p)
        for f in range(4):
            mine = r[links[:, 0] == f]
            assert len(set(mine.tolist())) == len(mine)


def _raw(q_f, q_s, links, streams, n_f=5, n_s=6, L=7, perms=1, chunk=0, device=-2, outs=True):
    lib = _capi.load()
    p = _capi._ptr
    lf = None if links is None else np.ascontiguousarray(links[:, 0], dtype=np.int32)
    ls = None if links is None else np.ascontiguousarray(links[:, 1], dtype=np.int32)
    st = None if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
    total, obs, n_ge = np.zeros(perms + 1 if 0 <= perms < 100 else 1, dtype=_capi.PARAFIT_SUM), np.zeros(L, dtype=_capi.PARAFIT_SUM), np.zeros(L, dtype=np.int64)
    return lib.st_parafit_codes(device, p(q_f), n_f, p(q_s), n_s, p(lf), p(ls), L, p(st), perms, 1, chunk, p(total) if outs else None, p(obs), p(n_ge), None)


def test_library_argument_errors_in_the_stated_order():
    q_f, q_s, links, streams = codes_case(5, 6, 7, 1)
    streams = np.arange(5)
    E = _capi.ST_ERR_ARG
    for kw, text in ((dict(q_f=None, n_f=2, n_s=2, L=2, perms=-1), "n_f = 2"), (dict(q_f=None, n_f=16385, n_s=2, L=2, perms=-1), "n_f = 16385"),
                     (dict(q_f=None, n_s=2, L=2, perms=-1), "n_s = 2"), (dict(q_f=None, L=2, perms=-1), "n_links = 2"),
                     (dict(q_f=None, L=16385, perms=-1), "n_links = 16385"), (dict(q_f=None, perms=-1), "< 0"), (dict(q_f=None, chunk=-1), "< 0"),
                     (dict(q_f=None, perms=1 << 31), "more than 2^31 - 1 permutations"), (dict(q_f=None, outs=False), "g_f, g_s, link_f, link_s or stream_f is NULL"),
                     (dict(outs=False), "total, link_obs or link_n_ge is NULL")):
        args = dict(q_f=q_f, q_s=q_s, links=links, streams=streams)
        args.update(kw)
        assert _raw(**args) == E and text in _capi.last_error(), text
    bad_links, bad_streams, bad_f, bad_s = links.copy(), streams.copy(), q_f.copy(), q_s.copy()
    bad_links[3, 1], bad_links[5, 0] = 6, -1
    bad_streams[2] = -1
    bad_f[1, 3] ^= 1
    bad_s[5, 2] ^= 1
    assert _raw(bad_f, bad_s, bad_links, bad_streams) == E and "link 3 " in _capi.last_error() and "S position is outside" in _capi.last_error()
    bad_links[3, 1] = links[3, 1]
    assert _raw(bad_f, bad_s, bad_links, bad_streams) == E and "link 5 " in _capi.last_error() and "F position is outside" in _capi.last_error()
    bad_links = links[[0, 1, 4, 3, 2, 5, 6]]
    assert _raw(bad_f, bad_s, bad_links, bad_streams) == E and "link 3 " in _capi.last_error() and "strictly increasing" in _capi.last_error()
    bad_links = links[[0, 1, 2, 3, 3, 5, 6]]
    assert _raw(bad_f, bad_s, bad_links, bad_streams) == E and "link 4 " in _capi.last_error() and "strictly increasing" in _capi.last_error()
    assert _raw(bad_f, bad_s, links, bad_streams) == E and "stream_f[2] < 0" in _capi.last_error()
    assert _raw(bad_f, bad_s, links, streams) == E and "g_f is not symmetric: g_f[1][3]" in _capi.last_error()
    assert _raw(q_f, bad_s, links, streams) == E and "g_s is not symmetric: g_s[2][5]" in _capi.last_error()
    assert _raw(q_f, q_s, links, streams) == E and "device must be -1" in _capi.last_error()
    assert _raw(q_f, q_s, links, streams, device=-1) == _capi.ST_OK


def test_python_errors_name_the_offender(systems):
    d_a, d_b, links = systems["random"]
    for kw, text in ((dict(transform="square"), "transform"), (dict(permutations=-1), "permutations"), (dict(seed=-1), "seed"),
                     (dict(chunk_tasks=-1), "chunk_tasks"), (dict(links=links[:2]), "2 links"), (dict(links=links.astype(float)), "integer array"),
                     (dict(links=np.vstack([links, [[30, 0]]])), "link 60: the F position 30"), (dict(links=np.vstack([links, [[0, -1]]])), "link 60: the S position -1"),
                     (dict(links=np.vstack([links[:5], links[2:3]])), "links 2 and 5 are the same"), (dict(shuffle_streams=np.arange(29)), "shuffle_streams"),
                     (dict(shuffle_streams=-np.arange(30)), "shuffle_streams"), (dict(d_f=d_a[:, :5]), "not square"), (dict(d_s=d_b + np.triu(d_b)), "d_s is not symmetric")):
        args = dict(d_f=d_a, d_s=d_b, links=links, permutations=3, seed=1, device=None)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            compare.parafit(**args)


def test_facade_errors_raised_before_any_upload():
    d = golden_path("gopher_louse")
    ta, tb = SuchTree(d + "/gopher.tree"), SuchTree(d + "/lice.tree")
    slt = SuchLinkedTrees(ta, tb, pd.read_csv(d + "/links.csv", index_col=0))
    for kw in ({"shuffle": "C"}, {"transform": "square"}, {"permutations": -1}, {"seed": -1}):
        with pytest.raises(ValueError):
            slt.parafit(**kw)
    assert ta._dev_tree is None and tb._dev_tree is None


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_parafit_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_parafit")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_parafit.cpp"), os.path.join(csrc, "parafit_plan.cpp"),
                           os.path.join(csrc, "mantel_plan.cpp"), os.path.join(csrc, "dispersion_plan.cpp"), os.path.join(csrc, "hommola_plan.cpp"),
                           os.path.join(csrc, "compare_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize parafit ok" in out.stdout
