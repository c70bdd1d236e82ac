"""(GPU) Grouped search end to end (vs_grouping_create / vs_search_groups /
vs_group_keys, include/vsearch.h "Grouped search").

References:
  (a) the engine's own full ranking of the query alone (vs_search, nq = 1,
      k = rows; held to the oracle by the existing suites) regrouped by
      tests/groups_ref.py: scores and rows must match bit for bit;
  (b) on exactly representable data (fp32 DOT, entries in {-1, 0, 1}/8: every
      dot product is a multiple of 2^-6 below 2^4, so any fp32 summation order
      is exact) a float64 numpy ranking, exactly. Two rows of different
      documents are identical and are query 0, so in every case two groups tie
      in their best score and the lower row decides; the test asserts the tie.
"""
import numpy as np
import pytest

import groups_ref as G

pytestmark = pytest.mark.gpu

NONE = G.GROUP_NONE
N = 20000
LIMITS = (1, 5, 128)
SIZES = (1, 3, 16)
NQ = 3


def _documents(n, rng, lo=1, hi=400):
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.integers(lo, hi + 1)))
    g = np.repeat(np.arange(len(lens), dtype=np.uint32), lens)[:n]
    return g, int(g.max()) + 2  # one more group than used: an empty one


def _layouts(n, seed):
    rng = np.random.default_rng(seed)
    g, ng = _documents(n, rng)
    g[rng.integers(0, n, n // 100)] = NONE  # a few rows without a document
    return {"contiguous": (g, ng), "shuffled": (g[rng.permutation(n)], ng)}


def _ternary(n, dim, rng):
    return rng.integers(-1, 2, (n, dim)).astype(np.float32) / 8


class Coll:
    def __init__(self, eng, pkg, name, dim, metric, dtype, X, Q, row_base=0):
        self.eng, self.name, self.X, self.Q, self.row_base = eng, name, X, Q, row_base
        self.n = X.shape[0]
        eng.create_collection(name, dim, metric, dtype, 0, row_base)
        eng.upsert(name, np.arange(self.n), X)
        self.layouts = _layouts(self.n, dim + metric + dtype)
        self._rank = {}

    def ranking(self, q, fid=0):
        """Keys of query q alone over the whole collection, descending."""
        if (q, fid) not in self._rank:
            if fid:
                s, r, c = self.eng.search_filter_id(self.name, self.Q[q], self.n, fid)
            else:
                s, r, c = self.eng.search(self.name, self.Q[q], self.n)
            self._rank[q, fid] = G.make_keys(G.score_image(s[0, :c[0]]), r[0, :c[0]])
        return self._rank[q, fid]


@pytest.fixture(scope="module")
def colls(engine, pkg):
    rng = np.random.default_rng(2024)
    centres = rng.standard_normal((200, 768)).astype(np.float32)
    X = centres[rng.integers(0, 200, N)] + 0.7 * rng.standard_normal((N, 768)).astype(np.float32)
    Q = centres[:NQ] + 0.3 * rng.standard_normal((NQ, 768)).astype(np.float32)
    out = {}
    for dt, dn in ((pkg.DTYPE_BF16, "bf16"), (pkg.DTYPE_F32, "f32")):
        for me, mn in ((pkg.METRIC_COSINE, "cos"), (pkg.METRIC_DOT, "dot")):
            out[dn, mn] = Coll(engine, pkg, f"grp_{dn}_{mn}", 768, me, dt, X, Q)
    out["generic"] = Coll(engine, pkg, "grp_f100", 100, pkg.METRIC_COSINE, pkg.DTYPE_F32,
                          np.ascontiguousarray(X[:, :100]), np.ascontiguousarray(Q[:, :100]),
                          row_base=5000)
    yield out
    for c in out.values():
        engine.drop_collection(c.name)


def _check(c, res, q0, nq, limit, S, gor, fid=0, what=None):
    groups, hits, scores, rows, count = res
    assert groups.shape == (nq, limit) and scores.shape == (nq, limit, S)
    for i in range(nq):
        ref = G.groups_ref(c.ranking(q0 + i, fid), gor, limit, S, c.row_base)
        w_groups, w_hits, w_keys, w_count = G.as_arrays(ref, limit, S)
        ctx = (what, c.name, q0 + i, limit, S)
        assert count[i] == w_count, ctx
        assert np.array_equal(groups[i], w_groups) and np.array_equal(hits[i], w_hits), ctx
        on = w_keys != 0
        got = np.where(on, G.make_keys(G.score_image(scores[i]), rows[i]), 0)
        assert np.array_equal(got, w_keys), ctx
        assert not scores[i][~on].any() and not rows[i][~on].any(), ctx


COLL_KEYS = [("bf16", "cos"), ("bf16", "dot"), ("f32", "cos"), ("f32", "dot"), "generic"]


@pytest.mark.parametrize("layout", ["contiguous", "shuffled"])
@pytest.mark.parametrize("key", COLL_KEYS, ids=lambda k: k if isinstance(k, str) else "-".join(k))
def test_equals_the_regrouped_full_ranking(engine, colls, key, layout):
    """(a)"""
    c = colls[key]
    gor, ng = c.layouts[layout]
    gid = engine.grouping_create(c.name, gor, ng)
    try:
        for nq in (1, NQ):
            for limit in LIMITS:
                for S in SIZES:
                    res = engine.search_groups(c.name, c.Q[:nq], limit, S, gid)
                    _check(c, res, 0, nq, limit, S, gor, what=layout)
        # a later query alone gives what it gave inside the batch
        res = engine.search_groups(c.name, c.Q[2], 5, 3, gid)
        _check(c, res, 2, 1, 5, 3, gor, what="alone")
    finally:
        engine.grouping_drop(gid)


@pytest.fixture(scope="module")
def exact(engine, pkg):
    rng = np.random.default_rng(77)
    X = _ternary(N, 768, rng)
    layouts = _layouts(N, 5)
    # two identical rows in different documents (under both layouts): query 0
    a = 4321
    b = next(r for r in range(9000, N)
             if all(g[r] != NONE and g[a] != NONE and g[r] != g[a] for g, _ in layouts.values()))
    X[b] = X[a]
    Q = np.stack([X[a], _ternary(1, 768, rng)[0], X[77]])
    c = Coll(engine, pkg, "grp_exact", 768, pkg.METRIC_DOT, pkg.DTYPE_F32, X, Q)
    c.layouts = layouts
    S64 = Q.astype(np.float64) @ X.astype(np.float64).T
    c.rank64 = []
    for s in S64:
        order = np.lexsort((np.arange(N), -s))
        c.rank64.append(G.make_keys(G.score_image(s[order].astype(np.float32)), order))
    c.tie_rows = (a, b)
    yield c
    engine.drop_collection(c.name)


@pytest.mark.parametrize("layout", ["contiguous", "shuffled"])
def test_exact_data_equals_float64(engine, exact, layout):
    """(b)"""
    c = exact
    gor, ng = c.layouts[layout]
    # the planted tie: query 0's two best groups have the same best score
    top2 = G.groups_ref(c.rank64[0], gor, 2, 1)
    (ga, (ka,)), (gb, (kb,)) = top2
    assert ga != gb and ka >> 32 == kb >> 32, "the fixture lost its tie"
    assert (int(G.key_rows(np.uint64(ka))), int(G.key_rows(np.uint64(kb)))) == c.tie_rows
    gid = engine.grouping_create(c.name, gor, ng)
    try:
        for nq in (1, NQ):
            for limit in LIMITS:
                for S in SIZES:
                    groups, hits, scores, rows, count = engine.search_groups(
                        c.name, c.Q[:nq], limit, S, gid)
                    for i in range(nq):
                        ref = G.groups_ref(c.rank64[i], gor, limit, S)
                        w_groups, w_hits, w_keys, w_count = G.as_arrays(ref, limit, S)
                        assert count[i] == w_count
                        assert np.array_equal(groups[i], w_groups)
                        assert np.array_equal(hits[i], w_hits)
                        on = w_keys != 0
                        got = np.where(on, G.make_keys(G.score_image(scores[i]), rows[i]), 0)
                        assert np.array_equal(got, w_keys), (layout, nq, limit, S, i)
                    assert groups[0, 0] == gor[c.tie_rows[0]]  # the lower row's group first
    finally:
        engine.grouping_drop(gid)


@pytest.mark.parametrize("key", [("bf16", "cos"), ("f32", "dot"), "generic"],
                         ids=lambda k: k if isinstance(k, str) else "-".join(k))
def test_own_groups_equal_plain_search(engine, colls, key):
    """(c) every row its own group, group_size 1: vs_search with k = limit."""
    c = colls[key]
    gid = engine.grouping_create(c.name, np.arange(c.n, dtype=np.uint32), c.n)
    try:
        for limit in LIMITS:
            groups, hits, scores, rows, count = engine.search_groups(c.name, c.Q, limit, 1, gid)
            for i in range(NQ):
                s, r, n = engine.search(c.name, c.Q[i], limit)
                assert count[i] == n[0] == limit and np.all(hits[i] == 1)
                assert np.array_equal(rows[i, :, 0], r[0])
                assert np.array_equal(scores[i, :, 0].view(np.uint32), s[0].view(np.uint32))
                assert np.array_equal(groups[i].astype(np.uint64) + c.row_base, r[0])
    finally:
        engine.grouping_drop(gid)


def test_resident_filter(engine, colls):
    """(d) a filter that masks one group's best row, all of another group, and
    one that masks every row."""
    c = colls["bf16", "cos"]
    gor, ng = c.layouts["contiguous"]
    gid = engine.grouping_create(c.name, gor, ng)
    fids = []
    try:
        base = G.groups_ref(c.ranking(0), gor, 5, 3)
        (g0, k0), (g1, _) = base[0], base[1]
        best_row = int(G.key_rows(np.uint64(k0[0])))
        allow = np.ones(c.n, bool)
        allow[best_row] = False
        allow[gor == g1] = False
        fids.append(engine.filter_create(c.name, allow))
        for nq, limit, S in ((1, 5, 3), (NQ, 128, 16), (1, 1, 1)):
            res = engine.search_groups(c.name, c.Q[:nq], limit, S, gid, fids[0])
            _check(c, res, 0, nq, limit, S, gor, fid=fids[0], what="filter")
            assert g1 not in res[0][0][:res[4][0]]
            assert best_row not in res[3][0]
        fids.append(engine.filter_create(c.name, np.zeros(c.n, bool)))
        groups, hits, scores, rows, count = engine.search_groups(c.name, c.Q, 5, 3, gid, fids[1])
        assert not count.any() and not groups.any() and not hits.any()
        assert not scores.any() and not rows.any()
        # the next unfiltered search is unharmed (scratch handed back clean)
        _check(c, engine.search_groups(c.name, c.Q[0], 5, 3, gid), 0, 1, 5, 3, gor)
    finally:
        for f in fids:
            engine.filter_drop(f)
        engine.grouping_drop(gid)


def _raises(pkg, code, fn, *a, **kw):
    with pytest.raises(pkg.VSError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


def test_stale_and_invalid(engine, pkg):
    """(e)"""
    rng = np.random.default_rng(1)
    name, n = "grp_stale", 1000
    X = rng.standard_normal((n + 10, 128)).astype(np.float32)
    engine.create_collection(name, 128, pkg.METRIC_COSINE, pkg.DTYPE_F32)
    try:
        engine.upsert(name, np.arange(n), X[:n])
        gor = (np.arange(n) // 10).astype(np.uint32)
        inv, nf = pkg.engine.VS_ERR_INVALID_ARG, pkg.engine.VS_ERR_NOT_FOUND
        _raises(pkg, inv, engine.grouping_create, name, gor[:-1], 100)      # wrong n_rows
        bad = gor.copy()
        bad[17] = 100
        _raises(pkg, inv, engine.grouping_create, name, bad, 100)            # id >= n_groups
        _raises(pkg, inv, engine.grouping_create, name, gor, n + 1)          # n_groups > rows
        _raises(pkg, nf, engine.grouping_create, "grp_missing", gor, 100)
        gid = engine.grouping_create(name, gor, 100)
        assert gid >= 1
        q = X[3]
        assert engine.search_groups(name, q, 5, 2, gid)[4][0] == 5
        for limit, S in ((0, 1), (129, 1), (1, 0), (1, 17)):
            _raises(pkg, inv, engine.search_groups, name, q, limit, S, gid)
        _raises(pkg, nf, engine.search_groups, name, q, 5, 2, gid + 1000)
        _raises(pkg, nf, engine.search_groups, name, q, 5, 2, gid, 987654)   # unknown filter
        # an append makes the grouping stale
        engine.upsert(name, np.arange(n, n + 10), X[n:])
        _raises(pkg, inv, engine.search_groups, name, q, 5, 2, gid)
        gid2 = engine.grouping_create(name, np.append(gor, [NONE] * 10).astype(np.uint32), 100)
        assert gid2 > gid  # ids are never reused
        res = engine.search_groups(name, q, 100, 16, gid2)
        assert res[4][0] == 100 and np.all(res[1][0] == 10)
        # vs_delete drops the collection's groupings
        engine.delete(name, [0, 1])
        _raises(pkg, nf, engine.search_groups, name, q, 5, 2, gid2)
        _raises(pkg, nf, engine.grouping_drop, gid2)
        # a dropped id is refused
        rows = engine.collection_info(name)["rows"]
        gid3 = engine.grouping_create(name, np.zeros(rows, np.uint32), 1)
        assert gid3 > gid2
        engine.grouping_drop(gid3)
        _raises(pkg, nf, engine.search_groups, name, q, 5, 2, gid3)
        _raises(pkg, nf, engine.grouping_drop, gid3)
    finally:
        engine.drop_collection(name)


def _device_groups(eng, torch, name, Q, limit, S, gid, fid=0):
    nq = Q.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    d_q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    d_keys = torch.full((nq, limit, S), -1, dtype=torch.int64, device="cuda")
    d_groups = torch.full((nq, limit), 7, dtype=torch.int32, device="cuda")
    eng.group_keys(name, d_q.data_ptr(), nq, Q.shape[1], limit, S, gid, fid, d_keys.data_ptr(),
                   d_groups.data_ptr(), st)
    torch.cuda.synchronize()
    return d_keys.cpu().numpy().view(np.uint64), d_groups.cpu().numpy().view(np.uint32)


def _host_as_keys(res):
    groups, hits, scores, rows, count = res
    keys = np.where(np.arange(scores.shape[2])[None, None, :] < hits[:, :, None],
                    G.make_keys(G.score_image(scores.reshape(-1)).reshape(scores.shape), rows), 0)
    gids = np.where(np.arange(groups.shape[1])[None, :] < count[:, None], groups, NONE)
    return keys.astype(np.uint64), gids.astype(np.uint32)


@pytest.mark.parametrize("key", [("bf16", "cos"), "generic"],
                         ids=lambda k: k if isinstance(k, str) else "-".join(k))
def test_group_keys_on_a_caller_stream(engine, colls, key):
    """(g)"""
    import torch
    c = colls[key]
    gor, ng = c.layouts["shuffled"]
    gid = engine.grouping_create(c.name, gor, ng)
    try:
        for nq, limit, S in ((1, 5, 3), (NQ, 128, 16), (NQ, 1, 1)):
            keys, gids = _device_groups(engine, torch, c.name, c.Q[:nq], limit, S, gid)
            w_keys, w_gids = _host_as_keys(engine.search_groups(c.name, c.Q[:nq], limit, S, gid))
            assert np.array_equal(keys, w_keys) and np.array_equal(gids, w_gids)
    finally:
        engine.grouping_drop(gid)


def test_placed_collection(pkg, colls):
    """(f) a placed collection answers from the second slot as from the first."""
    import torch
    src = colls["bf16", "cos"]
    n = 3000
    X, Q = src.X[:n], src.Q
    gor, ng = _layouts(n, 9)["contiguous"]
    with pkg.VectorEngine(shards=[0, 0], place_collections=True, engine_per_shard=True) as eng:
        res, dev = {}, {}
        for name in ("gp0", "gp1"):
            eng.create_collection(name, 768, pkg.METRIC_COSINE, pkg.DTYPE_BF16, n)
            eng.upsert(name, np.arange(n), X)
        for name in ("gp0", "gp1"):
            gid = eng.grouping_create(name, gor, ng)
            allow = np.arange(n) % 7 != 0
            fid = eng.filter_create(name, allow)
            res[name] = [eng.search_groups(name, Q, 5, 3, gid),
                         eng.search_groups(name, Q, 128, 16, gid, fid)]
            dev[name] = [_device_groups(eng, torch, name, Q, 5, 3, gid),
                         _device_groups(eng, torch, name, Q, 128, 16, gid, fid)]
            # against this collection's own full ranking
            for i in range(NQ):
                s, r, c = eng.search(name, Q[i], n)
                ranking = G.make_keys(G.score_image(s[0, :c[0]]), r[0, :c[0]])
                w = G.as_arrays(G.groups_ref(ranking, gor, 5, 3), 5, 3)
                got = res[name][0]
                assert got[4][i] == w[3] and np.array_equal(got[0][i], w[0])
                assert np.array_equal(_host_as_keys(got)[0][i], w[2])
            # a grouping of the other collection is refused
            other = "gp1" if name == "gp0" else "gp0"
            _raises(pkg, pkg.engine.VS_ERR_INVALID_ARG, eng.search_groups, other, Q, 5, 3, gid)
        for a, b in zip(res["gp0"], res["gp1"]):
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        for name in res:
            for host, device in zip(res[name], dev[name]):
                wk, wg = _host_as_keys(host)
                assert np.array_equal(device[0], wk) and np.array_equal(device[1], wg)
        eng.drop_collection("gp1")  # its groupings go with it
        _raises(pkg, pkg.engine.VS_ERR_NOT_FOUND, eng.search_groups, "gp1", Q, 5, 3, gid)


def test_row_striped_is_refused(pkg, colls):
    """(f) a row-striped collection keeps its rows' groups on several devices:
    vs_grouping_create and both searches refuse, deliberately."""
    import torch
    X, Q = colls["bf16", "cos"].X, colls["bf16", "cos"].Q
    with pkg.VectorEngine(shards=[0, 0]) as eng2:
        eng2.create_collection("gstriped", 768, pkg.METRIC_COSINE, pkg.DTYPE_BF16)
        eng2.upsert("gstriped", np.arange(64), X[:64])
        inv = pkg.engine.VS_ERR_INVALID_ARG
        _raises(pkg, inv, eng2.grouping_create, "gstriped", np.zeros(64, np.uint32), 1)
        _raises(pkg, inv, eng2.search_groups, "gstriped", Q, 5, 3, 1)
        d = torch.zeros(NQ * 768, dtype=torch.float32, device="cuda")
        k = torch.zeros(NQ * 15, dtype=torch.int64, device="cuda")
        g = torch.zeros(NQ * 5, dtype=torch.int32, device="cuda")
        _raises(pkg, inv, eng2.group_keys, "gstriped", d.data_ptr(), NQ, 768, 5, 3, 1, 0,
                k.data_ptr(), g.data_ptr(), 0)
