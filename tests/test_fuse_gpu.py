"""Fused search on the device (vs_search_fused / vs_fuse_keys, include/vsearch.h
"Fused search") against tests/fuse_ref.py.

* RRF must EQUAL the reference bit for bit: a term is one IEEE fp32 division of
  exactly representable operands and the sum's order is part of the rule, so
  nothing is left to rounding.
* DBSF equals it exactly where the fp64 statistics are exact in any summation
  order (dyadic scores), and on Gaussian scores is held to tau = 2^-16 absolute:
  |z| <= (n-1)/sqrt(n) < 11.3 for n <= 128, so a term lies in (-1.4, 2.4); a
  term's single rounding to fp32 is at most 2^-22 off, 8 terms 2^-19, and the
  at most 7 additions of partial sums below 32 add at most 7 x 2^-19.
* End to end the collections hold entries in {-1, 0, 1}/8 under DOT (as
  test_mmr_gpu.py's exact fixture), so every score is exact on every scan path
  and the candidate lists are numpy's exact top-F.
"""
import numpy as np
import pytest

import fuse_ref as FR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 128, 128), (2, 3, 2), (3, 100, 37), (5, 17, 17), (8, 128, 10),
          (8, 128, 128)]
TAU = 2.0 ** -16


def _fuse(engine, lists, k, fusion=FR.RRF, rrf_k=0):
    """vs_fuse_keys over uploaded lists [nq][n_sub][k_in]; the output sits between
    two guard rows, which must come back untouched."""
    import torch
    nq, n_sub, k_in = lists.shape
    d_in = torch.from_numpy(np.ascontiguousarray(lists).view(np.int64)).cuda()
    d_out = torch.full((nq + 2, k), -1, dtype=torch.int64, device="cuda")
    engine.fuse_keys(d_in.data_ptr(), nq, n_sub, k_in, k, fusion, rrf_k,
                     d_out[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[0] == -1).all() and (out[-1] == -1).all(), "wrote outside its output"
    assert np.array_equal(d_in.cpu().numpy().view(np.uint64), lists), "changed its input"
    return np.ascontiguousarray(out[1:-1]).view(np.uint64)


def _check_rrf(engine, lists, k, rrf_k=0, what=None):
    got = _fuse(engine, lists, k, FR.RRF, rrf_k)
    for q in range(lists.shape[0]):
        want = FR.rrf(lists[q], k, rrf_k)
        assert np.array_equal(got[q], want), (what, lists.shape, k, rrf_k, q)
    return got


# ---- vs_fuse_keys, RRF -----------------------------------------------------------
@pytest.mark.parametrize("n_sub,k_in,k", SHAPES)
def test_rrf_shapes(engine, n_sub, k_in, k):
    _check_rrf(engine, FR.overlap(3, n_sub, k_in, pool=k_in + k_in // 4 + 1), k, what="overlap")
    _check_rrf(engine, FR.disjoint(3, n_sub, k_in), k, what="disjoint")
    _check_rrf(engine, FR.identical(3, n_sub, k_in), k, what="identical")


@pytest.mark.parametrize("k", [1, 10, 128])
def test_rrf_reversed_pair(engine, k):
    got = _check_rrf(engine, FR.reversed_pair(3), k, what="reversed")
    if k == 128:   # exact ties all the way: pairs of equal scores, the lower row first
        sc, rows = FR.key_score(got), FR.key_row(got)
        assert np.all(sc[:, 0::2] == sc[:, 1::2]) and np.all(rows[:, 0::2] < rows[:, 1::2])


@pytest.mark.parametrize("nq", [1, 3, 257])
def test_rrf_batch_sizes(engine, nq):
    _check_rrf(engine, FR.overlap(nq, 5, 17, pool=24, seed=nq), 17)
    if nq <= 3:
        _check_rrf(engine, FR.overlap(nq, 8, 128, seed=nq), 128)


@pytest.mark.parametrize("rrf_k", [0, 1, 2, 60, 65536])
def test_rrf_constant(engine, rrf_k):
    lists = FR.overlap(3, 8, 128)
    got = _check_rrf(engine, lists, 10, rrf_k)
    if rrf_k == 0:   # the default is 2
        assert np.array_equal(got, _fuse(engine, lists, 10, FR.RRF, 2))


def test_rrf_empty_slots(engine):
    """Short lists 0-padded from some slot, one wholly empty list, an all-empty
    query, and k above the number of distinct rows (a zero tail)."""
    lists = FR.overlap(4, 8, 128)
    for l, cut in enumerate((128, 100, 64, 1, 0, 127, 33, 5)):
        lists[0, l, cut:] = 0
    lists[1] = 0
    lists[2, 1:] = 0
    lists[2, 0, 7:] = 0
    for k in (10, 128):
        got = _check_rrf(engine, lists, k)
        assert not got[1].any()
        assert np.count_nonzero(got[2]) == 7 and not got[2, 7:].any()
    # every query empty
    assert not _fuse(engine, np.zeros((3, 5, 17), np.uint64), 17).any()


def test_rrf_rows_near_2_32(engine):
    lists = FR.overlap(2, 8, 128, row0=2 ** 32 - 1 - 160)
    assert int(FR.key_row(lists).max()) == 2 ** 32 - 2
    _check_rrf(engine, lists, 128)
    _check_rrf(engine, lists[:, :3, :100].copy(), 37)


def test_rrf_runs_of_eight_and_one(engine):
    """One row in all 8 lists among neighbours (by row number) that sit in one
    list each: runs of length 8 and 1 side by side in the sort."""
    rng = np.random.default_rng(8)
    lists = np.zeros((2, 8, 16), np.uint64)
    for q in range(2):
        lone = np.setdiff1d(np.arange(940, 1061), [1000])
        lone = rng.permutation(lone)[:8 * 15].reshape(8, 15)
        for l in range(8):
            lists[q, l] = FR._list(np.insert(lone[l], 2 * l, 1000))
    got = _check_rrf(engine, lists, 16)
    assert np.all(FR.key_row(got[:, 0]) == 1000)


def test_fuse_keys_errors(engine, pkg):
    inv = pkg.engine.VS_ERR_INVALID_ARG
    # (nq, n_sub, k_in, k, fusion, rrf_k), the word its message must hold; the
    # pointers are never touched
    for a, word in (((1, 0, 8, 4, 0, 0), "n_sub"), ((1, 9, 8, 4, 0, 0), "n_sub"),
                    ((1, 2, 8, 0, 0, 0), "k must"), ((1, 2, 128, 129, 0, 0), "k 129"),
                    ((1, 2, 129, 4, 0, 0), "129"), ((1, 2, 0, 4, 0, 0), "k_in"),
                    ((1, 2, 8, 9, 0, 0), "k 9"), ((1, 2, 8, 4, 2, 0), "fusion"),
                    ((1, 2, 8, 4, -1, 0), "fusion"), ((1, 2, 8, 4, 0, 65537), "rrf_k"),
                    ((1, 2, 8, 4, 1, 1), "rrf_k"), ((1, 2, 8, 4, 1, 60), "rrf_k")):
        with pytest.raises(pkg.VSError) as e:
            engine.fuse_keys(0, *a, 0)
        assert e.value.code == inv and word in e.value.msg, (a, e.value.code, e.value.msg)
    with pytest.raises(pkg.VSError) as e:   # valid arguments, no lists
        engine.fuse_keys(0, 1, 2, 8, 4, 0, 0, 0)
    assert e.value.code == inv and "NULL" in e.value.msg
    engine.fuse_keys(0, 0, 2, 8, 4, 0, 0, 0)   # nq = 0: nothing to do


# ---- vs_fuse_keys, DBSF ----------------------------------------------------------
def _check_dbsf_exact(engine, lists, k, what):
    got = _fuse(engine, lists, k, FR.DBSF)
    for q in range(lists.shape[0]):
        assert np.array_equal(got[q], FR.dbsf(lists[q], k)[0]), (what, q)
    return got


def test_dbsf_flat_lists_give_half(engine):
    """sigma = 0 (equal scores) or n_l = 1: every term is 0.5."""
    lists = np.zeros((2, 4, 8), np.uint64)
    lists[0, 0] = FR._list(np.arange(8), np.full(8, 3.25, np.float32))
    lists[0, 1] = FR._list(np.arange(4, 12), np.full(8, -1.0, np.float32))
    lists[0, 2, :1] = FR._list([6], [9.0])          # n_l = 1
    lists[0, 3, :1] = FR._list([40], [-0.5])        # n_l = 1, a row of its own
    lists[1, 0, :1] = FR._list([3], [1.0])
    got = _check_dbsf_exact(engine, lists, 8, "flat")
    sc, rows = FR.key_score(got[0]), FR.key_row(got[0])
    assert rows.tolist() == [6, 4, 5, 7, 0, 1, 2, 3]   # 1.5, then 1.0 x 3, then 0.5 by row
    assert sc.tolist() == [1.5, 1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5]
    assert FR.key_row(got[1, 0]) == 3 and FR.key_score(got[1, 0]) == 0.5 and not got[1, 1:].any()


def test_dbsf_thirds(engine):
    """Lists {a, 0, -a}, a a power of two: mu = 0 and sigma = a exactly, so the
    terms are 2/3, 1/2 and 1/3, each rounded once."""
    lists = np.zeros((1, 3, 3), np.uint64)
    for l, (a, rows) in enumerate(((1.0, [1, 2, 3]), (4.0, [2, 3, 1]), (0.125, [3, 9, 2]))):
        lists[0, l] = FR._list(rows, [a, 0.0, -a])
    got = _check_dbsf_exact(engine, lists, 3, "thirds")
    f32 = np.float32
    t23, t13 = f32(2 / 3), f32(1 / 3)
    want = {1: f32(t23 + t13), 2: f32(f32(f32(0.5) + t23) + t13), 3: f32(f32(t13 + f32(0.5)) + t23)}
    for key in got[0]:
        assert FR.key_score(key) == want[int(FR.key_row(key))]


def test_dbsf_negative_scores_and_minus_zero(engine):
    """Dyadic scores, so the fp64 sums are exact in any order and every later
    operation (the two divisions, the square root, the products and differences)
    is one IEEE operation on equal operands: each list's sum is a multiple of
    its length, so its mean is exact too. -0.0 is stored as +0.0 by
    vs_key_encode."""
    lists = np.zeros((2, 4, 6), np.uint64)
    lists[0, 0, :3] = FR._list([5, 6, 7], [-0.0, -2.0, -4.0])
    lists[0, 1, :4] = FR._list([7, 6, 9, 5], [-1.0, -1.5, -2.0, -2.5])
    lists[0, 2, :6] = FR._list([9, 5, 1, 2, 3, 4], [-0.25, -0.5, -3.0, -3.5, -8.0, -8.75])
    lists[0, 3, :2] = FR._list([2, 6], [0.0, -0.0])                  # equal after encoding
    lists[1, 0, :5] = FR._list([1, 2, 3, 4, 5], [7.0, 0.5, -0.0, -0.75, -6.75])
    lists[1, 1, :3] = FR._list([4, 2, 8], [-1024.0, -1026.0, -4094.0])
    for l in lists.reshape(-1, 6):   # well-formed: sorted descending, 0-padded
        n = np.count_nonzero(l)
        assert np.all(l[:max(n, 1) - 1] > l[1:max(n, 1)]) and not l[n:].any()
    got = _check_dbsf_exact(engine, lists, 6, "negative")
    assert np.count_nonzero(got[0]) == 6 and np.count_nonzero(got[1]) == 6


@pytest.mark.parametrize("n_sub,k_in,k", [(8, 128, 10), (3, 100, 37), (8, 128, 128)])
def test_dbsf_gaussian_scores(engine, n_sub, k_in, k):
    rng = np.random.default_rng(n_sub * 1000 + k)
    nq, pool = 4, k_in + k_in // 4
    lists = np.zeros((nq, n_sub, k_in), np.uint64)
    for q in range(nq):
        for l in range(n_sub):
            sc = -np.sort(-rng.standard_normal(k_in).astype(np.float32))
            lists[q, l] = FR._list(rng.permutation(pool)[:k_in], sc)
    lists[0, n_sub - 1, k_in // 2:] = 0   # a short list
    got = _fuse(engine, lists, k, FR.DBSF)
    worst = 0.0
    for q in range(nq):
        _, f64 = FR.dbsf(lists[q], k)
        n = min(k, len(f64))
        assert np.count_nonzero(got[q]) == n and not got[q, n:].any(), q
        rows, sc = FR.key_row(got[q, :n]).tolist(), FR.key_score(got[q, :n]).astype(np.float64)
        assert len(set(rows)) == n and all(r in f64 for r in rows), q
        err = np.abs(sc - np.array([f64[r] for r in rows]))
        worst = max(worst, float(err.max()))
        assert np.all(err <= TAU), (q, float(err.max()))
        assert np.all(sc[:-1] >= sc[1:]), q
        rest = [v for r, v in f64.items() if r not in set(rows)]
        if rest:
            assert max(rest) <= sc[-1] + TAU, (q, max(rest), sc[-1])
    print(f"dbsf ({n_sub},{k_in},{k}): worst |fp32 - float64| {worst:.3e} (tau {TAU:.3e})")


# ---- vs_search_fused, end to end ---------------------------------------------------
def _ternary(n, dim, seed):
    """test_mmr_gpu.py's exact fixture: rows = one of 40 centres with 15% of the
    entries redrawn, entries in {-1, 0, 1}/8; every dot product is exact."""
    rng = np.random.default_rng(seed)
    C = rng.integers(-1, 2, (40, dim)).astype(np.float32)
    X = C[np.arange(n) % 40].copy()
    redraw = rng.random((n, dim)) < 0.15
    X[redraw] = rng.integers(-1, 2, int(redraw.sum())).astype(np.float32)
    # 32 questions x 8 rewrites: a centre with 15% redrawn per rewrite
    Q = np.repeat(C[:32, None, :], 8, axis=1).copy()
    redraw = rng.random(Q.shape) < 0.15
    Q[redraw] = rng.integers(-1, 2, int(redraw.sum())).astype(np.float32)
    return X / 8, Q / 8


class _Coll:
    def __init__(self, eng, pkg, name, n, dim, bf16, seed, row_base=0):
        self.name, self.row_base = name, row_base
        self.X, self.Q = _ternary(n, dim, seed)
        eng.create_collection(name, dim, pkg.METRIC_DOT, pkg.DTYPE_BF16 if bf16 else pkg.DTYPE_F32,
                              0, row_base)
        eng.upsert(name, np.arange(n), self.X)
        # [32][8][n] exact scores
        self.S = self.Q.astype(np.float64) @ self.X.astype(np.float64).T

    def lists(self, nq, n_sub, F, allow=None):
        """numpy's exact top-F of every sub-query, as key lists [nq][n_sub][F']
        with F' = min(F, rows) (score desc, row asc; 0-padded when few are allowed)."""
        n = self.X.shape[0]
        idx = np.arange(n) if allow is None else np.flatnonzero(allow)
        out = np.zeros((nq, n_sub, min(F, n)), np.uint64)
        for q in range(nq):
            for l in range(n_sub):
                s = self.S[q, l, idx]
                order = idx[np.lexsort((idx, -s))][:F]
                out[q, l, :len(order)] = FR.key_encode(self.S[q, l, order], order + self.row_base)
        return out


@pytest.fixture(scope="module")
def exact(engine, pkg):
    colls = {"b768": _Coll(engine, pkg, "fuse_b768", 3000, 768, True, 11),
             "f768": _Coll(engine, pkg, "fuse_f768", 3000, 768, False, 11),
             "b100": _Coll(engine, pkg, "fuse_b100", 1000, 100, True, 12, row_base=1000)}
    yield colls
    for c in colls.values():
        engine.drop_collection(c.name)


def _assert_fused(res, lists, k, fusion=FR.RRF, rrf_k=0, what=None):
    s, r, c = res
    for q in range(lists.shape[0]):
        want = FR.fuse(lists[q], k, fusion, rrf_k)
        n = int(np.count_nonzero(want))
        assert c[q] == n, (what, q, c[q], n)
        assert np.array_equal(r[q, :n], FR.key_row(want[:n])), (what, q)
        assert np.array_equal(s[q, :n].view(np.uint32), FR.key_score(want[:n]).view(np.uint32)), (what, q)
        assert not r[q, n:].any() and not s[q, n:].any(), (what, q)


def test_fixture_lists_overlap(exact):
    """The rewrites of one question share rows, so fusion has terms to add."""
    L = exact["b768"].lists(4, 3, 64)
    for q in range(4):
        rows = [set(FR.key_row(l).tolist()) for l in L[q]]
        assert len(rows[0] & rows[1] & rows[2]) >= 5
        assert len(rows[0] | rows[1] | rows[2]) > 64


@pytest.mark.parametrize("key", ["b768", "f768", "b100"])
@pytest.mark.parametrize("nq,n_sub,F,k", [(1, 2, 8, 5), (4, 3, 64, 10), (32, 8, 128, 128)])
def test_search_fused_rrf(engine, exact, key, nq, n_sub, F, k):
    c = exact[key]
    res = engine.search_fused(c.name, c.Q[:nq, :n_sub], k, F)
    _assert_fused(res, c.lists(nq, n_sub, F), k, what=(key, nq, n_sub, F, k))


def test_search_fused_defaults_and_dbsf(engine, pkg, exact):
    c = exact["b768"]
    # prefetch_limit 0 = min(4 k, 128); rrf_k 60
    _assert_fused(engine.search_fused(c.name, c.Q[:4, :3], 10, 0, pkg.FUSION_RRF, 60),
                  c.lists(4, 3, 40), 10, FR.RRF, 60, "default F")
    # DBSF end to end: scores are multiples of 2^-6, the sums exact in any order
    _assert_fused(engine.search_fused(c.name, c.Q[:4, :3], 10, 64, pkg.FUSION_DBSF),
                  c.lists(4, 3, 64), 10, FR.DBSF, 0, "dbsf")


def test_search_fused_resident_filter(engine, exact):
    c = exact["b768"]
    allow = np.random.default_rng(5).random(c.X.shape[0]) < 0.4
    fid = engine.filter_create(c.name, allow)
    try:
        _assert_fused(engine.search_fused(c.name, c.Q[:4, :3], 10, 64, filter_id=fid),
                      c.lists(4, 3, 64, allow), 10, what="filter")
    finally:
        engine.filter_drop(fid)
    few = np.zeros(c.X.shape[0], bool)   # fewer allowed rows than k: a zero tail
    few[[5, 45, 2999]] = True
    fid = engine.filter_create(c.name, few)
    try:
        res = engine.search_fused(c.name, c.Q[:2, :4], 8, 32, filter_id=fid)
        assert res[2].tolist() == [3, 3]
        _assert_fused(res, c.lists(2, 4, 32, few), 8, what="few")
    finally:
        engine.filter_drop(fid)


def test_search_fused_fewer_rows_than_prefetch(engine, pkg):
    c = _Coll(engine, pkg, "fuse_small", 20, 768, True, 41)
    try:
        for nq in (1, 4):
            res = engine.search_fused(c.name, c.Q[:nq, :3], 30, 64)
            assert np.all(res[2] == 20)
            _assert_fused(res, c.lists(nq, 3, 64), 30, what=("small", nq))
    finally:
        engine.drop_collection(c.name)


def test_single_sub_query_is_plain_search(engine, exact):
    c = exact["b768"]
    for nq in (1, 8):
        q = c.Q[:nq, :1]
        s, r, cnt = engine.search_fused(c.name, q, 10, 64)
        _, pr, pc = engine.search(c.name, q[:, 0], 10)
        assert np.array_equal(r, pr) and np.array_equal(cnt, pc)
        assert np.array_equal(s, np.tile(np.float32(1) / np.arange(2, 12).astype(np.float32), (nq, 1)))


def test_striped_engine_returns_the_same_keys(engine, pkg, exact):
    """vs_open_multi with two shards on device 0 (row-striped): the global
    candidate search, then the fusion on the first device. Not refused."""
    c = exact["b768"]
    with pkg.VectorEngine(shards=[0, 0]) as eng2:
        eng2.create_collection("fuse_striped", 768, pkg.METRIC_DOT, pkg.DTYPE_BF16)
        eng2.upsert("fuse_striped", np.arange(c.X.shape[0]), c.X)
        for nq, n_sub, F, k in ((1, 2, 8, 5), (4, 3, 64, 10), (32, 8, 128, 128)):
            res = eng2.search_fused("fuse_striped", c.Q[:nq, :n_sub], k, F)
            one = engine.search_fused(c.name, c.Q[:nq, :n_sub], k, F)
            for a, b in zip(res, one):
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b)
            _assert_fused(res, c.lists(nq, n_sub, F), k, what=("striped", nq, n_sub, F, k))
        allow = np.random.default_rng(6).random(c.X.shape[0]) < 0.5
        fid = eng2.filter_create("fuse_striped", allow)
        _assert_fused(eng2.search_fused("fuse_striped", c.Q[:4, :3], 10, 64, filter_id=fid),
                      c.lists(4, 3, 64, allow), 10, what="striped filter")


def test_fused_keys_feed_mmr_keys(engine, exact):
    """A fused list is sorted descending: vs_mmr_keys at diversity 0 returns its
    first k unchanged."""
    import torch
    c = exact["b768"]
    nq, n_sub, F = 4, 3, 64
    st = torch.cuda.current_stream().cuda_stream
    d_q = torch.from_numpy(np.ascontiguousarray(c.Q[:nq, :n_sub])).cuda()
    d_lists = torch.zeros((nq, n_sub, F), dtype=torch.int64, device="cuda")
    d_fused = torch.zeros((nq, 32), dtype=torch.int64, device="cuda")
    d_out = torch.full((nq, 10), -1, dtype=torch.int64, device="cuda")
    engine.search_keys(c.name, d_q.data_ptr(), nq * n_sub, 768, F, d_lists.data_ptr(), st)
    engine.fuse_keys(d_lists.data_ptr(), nq, n_sub, F, 32, FR.RRF, 0, d_fused.data_ptr(), st)
    engine.mmr_keys(c.name, d_fused.data_ptr(), nq, 32, 10, 0.0, d_out.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(d_lists.cpu().numpy().view(np.uint64), c.lists(nq, n_sub, F))
    assert torch.equal(d_out, d_fused[:, :10]) and bool((d_out != 0).all())
    want = np.stack([FR.rrf(l, 32) for l in c.lists(nq, n_sub, F)])
    assert np.array_equal(d_fused.cpu().numpy().view(np.uint64), want)


def test_search_fused_errors(engine, pkg, exact):
    c = exact["b768"]
    inv = pkg.engine.VS_ERR_INVALID_ARG

    def bad(code, word, q, *a, name="fuse_nope"):
        with pytest.raises(pkg.VSError) as e:
            engine.search_fused(name, q, *a)
        assert e.value.code == code and word in e.value.msg, (a, e.value.code, e.value.msg)

    q = c.Q[:2, :3]
    # argument errors come before the collection is looked at (it does not exist)
    bad(inv, "n_sub", np.zeros((2, 0, 768), np.float32), 4)
    bad(inv, "n_sub", np.zeros((1, 9, 768), np.float32), 4)
    bad(inv, "k must", q, 0)
    bad(inv, "k 129", q, 129)
    bad(inv, "prefetch_limit", q, 10, 129)
    bad(inv, "prefetch_limit", q, 20, 10)
    bad(inv, "fusion", q, 4, 16, 2)
    bad(inv, "rrf_k", q, 4, 16, pkg.FUSION_RRF, 65537)
    bad(inv, "rrf_k", q, 4, 16, pkg.FUSION_DBSF, 2)
    bad(pkg.engine.VS_ERR_NOT_FOUND, "not found", q, 4, 16)
    bad(pkg.engine.VS_ERR_DIM_MISMATCH, "dimension", q[:, :, :100], 4, 16, name=c.name)
    bad(pkg.engine.VS_ERR_NOT_FOUND, "filter", q, 4, 16, 0, 0, 987654, name=c.name)
    # nq = 0 is nothing to do
    s, r, cnt = engine.search_fused(c.name, np.zeros((0, 3, 768), np.float32), 4)
    assert s.shape == (0, 4) and cnt.shape == (0,)
