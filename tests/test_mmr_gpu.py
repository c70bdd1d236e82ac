"""MMR search (vs_search_mmr / vs_mmr_keys, include/vsearch.h "MMR search").

The reference is the header's rule restated in numpy (``_mmr_ref``), in
float64. Two kinds of data:

* exact arithmetic: DOT collections whose entries lie in {-1, 0, 1}/8 and
  queries that are rows of the same kind. Every dot product is a multiple of
  2^-6 below 2^4 (dim <= 768: |dot| <= 12), so an fp32 sum is exact in any
  order, and (1 - d) s - d p is exact for d in {0, .25, .5, .75, 1}. The device
  must then return the reference's selection EXACTLY, ties included. The
  fixture has near-duplicates (rows = one of 40 centres with 15% of the
  entries redrawn) and 50 exact copies, so ties and diversity both bite:
  ``test_fixture_is_not_vacuous`` asserts that every query of the three
  flagship shapes departs from the plain top-k and meets an exact tie.
* real data (COSINE, unit Gaussian and clustered rows): products are rounded,
  so equality with a float64 greedy run cannot be asked (most queries have a
  step whose margin is under the rounding error). Instead the engine's own
  selection sequence is replayed in float64 and must be greedy within
  tau = 2 D 2^-24 at every step: products of unit-norm rows accumulated in
  fp32 are off by at most D 2^-24 sum|a_i b_i| <= D 2^-24, for s and for sim
  alike, so each v is off by at most D 2^-24 and a comparison of two by twice
  that.

There is no call site in the reference (rag/vector-service/main.go:249-254
searches without a rerank); the need comes from its ingest's overlapping
chunks (rag/ingest-service/main.go:293-323).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT_D = (0.0, 0.25, 0.5, 0.75, 1.0)


# ---- the rule, in numpy ------------------------------------------------------
def _keys_encode(scores, rows):
    """vs_key_encode over arrays (include/vsearch.h "Result key layout")."""
    s = np.asarray(scores, np.float32).copy()
    s[s == 0] = 0.0
    u = s.view(np.uint32)
    o = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return (o.astype(np.uint64) << np.uint64(32)) | (
        np.uint64(0xFFFFFFFF) - np.asarray(rows, np.uint64))


def _top_f(S, F, row_base=0, allow=None):
    """Exact top-F of every query of S [nq][rows] (float64): (scores, rows), in
    search order (score desc, row asc); fewer when fewer rows are allowed."""
    out = []
    rows = np.arange(S.shape[1])
    for s in S:
        idx = rows if allow is None else rows[allow]
        order = idx[np.lexsort((idx, -s[idx]))][:F]
        out.append((s[order], order + row_base))
    return out


def _mmr_ref(s, G, k, d):
    """Selection order (candidate indices) by the header's rule, in float64;
    also whether some step met an exact tie between its two best."""
    F = len(s)
    a, d = float(np.float32(1) - np.float32(d)), float(np.float32(d))
    if F == 0:
        return [], False
    sel, free, pen, tie = [0], np.ones(F, bool), G[0].astype(np.float64).copy(), False
    free[0] = False
    for _ in range(1, min(k, F)):
        v = np.where(free, a * s - d * pen, -np.inf)
        i = int(np.argmax(v))  # the first maximum: ties go to the lower index
        tie |= int(np.sum(v == v[i])) > 1
        sel.append(i)
        free[i] = False
        pen = np.maximum(pen, G[i])
    return sel, tie


def _ref_rows(X, row_base, cands, k, d):
    """Per query: (rows, scores) selected from its (scores, global rows) candidates."""
    out, ties = [], []
    for s, r in cands:
        Xc = X[(r - row_base).astype(np.int64)].astype(np.float64)
        sel, tie = _mmr_ref(s.astype(np.float64), Xc @ Xc.T, k, d)
        out.append((r[sel], s[sel]))
        ties.append(tie)
    return out, ties


# ---- exact-arithmetic fixture --------------------------------------------------
def _ternary(n, dim, seed):
    rng = np.random.default_rng(seed)
    C = rng.integers(-1, 2, (40, dim)).astype(np.float32)
    X = C[np.arange(n) % 40].copy()
    redraw = rng.random((n, dim)) < 0.15
    X[redraw] = rng.integers(-1, 2, int(redraw.sum())).astype(np.float32)
    m = min(50, n // 2)
    dst = rng.choice(n, m, replace=False)
    src = (dst + 40 * rng.integers(1, 5, m)) % n   # exact copies (of the same centre's rows)
    X[dst] = X[src]
    return X / 8, C[:32] / 8


class _Coll:
    def __init__(self, eng, pkg, name, n, dim, bf16, seed, row_base=0):
        self.name, self.bf16, self.row_base = name, bf16, row_base
        self.X, self.Q = _ternary(n, dim, seed)
        eng.create_collection(name, dim, pkg.METRIC_DOT, pkg.DTYPE_BF16 if bf16 else pkg.DTYPE_F32,
                              0, row_base)
        eng.upsert(name, np.arange(n), self.X)
        self.S = self.Q.astype(np.float64) @ self.X.astype(np.float64).T


@pytest.fixture(scope="module")
def exact(engine, pkg):
    colls = {}
    for bf16 in (True, False):
        t = "b" if bf16 else "f"
        colls[bf16, 768] = _Coll(engine, pkg, f"mmr_{t}768", 3000, 768, bf16, 11)
        colls[bf16, 100] = _Coll(engine, pkg, f"mmr_{t}100", 1000, 100, bf16, 12, row_base=1000)
    colls["96"] = _Coll(engine, pkg, "mmr_b96", 1000, 96, True, 13)
    yield colls
    for c in colls.values():
        engine.drop_collection(c.name)


def _assert_same(res, want, k, what):
    s, r, c = res
    for q, (wr, ws) in enumerate(want):
        n = len(wr)
        assert c[q] == n, (what, q, c[q], n)
        assert np.array_equal(r[q, :n], wr.astype(np.uint64)), (what, q, r[q, :n], wr)
        assert np.array_equal(s[q, :n].view(np.uint32), ws.astype(np.float32).view(np.uint32)), (what, q)
        assert not r[q, n:].any() and not s[q, n:].any(), (what, q)


def test_fixture_is_not_vacuous(exact):
    """At the flagship shapes every query departs from the plain top-k and meets
    an exact tie at some step (so the tie rule and the penalty are both tested)."""
    for key, F, k, d in (((True, 768), 64, 10, 0.5), ((True, 768), 128, 16, 0.25),
                         ("96", 33, 33, 0.75)):
        c = exact[key]
        cands = _top_f(c.S, F)
        want, ties = _ref_rows(c.X, 0, cands, k, d)
        assert all(ties), (key, F, k, d, ties)
        assert all(not np.array_equal(w[0], cd[1][:k]) for w, cd in zip(want, cands)), (key, F, k, d)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("dim", [100, 768])
def test_mmr_keys_exact(engine, exact, bf16, dim):
    """The selection stage alone over uploaded candidate lists: every list
    length, k and batch size, lists 0-padded below n_cand, a K tail (dim 100:
    one partial 256-byte chunk), row_base != 0 (dim 100)."""
    import torch
    c = exact[bf16, dim]
    st = torch.cuda.current_stream().cuda_stream
    combo = 0
    for nq in (1, 5, 32):
        for n_cand in (1, 2, 17, 33, 64, 128):
            top = _top_f(c.S[:nq], n_cand, c.row_base)
            for k in sorted({1, min(10, n_cand), n_cand}):
                d = EXACT_D[combo % 5]
                combo += 1
                # every third query's list is short: zero keys from `keep` on
                cands, keys = [], np.zeros((nq, n_cand), np.uint64)
                for q, (s, r) in enumerate(top):
                    keep = n_cand if q % 3 else max(1, n_cand - 1 - q % 5)
                    cands.append((s[:keep], r[:keep]))
                    keys[q, :keep] = _keys_encode(s[:keep], r[:keep])
                want, _ = _ref_rows(c.X, c.row_base, cands, k, d)
                d_in = torch.from_numpy(keys.view(np.int64)).cuda()
                d_out = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
                engine.mmr_keys(c.name, d_in.data_ptr(), nq, n_cand, k, d, d_out.data_ptr(), st)
                torch.cuda.synchronize()
                got = d_out.cpu().numpy().view(np.uint64)
                for q, (wr, ws) in enumerate(want):
                    wk = np.zeros(k, np.uint64)
                    wk[:len(wr)] = _keys_encode(ws, wr)
                    assert np.array_equal(got[q], wk), (bf16, dim, nq, n_cand, k, d, q)


@pytest.mark.parametrize("key,F,k,d", [((True, 768), 64, 10, 0.5), ((True, 768), 128, 16, 0.25),
                                       ("96", 33, 33, 0.75), ((False, 768), 128, 16, 0.75),
                                       ((False, 100), 40, 10, 1.0), ((True, 100), 0, 7, 0.5)])
@pytest.mark.parametrize("nq", [1, 32])
def test_search_mmr_exact(engine, exact, key, F, k, d, nq):
    """Candidate search + selection in one call: one query (GEMV path) and a
    batch (MFMA path); F = 0 is the default min(4 k, 128)."""
    c = exact[key]
    Fe = F or min(4 * k, 128)
    want, _ = _ref_rows(c.X, c.row_base, _top_f(c.S[:nq], Fe, c.row_base), k, d)
    _assert_same(engine.search_mmr(c.name, c.Q[:nq], k, F, d), want, k, (key, F, k, d, nq))


@pytest.mark.parametrize("nq", [1, 32])
def test_search_mmr_resident_filter(engine, exact, nq):
    c = exact[True, 768]
    allow = np.random.default_rng(5).random(c.X.shape[0]) < 0.4
    fid = engine.filter_create(c.name, allow)
    try:
        want, _ = _ref_rows(c.X, 0, _top_f(c.S[:nq], 64, 0, allow), 12, 0.5)
        _assert_same(engine.search_mmr(c.name, c.Q[:nq], 12, 64, 0.5, fid), want, 12, nq)
        # a filter that allows fewer than k rows: out_count = allowed rows
        few = np.zeros(c.X.shape[0], bool)
        few[[5, 45, 2999]] = True
        fid2 = engine.filter_create(c.name, few)
        try:
            want, _ = _ref_rows(c.X, 0, _top_f(c.S[:nq], 32, 0, few), 8, 0.75)
            res = engine.search_mmr(c.name, c.Q[:nq], 8, 32, 0.75, fid2)
            assert np.all(res[2] == 3)
            _assert_same(res, want, 8, "few")
        finally:
            engine.filter_drop(fid2)
    finally:
        engine.filter_drop(fid)


def test_search_mmr_after_delete(engine, pkg):
    """A vs_delete moves tail rows into the holes: candidates are then read from
    their new places. The reference runs on the compacted matrix."""
    X, Q = _ternary(1500, 768, 21)
    engine.create_collection("mmr_del", 768, pkg.METRIC_DOT, pkg.DTYPE_BF16)
    try:
        engine.upsert("mmr_del", np.arange(1500), X)
        S = Q.astype(np.float64) @ X.astype(np.float64).T
        # delete the best candidates of query 0 below the new row count, so tail rows
        # (candidates of other queries among them) move into the holes
        gone = np.unique(np.concatenate([_top_f(S[:1], 40)[0][1][::2], np.arange(1200, 1210)]))
        frm, to = engine.delete("mmr_del", gone)
        assert len(frm) > 0
        Y = X.copy()
        Y[to.astype(np.int64)] = X[frm.astype(np.int64)]
        Y = Y[:1500 - len(gone)]
        assert np.array_equal(engine.read_rows("mmr_del", 0, len(Y)), Y)
        S = Q.astype(np.float64) @ Y.astype(np.float64).T
        for nq in (1, 32):
            cands = _top_f(S[:nq], 64)
            moved = set(int(t) for t in to)
            assert any(moved & set(int(r) for r in cd[1]) for cd in cands)
            want, _ = _ref_rows(Y, 0, cands, 10, 0.5)
            _assert_same(engine.search_mmr("mmr_del", Q[:nq], 10, 64, 0.5), want, 10, nq)
    finally:
        engine.drop_collection("mmr_del")


def test_placed_collection(pkg):
    """VS_FLAG_PLACE_COLLECTIONS with one device engine per entry of {0, 0}: the
    second collection lands on the second slot, whose calls take the home
    device's route (and vs_mmr_keys the cross-device copy)."""
    import torch
    X, Q = _ternary(1200, 768, 31)
    S = Q.astype(np.float64) @ X.astype(np.float64).T
    with pkg.VectorEngine(shards=[0, 0], place_collections=True, engine_per_shard=True) as eng:
        for name in ("p0", "p1"):
            eng.create_collection(name, 768, pkg.METRIC_DOT, pkg.DTYPE_BF16, 1200)
            eng.upsert(name, np.arange(1200), X)
        cands = _top_f(S, 64)
        want, _ = _ref_rows(X, 0, cands, 10, 0.5)
        keys = np.stack([_keys_encode(s, r) for s, r in cands])
        for name in ("p0", "p1"):
            _assert_same(eng.search_mmr(name, Q, 10, 64, 0.5), want, 10, name)
            _assert_same(eng.search_mmr(name, Q[:1], 10, 64, 0.5), want[:1], 10, name)
            d_in = torch.from_numpy(keys.view(np.int64)).cuda()
            d_out = torch.zeros((32, 10), dtype=torch.int64, device="cuda")
            eng.mmr_keys(name, d_in.data_ptr(), 32, 64, 10, 0.5, d_out.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy().view(np.uint64)
            assert np.array_equal(got, np.stack([_keys_encode(ws, wr) for wr, ws in want])), name


# ---- identities -----------------------------------------------------------------
@pytest.fixture(scope="module")
def real(engine, pkg, orc):
    """COSINE collections of unit Gaussian rows and of 64 clusters with noise 0.35."""
    colls = {}
    for n, dim in ((4096, 768), (2048, 1024)):
        for kind in ("gauss", "clust"):
            rng = np.random.default_rng(dim + len(kind))
            if kind == "gauss":
                X = rng.standard_normal((n, dim)).astype(np.float32)
                Q = rng.standard_normal((64, dim)).astype(np.float32)
            else:
                C = rng.standard_normal((64, dim)).astype(np.float32)
                C /= np.linalg.norm(C, axis=1, keepdims=True)
                X = (C[rng.integers(0, 64, n)] +
                     0.35 * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim))
                Q = (C + 0.35 * rng.standard_normal((64, dim)).astype(np.float32) / np.sqrt(dim))
            X, Q = X.astype(np.float32), Q.astype(np.float32)
            for bf16 in (True, False):
                name = f"mmr_real_{kind}_{dim}_{int(bf16)}"
                engine.create_collection(name, dim, pkg.METRIC_COSINE,
                                         pkg.DTYPE_BF16 if bf16 else pkg.DTYPE_F32)
                engine.upsert(name, np.arange(n), X)
                stored = engine.read_rows(name, 0, n).astype(np.float64)
                colls[kind, dim, bf16] = (name, stored, orc.preprocess(Q, True, bf16).astype(np.float64), Q)
    yield colls
    for name, *_ in colls.values():
        engine.drop_collection(name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("nq", [1, 64])
def test_identities(engine, real, nq):
    for (kind, dim, bf16), (name, X, Qp, Q) in real.items():
        q = Q[:nq]
        plain = engine.search(name, q, 16)
        zero = engine.search_mmr(name, q, 16, 128, 0.0)
        # d = 0: the first k of plain search, bit for bit
        assert np.array_equal(_bits(plain[0]), _bits(zero[0])), (name, nq)
        assert np.array_equal(plain[1], zero[1]) and np.array_equal(plain[2], zero[2]), (name, nq)
        full = engine.search(name, q, 48)
        allk = engine.search_mmr(name, q, 48, 48, 0.5)   # k == F: the same set
        assert np.array_equal(np.sort(full[1], axis=1), np.sort(allk[1], axis=1)), (name, nq)
        assert np.array_equal(full[2], allk[2])
        some = engine.search_mmr(name, q, 16, 128, 0.5)
        assert np.array_equal(some[1][:, 0], plain[1][:, 0])   # the first is plain search's first
        # ... with the score of the candidate search (k = F), as every result
        wide = engine.search(name, q, 128)
        assert np.array_equal(_bits(some[0][:, 0]), _bits(wide[0][:, 0]))
        # the selection stage itself at d = 0: the first k keys of every list
        import torch
        d_q = torch.from_numpy(q).cuda()
        d_keys = torch.zeros((nq, 128), dtype=torch.int64, device="cuda")
        d_out = torch.zeros((nq, 16), dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        engine.search_keys(name, d_q.data_ptr(), nq, dim, 128, d_keys.data_ptr(), st)
        engine.mmr_keys(name, d_keys.data_ptr(), nq, 128, 16, 0.0, d_out.data_ptr(), st)
        torch.cuda.synchronize()
        assert torch.equal(d_out, d_keys[:, :16]) and bool((d_out != 0).all()), (name, nq)


def test_count_with_fewer_rows_than_candidates(engine, pkg):
    X, Q = _ternary(20, 768, 41)
    for dtype in (pkg.DTYPE_BF16, pkg.DTYPE_F32):
        engine.create_collection("mmr_small", 768, pkg.METRIC_DOT, dtype)
        try:
            for nq in (1, 32):   # an empty collection answers with counts of 0
                s, r, c = engine.search_mmr("mmr_small", Q[:nq], 30, 64, 0.5)
                assert not c.any() and not r.any() and not s.any()
            engine.upsert("mmr_small", np.arange(20), X)
            S = Q.astype(np.float64) @ X.astype(np.float64).T
            for nq in (1, 32):
                want, _ = _ref_rows(X, 0, _top_f(S[:nq], 64), 30, 0.5)
                res = engine.search_mmr("mmr_small", Q[:nq], 30, 64, 0.5)
                assert np.all(res[2] == 20)
                _assert_same(res, want, 30, (dtype, nq))
        finally:
            engine.drop_collection("mmr_small")


# ---- real data: greedy within the rounding error ----------------------------------
@pytest.mark.parametrize("d", [0.3, 0.5])
def test_real_data_is_greedy_within_rounding(engine, real, d):
    F, k = 128, 16
    a64, d64 = float(np.float32(1) - np.float32(d)), float(np.float32(d))
    for (kind, dim, bf16), (name, X, Qp, Q) in real.items():
        tau = 2 * dim * 2.0 ** -24
        s_dev, r_dev, c_dev = engine.search_mmr(name, Q, k, F, d)
        _, r_cand, c_cand = engine.search(name, Q, F)   # c_0 .. c_{F-1} by definition
        assert np.all(c_dev == k) and np.all(c_cand == F)
        S = Qp @ X.T
        worst = 0.0
        for q in range(Q.shape[0]):
            cand = r_cand[q].astype(np.int64)
            pos = {int(r): i for i, r in enumerate(cand)}
            sel = [pos[int(r)] for r in r_dev[q]]   # KeyError: a row outside the candidates
            assert len(set(sel)) == k and sel[0] == 0, (name, q)
            s = S[q, cand]
            G = X[cand] @ X[cand].T
            # every selected row is among the F best in float64, and carries its score
            fth = np.sort(S[q])[-F]
            assert np.all(s[sel] >= fth - tau), (name, q)
            assert np.all(np.abs(s_dev[q] - s[sel]) <= 1e-5 * np.abs(s[sel]) + 1e-6), (name, q)
            free = np.ones(F, bool)
            free[0] = False
            pen = G[0].copy()
            for i in sel[1:]:
                v = a64 * s - d64 * pen
                gap = float(np.max(v[free]) - v[i])
                worst = max(worst, gap)
                assert gap <= tau, (name, q, i, gap, tau)
                free[i] = False
                pen = np.maximum(pen, G[i])
        print(f"{name} d={d}: worst step gap {worst:.3e} (tau {tau:.3e})")


# ---- errors ---------------------------------------------------------------------
def test_errors(engine, pkg, exact):
    c = exact[True, 768]
    q = c.Q[:2]

    def bad(code, word, *a, eng=engine, name=c.name, qq=q):
        with pytest.raises(pkg.VSError) as e:
            eng.search_mmr(name, qq, *a)
        assert e.value.code == code and word in e.value.msg, (a, e.value.code, e.value.msg)

    inv = pkg.engine.VS_ERR_INVALID_ARG
    bad(inv, "candidates_limit", 20, 10, 0.5)          # k > candidates_limit
    bad(inv, "candidates_limit", 10, 129, 0.5)         # candidates_limit > 128
    bad(inv, "k must", 0, 16, 0.5)                     # k = 0
    bad(inv, "k ", 129, 0, 0.5)                        # k beyond the largest default
    for d in (-0.01, 1.01, float("nan"), float("inf")):
        bad(inv, "diversity", 10, 64, d)
    bad(pkg.engine.VS_ERR_NOT_FOUND, "not found", 10, 64, 0.5, name="mmr_nope")
    bad(pkg.engine.VS_ERR_DIM_MISMATCH, "dimension", 10, 64, 0.5, qq=q[:, :100])
    # the device-pointer form checks the same arguments before it touches a pointer
    for a in ((1, 10, 20, 0.5), (1, 129, 10, 0.5), (1, 0, 1, 0.5), (1, 16, 0, 0.5),
              (1, 16, 4, 2.0), (1, 16, 4, float("nan"))):
        with pytest.raises(pkg.VSError) as e:
            engine.mmr_keys(c.name, 0, *a, 0)
        assert e.value.code == inv, a
    # a row-striped engine keeps candidate rows on several shards: refused, and said so
    with pkg.VectorEngine(shards=[0, 0]) as eng2:
        eng2.create_collection("striped", 768, pkg.METRIC_DOT, pkg.DTYPE_BF16)
        eng2.upsert("striped", np.arange(64), c.X[:64])
        bad(inv, "row-striped", 4, 16, 0.5, eng=eng2, name="striped")
        with pytest.raises(pkg.VSError) as e:
            eng2.mmr_keys("striped", 8, 1, 16, 4, 0.5, 8)
        assert e.value.code == inv and "row-striped" in e.value.msg
        assert eng2.search("striped", q, 4)[2].tolist() == [4, 4]   # plain search still serves it
    # rows that are not whole 8-byte words
    engine.create_collection("mmr_odd", 33, pkg.METRIC_DOT, pkg.DTYPE_BF16)
    try:
        engine.upsert("mmr_odd", np.arange(8), np.ones((8, 33), np.float32))
        bad(inv, "8-byte", 2, 4, 0.5, name="mmr_odd", qq=np.ones((1, 33), np.float32))
    finally:
        engine.drop_collection("mmr_odd")
