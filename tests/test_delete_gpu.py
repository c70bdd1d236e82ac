"""Point deletion (vs_delete, include/vsearch.h): the compaction rule, the
stored bits, and every search path on the compacted collection.

Expected rows come from numpy: the H/T rule of the header applied to the
matrix the test stored (``_rule`` / ``_compact`` below restate the header, not
the device code). Searches are then held to the oracle on that matrix under
the project's parity bar (oracle.check_topk at 1e-5), and to a
second collection restored from the post-delete snapshot, whose int8 copy is
built from scratch: the two must return identical keys, which pins the
incrementally requantised copy to a fresh one.

All collections use the DOT metric (no preprocessing), so stored bits are the
uploaded / generated ones. Points.Delete has no call site in the reference;
the anchors are the store and search calls it must leave intact
(rag/vector-service/main.go:209, :249-254).
"""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- the rule, in numpy ------------------------------------------------------
def _rule(n, rows):
    """(N', moved_from T, moved_to H) of include/vsearch.h vs_delete."""
    s = set(int(r) for r in rows)
    nn = n - len(s)
    holes = sorted(r for r in s if r < nn)
    surv = [r for r in range(nn, n) if r not in s]
    assert len(holes) == len(surv)
    return nn, np.array(surv, np.uint64), np.array(holes, np.uint64)


def _compact(X, rows):
    nn, frm, to = _rule(X.shape[0], rows)
    Y = X.copy()
    Y[to.astype(np.int64)] = X[frm.astype(np.int64)]
    return Y[:nn].copy(), frm, to


def _raw(X, bf16):
    X = np.ascontiguousarray(X, np.float32)
    return (X.view(np.uint32) >> 16).astype("<u2").tobytes() if bf16 else X.tobytes()


def _delete_set(rng, n, count):
    """Rows below and above N', a repeat, and the last row."""
    body = rng.choice(n - 1, count - 1, replace=False)
    tail = np.arange(n - count // 3, n - 1)[::2]  # some of the rows that would move
    d = np.concatenate([body, tail, [n - 1, body[0]]]).astype(np.uint64)
    rng.shuffle(d)
    return d


def _same_keys(a, b):
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and
            np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


def _check(orc, eng, name, X, Q, k, bf16, twin=None, twin_eng=None):
    res = eng.search(name, Q, k)
    s, r, c = res
    Qp = orc.preprocess(Q, False, bf16)
    _, s64, rr, cc = orc.search(X, Qp, k)
    bad = orc.check_topk(s, r, c, s64, rr, cc, orc.rescore(X, Qp, r, c), score_rtol=1e-5)
    assert not bad, (name, k, bad[:6])
    valid = np.arange(k)[None, :] < c[:, None]
    assert np.all(r[valid] < X.shape[0])
    if twin:
        assert _same_keys(res, (twin_eng or eng).search(twin, Q, k)), (name, twin, k)
    return res


# ---- rule and bits -----------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", [(0, 100), (1, 128), (1, 100), (1, 33)])
def test_rule_and_bits(engine, orc, tmp_path, dtype, dim):
    """fp32 dim 100 and bf16 dim 128 (16-byte moves), bf16 dim 100 (4-byte
    moves) and bf16 dim 33 (2-byte moves)."""
    n, bf16 = 1000, bool(dtype)
    name = f"dl_rb{dtype}_{dim}"
    rng = np.random.default_rng(dim + dtype)
    X = (rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(np.float32)  # ~unit rows
    if bf16:
        X = orc.np_bf16_round(X)
    d = _delete_set(rng, n, 90)
    want, frm, to = _compact(X, d)
    assert len(frm) > 10 and want.shape[0] == n - len(set(d.tolist())) < n - 80
    engine.create_collection(name, dim, 1, dtype)
    try:
        engine.upsert(name, np.arange(n), X)
        gf, gt = engine.delete(name, d)
        assert np.array_equal(gf, frm) and np.array_equal(gt, to)
        nn = want.shape[0]
        assert engine.collection_info(name)["rows"] == nn
        got = engine.read_rows(name, 0, nn)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert engine.checksum(name) == orc.checksum(_raw(want, bf16))
        path = str(tmp_path / "d.vsnap")
        engine.snapshot(name, path)
        engine.restore(name + "_r", path)
        try:
            back = engine.read_rows(name + "_r", 0, nn)
            assert engine.collection_info(name + "_r")["rows"] == nn
            assert np.array_equal(back.view(np.uint32), want.view(np.uint32))
        finally:
            engine.drop_collection(name + "_r")
        Q = rng.standard_normal((3, dim)).astype(np.float32)
        _check(orc, engine, name, want, Q[:1], 10, bf16)
        _check(orc, engine, name, want, Q, 7, bf16)
    finally:
        engine.drop_collection(name)


# ---- every search path after a delete -----------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("n,ndel,cases", [
    (300, 60, [(1, 10)]),                      # small path: <= 256 rows, one query
    (1000, 90, [(1, 10), (1, 200), (3, 200)]),  # one-query GEMV; k > 128
    (4000, 300, [(64, 10), (64, 16), (2, 1500)]),  # MFMA list pass; k > 1024 at a small N
])
def test_search_paths_small(engine, orc, tmp_path, dtype, n, ndel, cases):
    dim, bf16 = 128, bool(dtype)
    name = f"dl_sp{dtype}_{n}"
    rng = np.random.default_rng(n + dtype)
    engine.create_collection(name, dim, 1, dtype)
    try:
        engine.generate(name, n, 4242)
        X = orc.generate(4242, 0, n, dim, bf16=bf16)
        d = _delete_set(rng, n, ndel)
        want, frm, to = _compact(X, d)
        gf, gt = engine.delete(name, d)
        assert np.array_equal(gf, frm) and np.array_equal(gt, to)
        if n == 300:
            assert want.shape[0] <= 256
        path = str(tmp_path / "p.vsnap")
        engine.snapshot(name, path)
        engine.restore(name + "_r", path)
        try:
            Q = orc.generate(orc.SEED_QUERY, 0, 64, dim)
            for nq, k in cases:
                _check(orc, engine, name, want, Q[:nq], k, bf16, twin=name + "_r")
        finally:
            engine.drop_collection(name + "_r")
    finally:
        engine.drop_collection(name)


# ---- the int8 paths: ~70k x 768, candidate pass + prefilter --------------------
BIG_N, BIG_DIM, BIG_SEED = 70_000, 768, 9001


class _Big:
    pass


@pytest.fixture(scope="module")
def big(pkg, orc, tmp_path_factory):
    """One 70k x 768 bf16 collection deleted from once, on a default engine
    (int8 copy, speculative bound), an engine without speculation and one
    without the int8 copy; the post-delete snapshot restored beside the first;
    the numpy expectation. Shared, and left unchanged, by the tests below."""
    b = _Big()
    b.X0 = orc.generate(BIG_SEED, 0, BIG_N, BIG_DIM, bf16=True)
    rng = np.random.default_rng(5)
    b.d = _delete_set(rng, BIG_N, 700)
    b.X, b.frm, b.to = _compact(b.X0, b.d)
    b.engs = {"spec": pkg.VectorEngine(device=0),
              "nospec": pkg.VectorEngine(device=0, speculative=False),
              "bf16": pkg.VectorEngine(device=0, prefilter=False)}
    for key, e in b.engs.items():
        e.create_collection("big", BIG_DIM, 1, 1, BIG_N)
        e.generate("big", BIG_N, BIG_SEED)
    Q = orc.generate(orc.SEED_QUERY, 0, 256, BIG_DIM)
    b.Q = Q
    spec = b.engs["spec"]
    assert spec.prefilter_bytes("big") > 0 and b.engs["bf16"].prefilter_bytes("big") == 0
    for _ in range(3):  # the speculative bound learns its ratio and runs
        spec.search("big", Q, 10)
    b.tries_before = spec.spec_stats("big")["tries"]
    for key, e in b.engs.items():
        gf, gt = e.delete("big", b.d)
        assert np.array_equal(gf, b.frm) and np.array_equal(gt, b.to), key
    path = str(tmp_path_factory.mktemp("dl") / "big.vsnap")
    spec.snapshot("big", path)
    spec.restore("big_r", path)
    yield b
    for e in b.engs.values():
        e.close()


def test_speculation_survives_delete(big):
    """(d) three consecutive batches after the delete on the speculating engine
    equal the non-speculating engine's keys; the int8 copy is still there and
    speculative tries resume (counted inside this test: it does not depend on
    which test touches the shared collection first)."""
    spec, nospec = big.engs["spec"], big.engs["nospec"]
    assert spec.collection_info("big")["rows"] == big.X.shape[0]
    assert big.tries_before > 0  # the bound ran before the delete (fixture)
    st0 = spec.spec_stats("big")
    for i in range(3):
        a = spec.search("big", big.Q, 10)
        assert _same_keys(a, nospec.search("big", big.Q, 10)), i
    assert spec.prefilter_bytes("big") > 0
    assert spec.spec_stats("big")["tries"] > st0["tries"]


@pytest.mark.parametrize("nq,k", [(256, 10), (64, 50), (1, 10), (1, 100), (2, 200)])
def test_search_paths_int8(big, orc, nq, k):
    """Candidate pass + int8 prefilter (batches), the one-query int8 scan, and
    k > 128, against the oracle, the freshly built copy and the bf16 pass."""
    spec = big.engs["spec"]
    res = _check(orc, spec, "big", big.X, big.Q[:nq], k, True, twin="big_r")
    assert _same_keys(res, big.engs["bf16"].search("big", big.Q[:nq], k))


def test_deleted_and_moved_rows_as_queries(big, orc):
    """(a) a deleted row's vector does not find that row, and nothing at or past
    N' is returned; (b) a moved row's vector finds it at its NEW number, on the
    batched int8 path, the one-query int8 path and an engine without the
    int8 copy, with equal keys."""
    spec, plain = big.engs["spec"], big.engs["bf16"]
    nn = big.X.shape[0]
    gone = np.array(sorted(set(big.d.tolist()))[:40] + [BIG_N - 1], np.int64)
    moved = big.frm[:64].astype(np.int64)
    Q = np.concatenate([big.X0[gone], big.X0[moved]])
    res = _check(orc, spec, "big", big.X, Q, 10, True, twin="big_r")
    assert _same_keys(res, plain.search("big", Q, 10))
    assert np.all(res[1] < nn)
    # generated unit rows: a row's own score (~1) is far above any other's
    assert np.array_equal(res[1][len(gone):, 0], big.to[:64])
    assert np.all(res[0][:len(gone), 0] < 0.9)
    for i in (0, 5):
        one = spec.search("big", big.X0[moved[i]:moved[i] + 1], 10)
        assert int(one[1][0, 0]) == int(big.to[i])
        assert _same_keys(one, spec.search("big_r", big.X0[moved[i]:moved[i] + 1], 10))
        assert _same_keys(one, plain.search("big", big.X0[moved[i]:moved[i] + 1], 10))


def test_filtered_search_on_the_new_numbering(big, orc):
    spec = big.engs["spec"]
    nn = big.X.shape[0]
    mask = np.random.default_rng(3).random(nn) < 0.3
    idx = np.flatnonzero(mask)
    Q = big.Q[:16]
    s, r, c = spec.search_filtered("big", Q, 10, mask)
    Qp = orc.preprocess(Q, False, True)
    _, s64, rl, cc = orc.search(big.X[idx], Qp, 10)
    pos = np.searchsorted(idx, r.astype(np.int64)).astype(np.uint64)
    assert np.all(mask[r.astype(np.int64)])
    bad = orc.check_topk(s, r, c, s64, idx[rl.astype(np.int64)].astype(np.uint64), cc,
                         orc.rescore(big.X[idx], Qp, pos, c), score_rtol=1e-5)
    assert not bad, bad[:6]


def test_partial_tail_tile_then_append(pkg, orc):
    """(c) the last rows of a partial tail tile are deleted and queried, then j
    rows are appended at [N', N' + j) and found. On a collection with an int8
    copy, against an engine without one."""
    n, dim, j = 65_536 + 32 * 40 + 13, 768, 21  # the tail tile holds 13 rows
    X0 = orc.generate(31, 0, n, dim, bf16=True)
    d = np.arange(n - 9, n, dtype=np.uint64)  # 9 of those 13
    want, frm, to = _compact(X0, d)
    assert len(frm) == 0 and want.shape[0] == n - 9
    new = orc.generate(32, 0, j, dim, bf16=True)
    with pkg.VectorEngine(device=0) as a, pkg.VectorEngine(device=0, prefilter=False) as b:
        for e in (a, b):
            e.create_collection("t", dim, 1, 1, n + j)
            e.generate("t", n, 31)
        assert a.prefilter_bytes("t") > 0
        for e in (a, b):
            gf, gt = e.delete("t", d)
            assert len(gf) == 0 and len(gt) == 0
        Q = np.concatenate([X0[n - 9:], X0[n - 13:n - 9], orc.generate(orc.SEED_QUERY, 0, 19, dim)])
        res = _check(orc, a, "t", want, Q, 10, True)
        assert _same_keys(res, b.search("t", Q, 10))
        assert np.array_equal(res[1][9:13, 0], np.arange(n - 13, n - 9, dtype=np.uint64))
        one = a.search("t", Q[:1], 10)  # a deleted row, on the one-query int8 path
        assert _same_keys(one, b.search("t", Q[:1], 10)) and np.all(one[1] < n - 9)
        with pytest.raises(pkg.VSError):  # the append rule applies to the new count
            a.upsert("t", np.arange(n, n + j), new)
        for e in (a, b):
            e.upsert("t", np.arange(n - 9, n - 9 + j), new)
        full = np.concatenate([want, new])
        Q2 = np.concatenate([new, Q[:11]])
        res = _check(orc, a, "t", full, Q2, 10, True)
        assert _same_keys(res, b.search("t", Q2, 10))
        assert np.array_equal(res[1][:j, 0], np.arange(n - 9, n - 9 + j, dtype=np.uint64))
        assert a.prefilter_bytes("t") > 0


def test_shrinking_under_the_int8_size(pkg, orc):
    """A delete that takes a 768-d bf16 collection under the size that keeps an
    int8 copy (8 tiles a workgroup: 57,345 rows at 256 workgroups) drops the
    copy: the store-side writes maintain it only above that size, and the
    one-query int8 scan would go on reading a stale one. Overwrites and appends
    below the size, growing back over it (a new copy) and a delete of every
    row, each held to the oracle and to an engine without the copy, one query
    and batched."""
    n, dim = 66_000, 768
    X0 = orc.generate(41, 0, n, dim, bf16=True)
    rng = np.random.default_rng(41)
    d = rng.choice(n, 16_000, replace=False).astype(np.uint64)
    X, frm, to = _compact(X0, d)
    assert X.shape[0] == 50_000
    Qr = orc.generate(orc.SEED_QUERY, 0, 24, dim)

    def both(a, b, X, own):
        Q = np.concatenate([X[own], Qr])
        res = _check(orc, a, "s", X, Q, 10, True)  # batched
        assert _same_keys(res, b.search("s", Q, 10))
        assert np.array_equal(res[1][:len(own), 0], np.asarray(own, np.uint64))
        for i in (0, len(own) - 1, len(own)):  # one query
            one = _check(orc, a, "s", X, Q[i:i + 1], 10, True)
            assert _same_keys(one, b.search("s", Q[i:i + 1], 10))
            if i < len(own):
                assert int(one[1][0, 0]) == own[i]

    with pkg.VectorEngine(device=0) as a, pkg.VectorEngine(device=0, prefilter=False) as b:
        for e in (a, b):
            e.create_collection("s", dim, 1, 1, n + 4096)
            e.generate("s", n, 41)
        assert a.prefilter_bytes("s") > 0
        a.search("s", Qr, 10)
        for e in (a, b):
            gf, gt = e.delete("s", d)
            assert np.array_equal(gf, frm) and np.array_equal(gt, to)
        assert a.prefilter_bytes("s") == 0
        both(a, b, X, [int(to[0]), int(to[-1]), 49_999])
        # overwrite scattered rows and append, still under the size
        ow = np.unique(rng.integers(0, 50_000, 300)).astype(np.uint64)
        V1 = orc.generate(42, 0, len(ow), dim, bf16=True)
        V2 = orc.generate(43, 0, 2_000, dim, bf16=True)
        for e in (a, b):
            e.upsert("s", ow, V1)
            e.upsert("s", np.arange(50_000, 52_000), V2)
        X = np.concatenate([X, V2])
        X[ow.astype(np.int64)] = V1
        both(a, b, X, [int(ow[0]), int(ow[-1]), 50_000, 51_999])
        # grow back over the size: a copy again, built from the rows as they are
        V3 = orc.generate(44, 0, 8_000, dim, bf16=True)
        for e in (a, b):
            e.upsert("s", np.arange(52_000, 60_000), V3)
        X = np.concatenate([X, V3])
        assert a.prefilter_bytes("s") > 0
        both(a, b, X, [int(ow[0]), 50_000, 52_000, 59_999])
        # delete every row, then ingest again
        for e in (a, b):
            gf, gt = e.delete("s", np.arange(60_000))
            assert len(gf) == 0
        assert a.prefilter_bytes("s") == 0 and a.collection_info("s")["rows"] == 0
        for nq in (1, 16):
            assert np.all(a.search("s", Qr[:nq], 10)[2] == 0)
        for e in (a, b):
            e.upsert("s", np.arange(3_000), V3[:3_000])
        both(a, b, V3[:3_000], [0, 2_999])


# ---- edges ---------------------------------------------------------------------
def test_edges(engine, orc, pkg):
    n, dim = 500, 128
    X = orc.generate(77, 0, n, dim)
    engine.create_collection("dl_e", dim, 1, 0)
    try:
        engine.generate("dl_e", n, 77)
        sum0 = engine.checksum("dl_e")
        gf, gt = engine.delete("dl_e", [])  # n = 0
        assert len(gf) == 0 and len(gt) == 0
        with pytest.raises(pkg.VSError) as ei:  # a row >= N: nothing changes
            engine.delete("dl_e", [3, n, 5])
        assert ei.value.code == -1  # VS_ERR_INVALID_ARG
        assert engine.collection_info("dl_e")["rows"] == n and engine.checksum("dl_e") == sum0
        # a filter made before a delete is refused afterwards, also once appends
        # bring the row count back to the filter's
        fid = engine.filter_create("dl_e", np.ones(n, bool))
        assert engine.search_filter_id("dl_e", X[:1], 3, fid)[2][0] == 3
        engine.delete("dl_e", [0, 1])
        with pytest.raises(pkg.VSError):
            engine.search_filter_id("dl_e", X[:1], 3, fid)
        engine.upsert("dl_e", [n - 2, n - 1], X[:2])
        assert engine.collection_info("dl_e")["rows"] == n
        with pytest.raises(pkg.VSError):
            engine.search_filter_id("dl_e", X[:1], 3, fid)
        fid2 = engine.filter_create("dl_e", np.ones(n, bool))  # a fresh one works
        assert engine.search_filter_id("dl_e", X[:1], 3, fid2)[2][0] == 3
        # delete all, search, append, search
        gf, gt = engine.delete("dl_e", np.arange(n))
        assert len(gf) == 0 and engine.collection_info("dl_e")["rows"] == 0
        for nq in (1, 8):
            s, r, c = engine.search("dl_e", X[:nq], 5)
            assert np.all(c == 0)
        engine.upsert("dl_e", np.arange(40), X[100:140])
        _check(orc, engine, "dl_e", X[100:140], X[100:108], 5, False)
        with pytest.raises(pkg.VSError):
            engine.delete("nope", [0])
    finally:
        engine.drop_collection("dl_e")


# ---- sharded engines (one GPU: the shards share device 0) ----------------------
@pytest.mark.parametrize("shards", [[0, 0], [0, 0, 0]])
def test_striped_delete_equals_single_device(engine, orc, pkg, shards):
    """The same pairs, rows, checksum and search keys as the single-device
    engine after the same delete. N and S leave the shards' counts uneven:
    1003 rows, 95 distinct deleted."""
    n, dim = 1003, 128
    rng = np.random.default_rng(len(shards))
    X = orc.np_bf16_round((rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(np.float32))
    d = _delete_set(rng, n, 95)
    want, frm, to = _compact(X, d)
    Q = rng.standard_normal((5, dim)).astype(np.float32)
    with pkg.VectorEngine(shards=shards) as sh:
        for e in (sh, engine):
            e.create_collection("dl_s", dim, 1, 1)
        try:
            for e in (sh, engine):
                e.upsert("dl_s", np.arange(n), X)
                gf, gt = e.delete("dl_s", d)
                assert np.array_equal(gf, frm) and np.array_equal(gt, to)
                assert e.collection_info("dl_s")["rows"] == want.shape[0]
            got = sh.read_rows("dl_s", 0, want.shape[0])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            assert sh.checksum("dl_s") == engine.checksum("dl_s") == orc.checksum(_raw(want, True))
            for nq, k in ((1, 10), (5, 10), (2, 200)):
                res = _check(orc, sh, "dl_s", want, Q[:nq], k, True)
                assert _same_keys(res, engine.search("dl_s", Q[:nq], k))
            # appends go on from the new count on every shard
            for e in (sh, engine):
                e.upsert("dl_s", np.arange(want.shape[0], want.shape[0] + 7), X[:7])
            full = np.concatenate([want, X[:7]])
            res = _check(orc, sh, "dl_s", full, Q, 10, True)
            assert _same_keys(res, engine.search("dl_s", Q, 10))
            with pytest.raises(pkg.VSError):
                sh.delete("dl_s", [full.shape[0]])
        finally:
            sh.drop_collection("dl_s")
            engine.drop_collection("dl_s")


def test_striped_filter_dies_with_the_delete(pkg, orc):
    n, dim = 200, 128
    X = orc.generate(8, 0, n, dim)
    with pkg.VectorEngine(shards=[0, 0]) as sh:
        sh.create_collection("f", dim, 1, 0)
        sh.generate("f", n, 8)
        fid = sh.filter_create("f", np.ones(n, bool))
        assert sh.search_filter_id("f", X[:1], 3, fid)[2][0] == 3
        sh.delete("f", [5])
        with pytest.raises(pkg.VSError):
            sh.search_filter_id("f", X[:1], 3, fid)
        sh.upsert("f", [n - 1], X[:1])
        with pytest.raises(pkg.VSError):
            sh.search_filter_id("f", X[:1], 3, fid)


def test_placed_delete_on_the_second_slot(pkg, orc):
    """VS_FLAG_PLACE_COLLECTIONS with VS_FLAG_ENGINE_PER_SHARD: the second
    collection lands on the second slot and deletes there."""
    n, dim = 1000, 128
    rng = np.random.default_rng(9)
    d = _delete_set(rng, n, 90)
    with pkg.VectorEngine(shards=[0, 0], place_collections=True, engine_per_shard=True) as pl:
        X = {}
        for i, name in enumerate(("p0", "p1")):
            pl.create_collection(name, dim, 1, 1, n)
            # p0 takes the first slot, p1 the second (both on GPU 0)
            h = json.loads(pl.health())
            assert [dv["collections"] for dv in h["devices"]] == [1, i], h
            pl.generate(name, n, 50 + i)
            X[name] = orc.generate(50 + i, 0, n, dim, bf16=True)
        want, frm, to = _compact(X["p1"], d)
        fid = pl.filter_create("p1", np.ones(n, bool))
        gf, gt = pl.delete("p1", d)
        assert np.array_equal(gf, frm) and np.array_equal(gt, to)
        assert pl.collection_info("p1")["rows"] == want.shape[0]
        assert pl.collection_info("p0")["rows"] == n
        with pytest.raises(pkg.VSError):
            pl.search_filter_id("p1", X["p1"][:1], 3, fid)
        Q = orc.generate(orc.SEED_QUERY, 0, 4, dim)
        _check(orc, pl, "p1", want, Q, 10, True)
        _check(orc, pl, "p0", X["p0"], Q, 10, True)
