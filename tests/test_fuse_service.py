"""/search's "fusion" object in the service layer (include/vsearch_service.h), on CPU.

The real handler code (csrc/service/*.cpp) runs over a CPU test double of the
engine C-ABI: tests/fuse/fake_engine_fuse.cpp, the logging double of the MMR
tests plus vs_search_fused by the header's rule. The log shows WHICH engine call
a request became and with which arguments: a "fusion" request must be exactly
one vs_search_fused call with nq = 1 past the batcher, `query` first and
fusion.queries after it; a request without it must make the call it always
made. The 501 case links the same handlers against the MMR double, which has no
vs_search_fused (the symbol is referenced weakly). The GPU run over the HIP
engine is tests/test_fuse_http_gpu.py.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from test_delete_service import CONFIG, DIM, ROOT, SOURCES, _Svc, _uuid

FAKE_FUSE = os.path.join(ROOT, "tests", "fuse", "fake_engine_fuse.cpp")
FAKE_MMR = os.path.join(ROOT, "tests", "mmr", "fake_engine_mmr.cpp")
N = 90
RNG = np.random.default_rng(29)
CENTRES = RNG.standard_normal((6, DIM)).astype(np.float32)
VECS = (CENTRES[np.arange(N) % 6] + 0.3 * RNG.standard_normal((N, DIM))).astype(np.float32)
# three phrasings of one question
QUERIES = (CENTRES[1] + 0.25 * RNG.standard_normal((3, DIM))).astype(np.float32)


def _build(tmp, name, fake):
    so = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", *SOURCES, fake,
                    "-o", so], check=True, capture_output=True, timeout=600)
    L = ctypes.CDLL(so)
    L.fake_calls.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.fake_calls.restype = ctypes.c_size_t
    return L


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("fusesvc")
    return {"new": _build(d, "libvsvc_fuse.so", FAKE_FUSE), "old": _build(d, "libvsvc_mmr.so", FAKE_MMR)}


def _point(i):
    return {"id": _uuid(i), "vector": [float(x) for x in VECS[i]],
            "payload": {"text": f"chunk {i}", "document_id": f"d{i % 4}"}}


def _calls(L):
    buf = ctypes.create_string_buffer(1 << 16)
    L.fake_calls(buf, len(buf))
    return buf.value.decode().splitlines()


def _open(L, **cfg):
    s = _Svc(L, dict(CONFIG, **cfg))
    st, body, _ = s.handle("POST", "/upsert", {"collection": "docs",
                                               "points": [_point(i) for i in range(N)]})
    assert st == 200, body
    _calls(L)
    return s


@pytest.fixture()
def svc(libs):
    s = _open(libs["new"])
    yield s
    s.close()


def _vec(v):
    return [float(x) for x in v]


def _body(k=8, **extra):
    return dict(collection="docs", top_k=k, query=_vec(QUERIES[0]), **extra)


def _fusion(**kw):
    return dict({"queries": [_vec(QUERIES[1]), _vec(QUERIES[2])]}, **kw)


def _head(line):
    """A fused log line without its query hashes; and the hashes."""
    parts = line.split(" q=")
    return parts[0], parts[1:]


def _fused_ids(queries, k, F, method="rrf", K=2, allow=None):
    """The header's rule over the stored (normalised) rows: (ids, scores)."""
    X = VECS.astype(np.float64)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    rows = np.arange(N) if allow is None else np.flatnonzero(allow)
    fused = {}
    for q in np.asarray(queries, np.float64):
        s = X[rows] @ (q / np.linalg.norm(q))
        order = np.lexsort((rows, -s))[:F]
        sc = s[order]
        mu, sd = sc.mean(), (sc.std(ddof=1) if len(sc) > 1 else 0.0)
        for p, i in enumerate(order):
            if method == "rrf":
                t = np.float32(1) / np.float32(p + K)
            else:
                t = np.float32((sc[p] - (mu - 3 * sd)) / (6 * sd)) if sd > 0 else np.float32(0.5)
            r = int(rows[i])
            fused[r] = t if r not in fused else np.float32(fused[r] + t)
    top = sorted(fused.items(), key=lambda kv: (-kv[1], kv[0]))[:k]
    return [_uuid(r) for r, _ in top], [float(v) for _, v in top]


def test_fused_request_is_one_engine_call_past_the_batcher(svc):
    st, out, ct = svc.handle("POST", "/search", _body(8, fusion=_fusion(prefetch_limit=40)))
    assert st == 200 and ct == "application/json", out
    log = _calls(svc.L)
    assert len(log) == 1, log
    head, hashes = _head(log[0])
    assert head == "vs_search_fused docs nq=1 n_sub=3 dim=16 k=8 F=40 fusion=0 rrf_k=0 filter=0"
    assert len(hashes) == 3 and len(set(hashes)) == 3
    res = json.loads(out)
    ids, scores = _fused_ids(QUERIES, 8, 40)
    assert res["count"] == 8 and [h["id"] for h in res["results"]] == ids
    # the score is the fused score: RRF is exact whatever the double's dot products round to
    assert [h["score"] for h in res["results"]] == scores
    plain = {h["id"]: h for h in svc.search(QUERIES[0], N)}
    for h in res["results"]:
        assert h["payload"] == plain[h["id"]]["payload"]
    # `query` is sub-query 0 and fusion.queries follow in order: the plain request's
    # query hash is the first, and swapping the extras swaps the other two
    _calls(svc.L)
    svc.search(QUERIES[0], 3)
    q0 = _calls(svc.L)[0].split(" q=")[1]
    assert hashes[0] == q0
    svc.handle("POST", "/search", _body(8, fusion={"queries": [_vec(QUERIES[2]), _vec(QUERIES[1])]}))
    assert _head(_calls(svc.L)[0])[1] == [hashes[0], hashes[2], hashes[1]]


def test_defaults_methods_and_clamping(svc):
    two = [_vec(QUERIES[1]), _vec(QUERIES[2])]
    for fusion, k, want in (
            ({"queries": two}, 8, "n_sub=3 dim=16 k=8 F=0 fusion=0 rrf_k=0 filter=0"),
            ({"queries": two[:1], "method": "rrf", "rrf_k": 60}, 3,
             "n_sub=2 dim=16 k=3 F=0 fusion=0 rrf_k=60 filter=0"),
            ({"queries": two, "method": "dbsf"}, 5, "n_sub=3 dim=16 k=5 F=0 fusion=1 rrf_k=0 filter=0"),
            ({"queries": two, "prefetch_limit": 4}, 9, "n_sub=3 dim=16 k=9 F=9 fusion=0 rrf_k=0 filter=0"),
            ({"queries": two, "prefetch_limit": 128, "rrf_k": 65536}, 500,
             f"n_sub=3 dim=16 k={N} F=128 fusion=0 rrf_k=65536 filter=0"),
            ({"queries": two, "method": None, "prefetch_limit": None, "rrf_k": None, "other": 1}, 2,
             "n_sub=3 dim=16 k=2 F=0 fusion=0 rrf_k=0 filter=0"),
            ({"queries": two * 3 + two[:1], "rrf_k": 0}, 4,
             "n_sub=8 dim=16 k=4 F=0 fusion=0 rrf_k=0 filter=0")):
        st, out, _ = svc.handle("POST", "/search", _body(k, fusion=fusion))
        assert st == 200, (fusion, out)
        log = _calls(svc.L)
        assert len(log) == 1 and _head(log[0])[0] == "vs_search_fused docs nq=1 " + want, (fusion, log)
        kk = min(k, N)
        F = max(fusion.get("prefetch_limit") or 0, kk) if fusion.get("prefetch_limit") else min(4 * kk, 128)
        qs = np.concatenate([QUERIES[:1], np.asarray(fusion["queries"], np.float32)])
        res = json.loads(out)["results"]
        if fusion.get("method") == "dbsf":   # fp32 dot products in the double: scores within rounding
            ids, scores = _fused_ids(qs, kk, F, "dbsf")
            assert len(res) == kk
            assert np.allclose([h["score"] for h in res], scores, atol=1e-4)
        else:
            ids, scores = _fused_ids(qs, kk, F, "rrf", fusion.get("rrf_k") or 2)
            assert [h["score"] for h in res] == scores, fusion
            assert sorted(h["id"] for h in res) == sorted(ids) or len(set(scores)) < len(scores)
    body = _body(fusion={"queries": two})   # top_k defaults to 5 as always
    del body["top_k"]
    assert svc.handle("POST", "/search", body)[0] == 200
    assert " k=5 F=0 " in _calls(svc.L)[0]


ONE = [[0.0] * DIM]


@pytest.mark.parametrize("fusion", [
    [], "rrf", 3, True, {}, {"queries": None}, {"queries": []}, {"queries": ONE * 8},
    {"queries": "x"}, {"queries": {}}, {"queries": ONE, "method": "sum"},
    {"queries": ONE, "method": 1}, {"queries": ONE, "method": ["rrf"]},
    {"queries": ONE, "prefetch_limit": -1}, {"queries": ONE, "prefetch_limit": 129},
    {"queries": ONE, "prefetch_limit": 2.5}, {"queries": ONE, "prefetch_limit": "8"},
    {"queries": ONE, "rrf_k": -1}, {"queries": ONE, "rrf_k": 65537}, {"queries": ONE, "rrf_k": 1.5},
    {"queries": ONE, "rrf_k": "2"}, {"queries": ONE, "rrf_k": 1 << 40},
    {"queries": ONE, "method": "dbsf", "rrf_k": 2}, {"queries": ONE, "method": "dbsf", "rrf_k": 0}])
def test_malformed_fusion_is_a_bad_request(svc, fusion):
    st, out, ct = svc.handle("POST", "/search", _body(5, fusion=fusion))
    assert (st, out, ct) == (400, b'{"error":"Invalid request body"}\n', "application/json"), fusion
    assert _calls(svc.L) == []   # nothing reached the engine


def test_fusion_excludes_mmr_and_group_by(svc):
    for extra in ({"mmr": {}}, {"group_by": "document_id"}):
        st, out, _ = svc.handle("POST", "/search", _body(5, fusion={"queries": ONE}, **extra))
        assert (st, out) == (400, b'{"error":"Invalid request body"}\n'), extra
    assert _calls(svc.L) == []


def test_extra_vectors_follow_convert_vector(svc):
    """Each extra vector passes convertVector's rules with its texts (as /upsert's
    vectors do), and must have the collection's dim (as `query` must)."""
    for qs, text in (([5], "point vector must be an array"),
                     ([ONE[0], "x"], "point vector must be an array"),
                     ([{"a": 1}], "point vector must be an array"),
                     ([[0.5, "1"] + [0.0] * (DIM - 2)], "vector contains non-numeric value"),
                     ([ONE[0], [None] * DIM], "vector contains non-numeric value")):
        st, out, _ = svc.handle("POST", "/search", _body(5, fusion={"queries": qs}))
        assert st == 400 and json.loads(out)["error"] == text, (qs, out)
    short = dict(_body(5), query=_vec(QUERIES[0][:3]))
    want = svc.handle("POST", "/search", short)          # the dimension error of `query`
    assert want[0] == 500
    st, out, _ = svc.handle("POST", "/search", _body(5, fusion={"queries": [ONE[0], [1.0, 2.0, 3.0]]}))
    assert (st, out) == (want[0], want[1])
    _calls(svc.L)
    assert svc.handle("POST", "/search", dict(short, fusion={"queries": ONE}))[:2] == want[:2]
    assert [l for l in _calls(svc.L) if l.startswith("vs_search_fused")] == []


def test_top_k_above_the_limit_after_the_clamp(libs):
    s = _open(libs["new"])
    try:
        more = [{"id": _uuid(1000 + i), "vector": _vec(RNG.standard_normal(DIM))} for i in range(60)]
        assert s.handle("POST", "/upsert", {"collection": "docs", "points": more})[0] == 200
        _calls(libs["new"])
        st, out, _ = s.handle("POST", "/search", _body(129, fusion=_fusion()))   # 150 rows
        assert st == 400 and json.loads(out)["error"] == "top_k must not exceed 128 with fusion"
        assert _calls(libs["new"]) == []
        st, out, _ = s.handle("POST", "/search", _body(128, fusion=_fusion()))
        assert st == 200 and json.loads(out)["count"] == 128
        assert " k=128 F=0 " in _calls(libs["new"])[0]
        assert s.handle("POST", "/search", _body(-1, fusion=_fusion()))[0] == 400
        assert s.handle("POST", "/search", dict(_body(5, fusion=_fusion()), collection="nope"))[0] == 500
    finally:
        s.close()


def test_request_without_fusion_is_unchanged(libs):
    """The same body without "fusion" (and with "fusion": null) leaves the call
    log of a plain search, with and without batching, and the same reply."""
    for batching in (True, False):
        s = _open(libs["new"], batching={"enabled": batching, "max_batch": 64})
        try:
            st, plain, _ = s.handle("POST", "/search", _body(8))
            first = _calls(libs["new"])
            assert st == 200 and len(first) == 1
            q = first[0].split(" q=")[1]
            assert first[0] == f"vs_search docs nq=1 dim=16 k=8 q={q}", first
            st, again, _ = s.handle("POST", "/search", _body(8, fusion=None))
            assert st == 200 and again == plain and _calls(libs["new"]) == first
            raw = json.dumps({"collection": "docs", "filter": None, "query": _vec(QUERIES[0]),
                              "top_k": 8}).encode()
            st, fast, _ = s.handle("POST", "/search", raw)
            assert st == 200 and fast == plain and _calls(libs["new"]) == first
            # mmr and group_by requests are not touched either
            assert s.handle("POST", "/search", _body(8, mmr={}))[0] == 200
            assert _calls(libs["new"])[0].startswith("vs_search_mmr docs nq=1 dim=16 k=8 ")
        finally:
            s.close()


def test_fusion_with_a_payload_filter(libs):
    """"filter":"match": the filter is made resident and its id goes to
    vs_search_fused; "filter":"ignore" (the default) drops it, as for plain search."""
    s = _open(libs["new"], filter="match")
    try:
        st, out, _ = s.handle("POST", "/search", _body(6, filter={"document_id": "d1"},
                                                       fusion=_fusion(prefetch_limit=20)))
        assert st == 200, out
        log = _calls(libs["new"])
        head = _head(log[0])[0]
        assert len(log) == 1 and " F=20 fusion=0 rrf_k=0 filter=" in head and not head.endswith("filter=0")
        ids, scores = _fused_ids(QUERIES, 6, 20, allow=np.arange(N) % 4 == 1)
        res = json.loads(out)["results"]
        assert [h["score"] for h in res] == scores
        assert all(int(h["id"][:8], 16) % 4 == 1 for h in res)
        # fewer matching points than top_k: all of them, counted
        st, out, _ = s.handle("POST", "/search", _body(6, filter={"text": "chunk 7"}, fusion=_fusion()))
        assert st == 200 and [h["id"] for h in json.loads(out)["results"]] == [_uuid(7)]
    finally:
        s.close()
    s = _open(libs["new"])
    try:
        st, out, _ = s.handle("POST", "/search", _body(6, filter={"document_id": "d1"}, fusion=_fusion()))
        assert st == 200 and _head(_calls(libs["new"])[0])[0].endswith(" filter=0")
    finally:
        s.close()


def test_501_without_vs_search_fused(libs):
    s = _Svc(libs["old"])
    try:
        st, body, _ = s.handle("POST", "/upsert", {"collection": "docs",
                                                   "points": [_point(i) for i in range(6)]})
        assert st == 200, body
        st, out, _ = s.handle("POST", "/search", _body(3, fusion=_fusion()))
        assert st == 501 and "error" in json.loads(out)
        assert s.handle("POST", "/search", _body(3, fusion="x"))[0] == 400   # request checks come first
        assert s.handle("POST", "/search", _body(3, fusion={"queries": [5]}))[0] == 400
        assert len(s.search(QUERIES[0], 3)) == 3                              # plain search is served
        assert len(json.loads(s.handle("POST", "/search", _body(3, fusion=None))[1])["results"]) == 3
    finally:
        s.close()
