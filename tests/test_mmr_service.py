"""/search's "mmr" object in the service layer (include/vsearch_service.h), on CPU.

The real handler code (csrc/service/*.cpp) runs over a CPU test double of the
engine C-ABI: tests/mmr/fake_engine_mmr.cpp, which is the double of the /delete
tests plus vs_search_mmr by the header's rule and a log of every search call.
The log is how the tests see WHICH engine call a request became: an "mmr"
request must be one vs_search_mmr call past the batcher, and a request without
it must make the call it always made. The 501 case links the same handlers
against the old double, which has no vs_search_mmr (the symbol is referenced
weakly). The reference's /search has no rerank (rag/vector-service/
main.go:227-278); the GPU run over the HIP engine is tests/test_mmr_http_gpu.py.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_delete_service import CONFIG, DIM, FAKE_OLD, ROOT, SOURCES, _Svc, _uuid

FAKE_MMR = os.path.join(ROOT, "tests", "mmr", "fake_engine_mmr.cpp")
N = 90
RNG = np.random.default_rng(23)
CENTRES = RNG.standard_normal((6, DIM)).astype(np.float32)
# near-duplicates: six clusters, and every third point an exact copy of its neighbour
VECS = (CENTRES[np.arange(N) % 6] + 0.05 * RNG.standard_normal((N, DIM))).astype(np.float32)
VECS[2::3] = VECS[1::3]
QUERY = (CENTRES[1] + 0.3 * CENTRES[0]).astype(np.float32)


def _build(tmp, name, fake):
    so = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", *SOURCES, fake,
                    "-o", so], check=True, capture_output=True, timeout=600)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mmrsvc")
    new = _build(d, "libvsvc_mmr.so", FAKE_MMR)
    new.fake_calls.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    new.fake_calls.restype = ctypes.c_size_t
    return {"new": new, "old": _build(d, "libvsvc_old.so", FAKE_OLD)}


def _point(i):
    return {"id": _uuid(i), "vector": [float(x) for x in VECS[i]],
            "payload": {"text": f"chunk {i}", "document_id": f"d{i % 4}"}}


def _calls(L):
    buf = ctypes.create_string_buffer(1 << 16)
    L.fake_calls(buf, len(buf))
    return buf.value.decode().splitlines()


def _noq(line):
    """A log line without its query hash."""
    return re.sub(r" q=[0-9a-f]{16}", "", line)


def _open(L, **cfg):
    s = _Svc(L, dict(CONFIG, **cfg))
    st, body, _ = s.handle("POST", "/upsert", {"collection": "docs",
                                               "points": [_point(i) for i in range(N)]})
    assert st == 200, body
    return s


@pytest.fixture()
def svc(libs):
    s = _open(libs["new"])
    _calls(libs["new"])
    yield s
    s.close()


def _body(k=8, **extra):
    return dict(collection="docs", top_k=k, query=[float(x) for x in QUERY], **extra)


def _normed(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _mmr_ids(k, F, d, allow=None):
    """The header's rule over the stored (normalised) rows, in float64."""
    X, q = _normed(VECS), _normed(QUERY)
    rows = np.arange(N) if allow is None else np.flatnonzero(allow)
    s = X[rows] @ q
    cand = rows[np.lexsort((rows, -s))][:F]
    s, G = X[cand] @ q, X[cand] @ X[cand].T
    sel, free, pen = [0], np.ones(len(cand), bool), G[0].copy()
    free[0] = False
    while len(sel) < min(k, len(cand)):
        v = np.where(free, (1 - d) * s - d * pen, -np.inf)
        i = int(np.argmax(v))
        sel.append(i)
        free[i] = False
        pen = np.maximum(pen, G[i])
    return [_uuid(int(cand[i])) for i in sel]


def test_mmr_request_is_one_engine_call_past_the_batcher(svc):
    """Batching is on in CONFIG: a plain request reaches the engine through the
    batcher's vs_search; an mmr request is exactly one vs_search_mmr call."""
    st, out, ct = svc.handle("POST", "/search", _body(8, mmr={"diversity": 0.5,
                                                               "candidates_limit": 40}))
    assert st == 200 and ct == "application/json", out
    log = _calls(svc.L)
    assert len(log) == 1 and log[0].startswith("vs_search_mmr docs nq=1 dim=16 k=8 "), log
    assert log[0].endswith(" F=40 d=0.5 filter=0"), log
    res = json.loads(out)
    assert res["count"] == 8 and [h["id"] for h in res["results"]] == _mmr_ids(8, 40, 0.5)
    # selection order, not score order; every hit carries its relevance score and payload
    scores = [h["score"] for h in res["results"]]
    assert scores != sorted(scores, reverse=True)
    plain = {h["id"]: h for h in svc.search(QUERY, N)}
    for h in res["results"]:
        assert h["payload"] == plain[h["id"]]["payload"]
        assert abs(h["score"] - plain[h["id"]]["score"]) < 1e-6
    # the exact copies crowd plain search's answer, and this one less
    def distinct(hits):
        return len({tuple(VECS[int(h["id"][:8], 16)]) for h in hits})
    assert distinct(res["results"]) > distinct(svc.search(QUERY, 8))


def test_defaults_and_clamping(svc):
    for mmr, k, want in (({}, 8, " k=8 F=0 d=0.5 filter=0"),                      # both defaults
                         ({"diversity": 0.25}, 3, " k=3 F=0 d=0.25 filter=0"),
                         ({"candidates_limit": 4}, 9, " k=9 F=9 d=0.5 filter=0"),   # raised to k
                         ({"candidates_limit": 128, "diversity": 1}, 500, f" k={N} F=128 d=1 filter=0"),
                         ({"diversity": None, "candidates_limit": None}, 2, " k=2 F=0 d=0.5 filter=0"),
                         ({"diversity": 0, "candidates_limit": 0, "other": [1]}, 2,
                          " k=2 F=0 d=0 filter=0")):
        st, out, _ = svc.handle("POST", "/search", _body(k, mmr=mmr))
        assert st == 200, (mmr, out)
        log = _calls(svc.L)
        assert len(log) == 1 and log[0].startswith("vs_search_mmr docs nq=1 dim=16") and \
            _noq(log[0]).endswith(want), (mmr, log)
        kk, cl, d = min(k, N), mmr.get("candidates_limit") or 0, mmr.get("diversity")
        F = max(cl, kk) if cl else min(4 * kk, 128)
        # the double computes in fp32: deep into a long selection its near-ties (the
        # exact copies' penalties of 1 +- an ulp) may fall the other way, so the
        # order is held for the first 8 and the rest as a set
        got, want_ids = [h["id"] for h in json.loads(out)["results"]], \
            _mmr_ids(kk, F, 0.5 if d is None else d)
        assert got[:8] == want_ids[:8] and len(got) == len(want_ids), mmr
        if kk == N:
            assert set(got) == set(want_ids)
    # top_k defaults to 5 as always
    body = _body(mmr={})
    del body["top_k"]
    assert svc.handle("POST", "/search", body)[0] == 200
    assert _noq(_calls(svc.L)[0]).endswith(" k=5 F=0 d=0.5 filter=0")


@pytest.mark.parametrize("mmr", [[], "x", 3, True, {"diversity": "0.5"}, {"diversity": [0.5]},
                                 {"diversity": -0.01}, {"diversity": 1.5}, {"diversity": 1e40},
                                 {"candidates_limit": 2.5}, {"candidates_limit": "8"},
                                 {"candidates_limit": -1}, {"candidates_limit": 129},
                                 {"candidates_limit": 1 << 40}, {"candidates_limit": {}}])
def test_malformed_mmr_is_a_bad_request(svc, mmr):
    st, out, ct = svc.handle("POST", "/search", _body(5, mmr=mmr))
    assert (st, out, ct) == (400, b'{"error":"Invalid request body"}\n', "application/json"), mmr
    assert _calls(svc.L) == []   # nothing reached the engine


def test_top_k_above_the_limit_after_the_clamp(libs):
    s = _open(libs["new"])
    try:
        more = [{"id": _uuid(1000 + i), "vector": [float(x) for x in RNG.standard_normal(DIM)]}
                for i in range(60)]
        assert s.handle("POST", "/upsert", {"collection": "docs", "points": more})[0] == 200
        _calls(libs["new"])
        st, out, _ = s.handle("POST", "/search", _body(129, mmr={}))   # 150 rows: no clamp helps
        assert st == 400 and json.loads(out)["error"] == "top_k must not exceed 128 with mmr"
        assert _calls(libs["new"]) == []
        st, out, _ = s.handle("POST", "/search", _body(128, mmr={}))
        assert st == 200 and json.loads(out)["count"] == 128
        assert _noq(_calls(libs["new"])[0]).endswith(" k=128 F=0 d=0.5 filter=0")
        # as a plain /search answers them: a negative top_k, a wrong dim, an unknown collection
        assert s.handle("POST", "/search", _body(-1, mmr={}))[0] == 400
        bad = _body(5, mmr={})
        bad["query"] = bad["query"][:3]
        assert s.handle("POST", "/search", bad) == s.handle("POST", "/search",
                                                            {k: v for k, v in bad.items() if k != "mmr"})
        assert s.handle("POST", "/search", dict(_body(5, mmr={}), collection="nope"))[0] == 500
        assert s.handle("GET", "/search")[0] == 405
    finally:
        s.close()


def test_request_without_mmr_is_unchanged(libs):
    """The same body without "mmr" (and with "mmr": null) makes the engine call
    it always made, the same with and without batching, and the same reply."""
    for batching in (True, False):
        s = _open(libs["new"], batching={"enabled": batching, "max_batch": 64})
        try:
            _calls(libs["new"])
            st, plain, _ = s.handle("POST", "/search", _body(8))
            first = _calls(libs["new"])
            assert st == 200 and len(first) == 1
            q = first[0].split(" q=")[1]
            assert first[0] == f"vs_search docs nq=1 dim=16 k=8 q={q}", first
            st, again, _ = s.handle("POST", "/search", _body(8, mmr=None))
            assert st == 200 and again == plain and _calls(libs["new"]) == first
            # the mmr request carries the same query bytes to the engine
            assert s.handle("POST", "/search", _body(8, mmr={}))[0] == 200
            assert _calls(libs["new"])[0].split(" q=")[1].split()[0] == q
            # the fast decoder's body (retrieval-service's shape) too
            raw = json.dumps({"collection": "docs", "filter": None, "query": [float(x) for x in QUERY],
                              "top_k": 8}).encode()
            st, fast, _ = s.handle("POST", "/search", raw)
            assert st == 200 and fast == plain and _calls(libs["new"]) == first
        finally:
            s.close()


def test_mmr_with_a_payload_filter(libs):
    """"filter":"match": the request's filter is made resident and its id goes to
    vs_search_mmr; "filter":"ignore" (the default) drops it, as for plain search."""
    s = _open(libs["new"], filter="match")
    try:
        _calls(libs["new"])
        f = {"document_id": "d1"}
        st, out, _ = s.handle("POST", "/search", _body(6, filter=f, mmr={"candidates_limit": 20}))
        assert st == 200, out
        log = _calls(libs["new"])
        assert len(log) == 1 and " F=20 d=0.5 filter=" in log[0] and not log[0].endswith("filter=0")
        allow = np.arange(N) % 4 == 1
        assert [h["id"] for h in json.loads(out)["results"]] == _mmr_ids(6, 20, 0.5, allow)
        # fewer matching points than top_k: all of them, counted
        st, out, _ = s.handle("POST", "/search", _body(6, filter={"text": "chunk 7"}, mmr={}))
        assert st == 200 and [h["id"] for h in json.loads(out)["results"]] == [_uuid(7)]
    finally:
        s.close()
    s = _open(libs["new"])
    try:
        _calls(libs["new"])
        st, out, _ = s.handle("POST", "/search", _body(6, filter={"document_id": "d1"}, mmr={}))
        assert st == 200 and _calls(libs["new"])[0].endswith(" filter=0")
        assert [h["id"] for h in json.loads(out)["results"]] == _mmr_ids(6, 24, 0.5)
    finally:
        s.close()


def test_501_without_vs_search_mmr(libs):
    s = _Svc(libs["old"])
    try:
        st, body, _ = s.handle("POST", "/upsert", {"collection": "docs",
                                                   "points": [_point(i) for i in range(6)]})
        assert st == 200, body
        st, out, _ = s.handle("POST", "/search", _body(3, mmr={"diversity": 0.3}))
        assert st == 501 and "error" in json.loads(out)
        assert s.handle("POST", "/search", _body(3, mmr="x"))[0] == 400   # request checks come first
        assert s.handle("GET", "/search")[0] == 405
        assert len(s.search(QUERY, 3)) == 3                                # plain search is served
        assert len(json.loads(s.handle("POST", "/search", _body(3, mmr=None))[1])["results"]) == 3
    finally:
        s.close()
