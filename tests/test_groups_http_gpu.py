"""/search with "group_by" over real HTTP on the device: the listener
(vsvc_http_start) in front of the handler mirror and the HIP engine. 300
points of 40 documents on exactly representable data (entries in {-1, 0, 1}/8,
a DOT collection: every score is exact), top_k = 5 groups of group_size = 2,
held to tests/groups_ref.py over a float64 ranking. The same request without
"group_by" must answer as plain search does. The CPU tests of the route are
tests/test_groups_service.py; the engine's are tests/test_groups_gpu.py."""
import http.client
import json
import uuid

import numpy as np
import pytest

import groups_ref as G

pytestmark = pytest.mark.gpu

CFG = {"collections": [{"name": "chunks", "dim": 768, "metric": "Dot", "dtype": "bf16"}],
       "batching": {"max_wait_us": 2000}, "filter": "match"}


def _post(port, path, obj):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", path, body=json.dumps(obj), headers={"Content-Type": "application/json"})
    r = c.getresponse()
    out = (r.status, r.read())
    c.close()
    return out


def test_groups_over_http_gpu(pkg):
    from importlib import import_module
    svcmod = import_module(pkg.__name__ + ".service")
    n, dim, docs = 300, 768, 40
    rng = np.random.default_rng(13)
    X = rng.integers(-1, 2, (n, dim)).astype(np.float32) / 8
    Q = rng.integers(-1, 2, (3, dim)).astype(np.float32) / 8
    doc = np.sort(rng.integers(0, docs, n))       # contiguous chunks, uneven documents
    doc[::17] = -1                                # a few chunks without a document_id
    ids = [str(uuid.UUID(bytes=rng.bytes(16), version=4)) for _ in range(n)]

    def payload(i):
        p = {"i": i, "lang": "en" if i % 2 else "de"}
        if doc[i] >= 0:
            p["document_id"] = f"doc-{doc[i]}"
        return p

    def want(qi, limit, size, allow=None):
        s = Q[qi].astype(np.float64) @ X.astype(np.float64).T
        values, gor = [], np.full(n, G.GROUP_NONE, np.uint32)
        for r in range(n):
            if doc[r] >= 0 and (allow is None or allow[r]):
                v = f"doc-{doc[r]}"
                if v not in values:
                    values.append(v)
                gor[r] = values.index(v)
        order = np.lexsort((np.arange(n), -s))
        keys = G.make_keys(G.score_image(s[order].astype(np.float32)), order)
        return [(values[g], [(int(G.key_rows(np.uint64(k))), float(G.image_score(np.array([k >> 32], np.uint32))[0]))
                             for k in ks]) for g, ks in G.groups_ref(keys, gor, limit, size)]

    eng = pkg.VectorEngine(device=0)
    s = svcmod.VectorService(eng, CFG)
    try:
        with s.serve("127.0.0.1:0") as lis:
            st, body = _post(lis.port, "/upsert", {"collection": "chunks", "points": [
                {"id": ids[i], "vector": X[i].tolist(), "payload": payload(i)} for i in range(n)]})
            assert st == 200, body

            def ask(qi, k, **extra):
                st, body = _post(lis.port, "/search", dict(collection="chunks", query=Q[qi].tolist(),
                                                           top_k=k, **extra))
                assert st == 200, body
                res = json.loads(body)
                assert res["count"] == len(res["results"])
                assert all(ids[r["payload"]["i"]] == r["id"] for r in res["results"])
                return res

            def check(res, w):
                assert res["groups"] == [{"id": v, "hits": len(h)} for v, h in w]
                flat = [x for _, h in w for x in h]
                assert [(r["payload"]["i"], r["score"]) for r in res["results"]] == flat
                assert all(r["payload"] == payload(r["payload"]["i"]) for r in res["results"])

            for qi in range(3):
                check(ask(qi, 5, group_by="document_id", group_size=2), want(qi, 5, 2))
            check(ask(0, 128, group_by="document_id", group_size=16), want(0, 128, 16))
            check(ask(1, 3, group_by="document_id"), want(1, 3, 1))          # group_size: 1
            # with a payload filter (a resident filter's id goes to the engine)
            allow = np.arange(n) % 2 == 1
            check(ask(2, 5, group_by="document_id", group_size=2, filter={"lang": "en"}),
                  want(2, 5, 2, allow))
            # the same request without group_by: plain search, unchanged
            s0 = Q[0].astype(np.float64) @ X.astype(np.float64).T
            order = np.lexsort((np.arange(n), -s0))[:5]
            for extra in ({}, {"group_by": None}):
                res = ask(0, 5, **extra)
                assert list(res) == ["results", "count"]
                assert [r["payload"]["i"] for r in res["results"]] == [int(r) for r in order]
            # after an /upsert the grouping is rebuilt: a new document takes the lead
            st, body = _post(lis.port, "/upsert", {"collection": "chunks", "points": [
                {"id": str(uuid.UUID(int=7, version=4)), "vector": (Q[0] * 2).tolist(),
                 "payload": {"i": n, "document_id": "doc-new"}}]})
            assert st == 200, body
            st, body = _post(lis.port, "/search", dict(collection="chunks", query=Q[0].tolist(),
                                                       top_k=5, group_by="document_id", group_size=2))
            res = json.loads(body)
            assert st == 200 and res["groups"][0] == {"id": "doc-new", "hits": 1}
            assert res["groups"][1:] == [{"id": v, "hits": len(h)} for v, h in want(0, 5, 2)[:4]]
            # bad requests: nothing is searched
            for bad in ({"group_by": 3}, {"group_by": "document_id", "group_size": 17},
                        {"group_by": "document_id", "mmr": {}}):
                st, body = _post(lis.port, "/search", dict(collection="chunks", query=Q[0].tolist(),
                                                           top_k=5, **bad))
                assert st == 400 and json.loads(body) == {"error": "Invalid request body"}, bad
            st, body = _post(lis.port, "/search", dict(collection="chunks", query=Q[0].tolist(),
                                                       top_k=129, group_by="document_id"))
            assert st == 400, body
    finally:
        s.close()
        eng.close()
