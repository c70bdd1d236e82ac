"""POST /delete over real HTTP on the device: the listener (vsvc_http_start)
in front of the handler mirror and the HIP engine. Points are removed by ids
and by a payload filter between searches, and every /search reply is held to
the oracle on the rows that are left, with ids mapped through the test's own
bookkeeping, not the service's: a moved row must answer with the id and
payload it was upserted with. The CPU tests of the route are
tests/test_delete_service.py; the engine's are tests/test_delete_gpu.py."""
import http.client
import json
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = {"collections": [{"name": "b16", "dim": 768, "metric": "Cosine", "dtype": "bf16"}],
       "batching": {"max_wait_us": 2000}}


def _post(port, path, obj):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", path, body=json.dumps(obj), headers={"Content-Type": "application/json"})
    r = c.getresponse()
    out = (r.status, r.read())
    c.close()
    return out


def test_delete_over_http_gpu(pkg, orc):
    from importlib import import_module
    svcmod = import_module(pkg.__name__ + ".service")
    n, dim = 3000, 768
    rng = np.random.default_rng(8)
    ids = [str(uuid.UUID(bytes=rng.bytes(16), version=4)) for _ in range(n)]
    X = orc.generate(71, 0, n, dim)
    Xp = orc.preprocess(X, True, True)
    eng = pkg.VectorEngine(device=0)
    s = svcmod.VectorService(eng, CFG)
    try:
        with s.serve("127.0.0.1:0") as lis:
            for lo in range(0, n, 500):
                st, body = _post(lis.port, "/upsert", {"collection": "b16", "points": [
                    {"id": ids[i], "vector": X[i].tolist(),
                     "payload": {"i": i, "document_id": f"doc{i % 9}"}}
                    for i in range(lo, lo + 500)]})
                assert st == 200, body
            live = np.ones(n, bool)
            Q = orc.generate(orc.SEED_QUERY, 40, 6, dim)

            def check():
                idx = np.flatnonzero(live)
                pos = {ids[i]: j for j, i in enumerate(idx)}
                for qi, k in ((0, 10), (1, 3), (2, 50)):
                    q = Q[qi] if qi % 2 == 0 else X[idx[-1 - qi]]  # a tail row: moved rows
                    st, body = _post(lis.port, "/search", {"collection": "b16", "filter": None,
                                                           "query": q.tolist(), "top_k": k})
                    assert st == 200, body
                    res = json.loads(body)["results"]
                    assert len(res) == k and all(r["id"] in pos for r in res)
                    assert all(ids[r["payload"]["i"]] == r["id"] for r in res)
                    rows = np.array([[pos[r["id"]] for r in res]], np.uint64)
                    scores = np.array([[r["score"] for r in res]])
                    qp = orc.preprocess(q[None, :], True, True)
                    _, s64, rr, cc = orc.search(Xp[idx], qp, k)
                    resc = orc.rescore(Xp[idx], qp, rows, np.array([k], np.uint32))
                    bad = orc.check_topk(scores, rows, np.array([k]), s64, rr, cc, resc, 1e-5)
                    assert not bad, bad[:3]

            check()
            gone = [5, 1700, n - 1, n - 2, 64]
            st, body = _post(lis.port, "/delete", {"collection": "b16",
                                                   "ids": [ids[i] for i in gone] + [ids[5]]})
            assert st == 200 and json.loads(body) == {"collection": "b16", "deleted": 5,
                                                      "status": "success"}, body
            live[gone] = False
            check()
            st, body = _post(lis.port, "/delete", {"collection": "b16",
                                                   "filter": {"document_id": "doc4"}})
            want = [i for i in range(n) if live[i] and i % 9 == 4]
            assert st == 200 and json.loads(body)["deleted"] == len(want), body
            live[want] = False
            check()
            assert eng.collection_info("b16")["rows"] == int(live.sum())
            # a deleted id upserted again is a new point, appended
            st, body = _post(lis.port, "/upsert", {"collection": "b16", "points": [
                {"id": ids[5], "vector": X[5].tolist(), "payload": {"i": 5, "document_id": "x"}}]})
            assert st == 200, body
            st, body = _post(lis.port, "/search", {"collection": "b16", "query": X[5].tolist(),
                                                   "top_k": 1})
            assert st == 200 and json.loads(body)["results"][0]["id"] == ids[5]
            assert eng.collection_info("b16")["rows"] == int(live.sum()) + 1
    finally:
        s.close()
        eng.close()
