"""/search with "mmr" over real HTTP on the device: the listener
(vsvc_http_start) in front of the handler mirror and the HIP engine, on the
exact-arithmetic fixture of tests/test_mmr_gpu.py (entries in {-1, 0, 1}/8, a
DOT collection: every product and every v is exact, so the reply must name the
reference's ids in the reference's order, ties included). The same request
without "mmr" must answer as plain search does. The CPU tests of the route are
tests/test_mmr_service.py; the engine's are tests/test_mmr_gpu.py."""
import http.client
import json
import uuid

import numpy as np
import pytest

from test_mmr_gpu import _ref_rows, _ternary, _top_f

pytestmark = pytest.mark.gpu

CFG = {"collections": [{"name": "tern", "dim": 768, "metric": "Dot", "dtype": "bf16"}],
       "batching": {"max_wait_us": 2000}, "filter": "match"}


def _post(port, path, obj):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", path, body=json.dumps(obj), headers={"Content-Type": "application/json"})
    r = c.getresponse()
    out = (r.status, r.read())
    c.close()
    return out


def test_mmr_over_http_gpu(pkg):
    from importlib import import_module
    svcmod = import_module(pkg.__name__ + ".service")
    n, dim = 1200, 768
    X, Q = _ternary(n, dim, 51)
    S = Q.astype(np.float64) @ X.astype(np.float64).T
    rng = np.random.default_rng(9)
    ids = [str(uuid.UUID(bytes=rng.bytes(16), version=4)) for _ in range(n)]
    eng = pkg.VectorEngine(device=0)
    s = svcmod.VectorService(eng, CFG)
    try:
        with s.serve("127.0.0.1:0") as lis:
            for lo in range(0, n, 400):
                st, body = _post(lis.port, "/upsert", {"collection": "tern", "points": [
                    {"id": ids[i], "vector": X[i].tolist(), "payload": {"i": i, "doc": f"d{i % 3}"}}
                    for i in range(lo, lo + 400)]})
                assert st == 200, body

            def ask(qi, k, **extra):
                st, body = _post(lis.port, "/search", dict(collection="tern", query=Q[qi].tolist(),
                                                           top_k=k, **extra))
                assert st == 200, body
                res = json.loads(body)
                assert res["count"] == len(res["results"])
                assert all(ids[r["payload"]["i"]] == r["id"] for r in res["results"])
                return [r["payload"]["i"] for r in res["results"]], [r["score"] for r in res["results"]]

            for qi, k, F, d in ((0, 10, 64, 0.5), (1, 16, 128, 0.25), (2, 7, 0, 0.75), (3, 12, 12, 1.0)):
                Fe = F or min(4 * k, 128)
                want, _ = _ref_rows(X, 0, _top_f(S[qi:qi + 1], Fe), k, d)
                rows, scores = ask(qi, k, mmr={"diversity": d, "candidates_limit": F})
                assert rows == [int(r) for r in want[0][0]], (qi, k, F, d)
                assert scores == [float(x) for x in want[0][1]], (qi, k, F, d)
                # the same request without "mmr": plain search, unchanged
                plain = _top_f(S[qi:qi + 1], k)[0]
                rows, scores = ask(qi, k)
                assert rows == [int(r) for r in plain[1]] and scores == [float(x) for x in plain[0]]
                assert ask(qi, k, mmr=None) == (rows, scores)
            # with a payload filter ("filter":"match": a resident filter's id goes to the engine)
            allow = np.arange(n) % 3 == 1
            want, _ = _ref_rows(X, 0, _top_f(S[4:5], 48, 0, allow), 9, 0.5)
            rows, _ = ask(4, 9, filter={"doc": "d1"}, mmr={"candidates_limit": 48})
            assert rows == [int(r) for r in want[0][0]]
            # defaults: diversity 0.5, candidates_limit min(4 top_k, 128)
            want, _ = _ref_rows(X, 0, _top_f(S[5:6], 20), 5, 0.5)
            assert ask(5, 5, mmr={})[0] == [int(r) for r in want[0][0]]
            # bad requests: nothing is searched
            for bad in ({"mmr": 3}, {"mmr": {"diversity": 2}}, {"mmr": {"candidates_limit": 129}}):
                st, body = _post(lis.port, "/search", dict(collection="tern", query=Q[0].tolist(),
                                                           top_k=5, **bad))
                assert st == 400 and json.loads(body) == {"error": "Invalid request body"}, bad
            st, body = _post(lis.port, "/search", dict(collection="tern", query=Q[0].tolist(),
                                                       top_k=129, mmr={}))
            assert st == 400, body
    finally:
        s.close()
        eng.close()
