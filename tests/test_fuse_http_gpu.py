"""/search with "fusion" over real HTTP on the device: the listener
(vsvc_http_start) in front of the handler mirror and the HIP engine, on the
exact-arithmetic fixture of tests/test_fuse_gpu.py (entries in {-1, 0, 1}/8, a
DOT collection: every score is exact, so the candidate lists are numpy's exact
top-F and the reply must carry tests/fuse_ref.py's rows and fused scores bit for
bit). The same request without "fusion" must answer as plain search does. The
CPU tests of the route are tests/test_fuse_service.py; the engine's are
tests/test_fuse_gpu.py."""
import http.client
import json
import uuid

import numpy as np
import pytest

import fuse_ref as FR
from test_fuse_gpu import _ternary

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


def _lists(S, F, allow=None):
    """[n_sub][F] key lists: numpy's exact top-F of every row of S (score desc, row asc)."""
    idx = np.arange(S.shape[1]) if allow is None else np.flatnonzero(allow)
    out = np.zeros((S.shape[0], F), np.uint64)
    for l, s in enumerate(S):
        order = idx[np.lexsort((idx, -s[idx]))][:F]
        out[l, :len(order)] = FR.key_encode(s[order], order)
    return out


def test_fusion_over_http_gpu(pkg):
    from importlib import import_module
    svcmod = import_module(pkg.__name__ + ".service")
    n, dim = 1200, 768
    X, Q = _ternary(n, dim, 51)       # Q: [32 questions][8 rewrites][dim]
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
                st, body = _post(lis.port, "/search", dict(collection="tern", query=Q[qi, 0].tolist(),
                                                           top_k=k, **extra))
                assert st == 200, body
                res = json.loads(body)
                assert res["count"] == len(res["results"])
                assert all(ids[r["payload"]["i"]] == r["id"] for r in res["results"])
                return [r["payload"]["i"] for r in res["results"]], [r["score"] for r in res["results"]]

            def want(keys):
                keys = keys[keys != 0]
                return [int(r) for r in FR.key_row(keys)], [float(x) for x in FR.key_score(keys)]

            for qi, n_sub, k, F, method, K in ((0, 3, 10, 64, "rrf", 0), (1, 8, 16, 128, "rrf", 60),
                                               (2, 2, 7, 0, "rrf", 1), (3, 4, 12, 32, "dbsf", None)):
                fusion = {"method": method, "queries": Q[qi, 1:n_sub].tolist(), "prefetch_limit": F}
                if K is not None:
                    fusion["rrf_k"] = K
                L = _lists(S[qi, :n_sub], F or min(4 * k, 128))
                ref = FR.rrf(L, k, K) if method == "rrf" else FR.dbsf(L, k)[0]
                assert ask(qi, k, fusion=fusion) == want(ref), (qi, n_sub, k, F, method, K)
                # the same request without "fusion": plain search of `query`, unchanged
                plain = want(_lists(S[qi, :1], k)[0])
                assert ask(qi, k) == plain and ask(qi, k, fusion=None) == plain
            # with a payload filter ("filter":"match": a resident filter's id goes to the engine)
            allow = np.arange(n) % 3 == 1
            got = ask(4, 9, filter={"doc": "d1"}, fusion={"queries": Q[4, 1:4].tolist(),
                                                          "prefetch_limit": 48})
            assert got == want(FR.rrf(_lists(S[4, :4], 48, allow), 9))
            # "method" defaults to rrf, prefetch_limit to min(4 top_k, 128)
            assert ask(5, 5, fusion={"queries": Q[5, 1:3].tolist()}) == want(FR.rrf(_lists(S[5, :3], 20), 5))
            # bad requests: nothing is searched
            one = [Q[0, 1].tolist()]
            for bad in ({"fusion": 3}, {"fusion": {"queries": []}}, {"fusion": {"queries": one * 8}},
                        {"fusion": {"queries": one, "prefetch_limit": 129}},
                        {"fusion": {"queries": one, "method": "dbsf", "rrf_k": 2}},
                        {"fusion": {"queries": one}, "mmr": {}}):
                st, body = _post(lis.port, "/search", dict(collection="tern", query=Q[0, 0].tolist(),
                                                           top_k=5, **bad))
                assert st == 400 and json.loads(body) == {"error": "Invalid request body"}, bad
            st, body = _post(lis.port, "/search", dict(collection="tern", query=Q[0, 0].tolist(),
                                                       top_k=129, fusion={"queries": one}))
            assert st == 400, body
    finally:
        s.close()
        eng.close()
