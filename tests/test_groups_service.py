"""/search's "group_by" / "group_size" in the service layer
(include/vsearch_service.h), on CPU.

The real handler code (csrc/service/*.cpp) runs over a CPU test double of the
engine C-ABI: tests/groups/fake_engine_groups.cpp, which is the MMR tests'
double plus vs_grouping_create / vs_grouping_drop / vs_search_groups by the
header's rule, with a log of every such call. The log is how the tests see
WHICH engine calls a request became. The 501 case links the same handlers
against the old double, which lacks the symbols (they are referenced weakly).
The GPU run over the HIP engine is tests/test_groups_http_gpu.py.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import groups_ref as G
from test_delete_service import CLANG, CONFIG, DIM, FAKE_OLD, ROOT, SOURCES, SVC, _Svc, _uuid
from test_mmr_service import _build, _calls, _noq

FAKE = os.path.join(ROOT, "tests", "groups", "fake_engine_groups.cpp")
DRIVER = os.path.join(ROOT, "tests", "groups", "tsan_groups_driver.cpp")
N = 96
RNG = np.random.default_rng(31)
VECS = RNG.standard_normal((N + 40, DIM)).astype(np.float32)
QUERY = RNG.standard_normal(DIM).astype(np.float32)


def _payload(i):
    p = {"text": f"chunk {i}", "page": i % 7}
    if i % 10 == 3:
        return p                                   # no document_id: no group
    p["document_id"] = [f"doc-{i // 6}", {"x": 1}, 2.5, True, None][0 if i % 10 != 7 else 1 + (i // 10) % 4]
    return p                                       # every i % 10 == 7: a type that is no group


def _point(i):
    return {"id": _uuid(i), "vector": [float(x) for x in VECS[i]], "payload": _payload(i)}


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("grpsvc")
    new = _build(d, "libvsvc_grp.so", FAKE)
    new.fake_calls.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    new.fake_calls.restype = ctypes.c_size_t
    new.fake_stale_groupings.restype = ctypes.c_uint64
    return {"new": new, "old": _build(d, "libvsvc_old.so", FAKE_OLD)}


def _open(L, n=N, **cfg):
    s = _Svc(L, dict(CONFIG, **cfg))
    st, body, _ = s.handle("POST", "/upsert", {"collection": "docs",
                                               "points": [_point(i) for i in range(n)]})
    assert st == 200, body
    _calls(L)
    return s


@pytest.fixture()
def svc(libs):
    s = _open(libs["new"])
    yield s
    s.close()


def _body(k=5, **extra):
    return dict(collection="docs", top_k=k, query=[float(x) for x in QUERY], **extra)


def _want(n, key, limit, size, allow=None):
    """The header's rule over the stored (normalised) rows, in float64:
    [(payload value, [row, ...]), ...]."""
    X = VECS[:n].astype(np.float64)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    s = X @ (QUERY.astype(np.float64) / np.linalg.norm(QUERY.astype(np.float64)))
    values, gor = [], np.full(n, G.GROUP_NONE, np.uint32)
    for r in range(n):
        v = _payload(r).get(key)
        if (isinstance(v, str) or (isinstance(v, int) and not isinstance(v, bool))) and \
                (allow is None or allow[r]):
            if v not in values:
                values.append(v)
            gor[r] = values.index(v)
    order = np.lexsort((np.arange(n), -s))
    keys = G.make_keys(G.score_image(s[order].astype(np.float32)), order)
    # distinct fp32 images are not needed: the row word breaks equal images as the rule does
    ref = G.groups_ref(keys, gor, limit, size)
    return [(values[g], [int(G.key_rows(np.uint64(k))) for k in ks]) for g, ks in ref]


def _assert_reply(out, want):
    res = json.loads(out)
    assert list(res) == ["results", "count", "groups"]
    assert res["groups"] == [{"id": v, "hits": len(rows)} for v, rows in want]
    flat = [r for _, rows in want for r in rows]
    assert res["count"] == len(flat) == len(res["results"])
    assert [h["id"] for h in res["results"]] == [_uuid(r) for r in flat]
    for h, r in zip(res["results"], flat):
        assert h["payload"] == _payload(r)
    return res


def test_group_request_is_one_engine_call_past_the_batcher(svc):
    st, out, ct = svc.handle("POST", "/search", _body(4, group_by="document_id", group_size=3))
    assert st == 200 and ct == "application/json", out
    log = _calls(svc.L)
    assert len(log) == 2, log
    rows_with_group = sum(1 for i in range(N) if isinstance(_payload(i).get("document_id"), str))
    groups = len({_payload(i)["document_id"] for i in range(N)
                  if isinstance(_payload(i).get("document_id"), str)})
    assert rows_with_group < N
    gid = log[0].rsplit("id=", 1)[1]
    assert log[0] == f"vs_grouping_create docs rows={N} groups={groups} id={gid}" and int(gid) >= 1
    assert log[1].startswith("vs_search_groups docs nq=1 dim=16 k=4 ") and \
        log[1].endswith(f" S=3 grouping={gid} filter=0"), log
    res = _assert_reply(out, _want(N, "document_id", 4, 3))
    # group order: the groups' best scores fall; inside a group the scores fall
    heads, at = [], 0
    for g in res["groups"]:
        sc = [h["score"] for h in res["results"][at:at + g["hits"]]]
        assert sc == sorted(sc, reverse=True)
        heads.append(sc[0])
        at += g["hits"]
    assert heads == sorted(heads, reverse=True)
    # rows lacking the key, or holding a value that is no group, never appear
    st, out, _ = svc.handle("POST", "/search", _body(128, group_by="document_id", group_size=16))
    ids = {h["id"] for h in json.loads(out)["results"]}
    assert ids == {_uuid(i) for i in range(N) if isinstance(_payload(i).get("document_id"), str)}
    assert svc.L.fake_stale_groupings() == 0


def test_grouping_is_cached_and_rebuilt_after_upsert_and_delete(svc):
    L = svc.L
    for _ in range(2):
        assert svc.handle("POST", "/search", _body(3, group_by="document_id"))[0] == 200
    log = [_noq(x) for x in _calls(L)]
    create = [x for x in log if x.startswith("vs_grouping_create")]
    searches = [x for x in log if x.startswith("vs_search_groups")]
    assert len(create) == 1 and len(searches) == 2 and len(log) == 3, log
    gid = create[0].rsplit("id=", 1)[1]
    assert all(x.endswith(f" S=1 grouping={gid} filter=0") for x in searches)   # group_size: 1
    # another key: another grouping, the first one kept
    st, out, _ = svc.handle("POST", "/search", _body(7, group_by="page", group_size=2))
    assert st == 200
    log = _calls(L)
    assert [x.split()[0] for x in log] == ["vs_grouping_create", "vs_search_groups"], log
    _assert_reply(out, _want(N, "page", 7, 2))         # integer keys, as given
    assert svc.handle("POST", "/search", _body(3, group_by="document_id"))[0] == 200
    assert [x.split()[0] for x in _calls(L)] == ["vs_search_groups"]
    # /upsert: the next grouped search rebuilds (and the stale ones are let go)
    more = [_point(i) for i in range(N, N + 12)]
    assert svc.handle("POST", "/upsert", {"collection": "docs", "points": more})[0] == 200
    _calls(L)
    st, out, _ = svc.handle("POST", "/search", _body(5, group_by="document_id", group_size=2))
    log = _calls(L)
    names = [x.split()[0] for x in log]
    assert names.count("vs_grouping_create") == 1 and names[-1] == "vs_search_groups", log
    assert f"rows={N + 12}" in [x for x in log if x.startswith("vs_grouping_create")][0]
    assert names.index("vs_grouping_create") < names.index("vs_search_groups")
    _assert_reply(out, _want(N + 12, "document_id", 5, 2))
    # /delete: rebuilt again, over the renumbered rows
    st, out, _ = svc.handle("POST", "/delete", {"collection": "docs",
                                                "ids": [_uuid(i) for i in range(N, N + 12)]})
    assert st == 200 and json.loads(out)["deleted"] == 12
    _calls(L)
    st, out, _ = svc.handle("POST", "/search", _body(4, group_by="document_id", group_size=3))
    log = _calls(L)
    assert [x.split()[0] for x in log if not x.startswith("vs_grouping_drop")] == \
        ["vs_grouping_create", "vs_search_groups"], log
    _assert_reply(out, _want(N, "document_id", 4, 3))   # the tail was deleted: rows as before
    assert L.fake_stale_groupings() == 0


@pytest.mark.parametrize("extra", [{"group_by": []}, {"group_by": 3}, {"group_by": True},
                                   {"group_by": {"k": "v"}},
                                   {"group_by": "document_id", "group_size": "2"},
                                   {"group_by": "document_id", "group_size": 0},
                                   {"group_by": "document_id", "group_size": 17},
                                   {"group_by": "document_id", "group_size": -1},
                                   {"group_by": "document_id", "group_size": 2.5},
                                   {"group_by": "document_id", "group_size": [2]},
                                   {"group_by": "document_id", "group_size": 1 << 40},
                                   {"group_size": 99},
                                   {"group_by": "document_id", "mmr": {}},
                                   {"group_by": "document_id", "mmr": {"diversity": 0.3}}])
def test_malformed_group_fields_are_a_bad_request(svc, extra):
    body = json.dumps(_body(5, **extra)).encode()
    st, out, ct = svc.handle("POST", "/search", body)
    assert (st, out, ct) == (400, b'{"error":"Invalid request body"}\n', "application/json"), extra
    assert _calls(svc.L) == []   # nothing reached the engine
    # vsvc_validate agrees, and names the first error
    msg = ctypes.c_void_p()
    svc.L.vsvc_validate.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_void_p)]
    assert svc.L.vsvc_validate(b"/search", body, len(body), ctypes.byref(msg)) == 400
    text = ctypes.string_at(msg.value).decode()
    svc.L.vsvc_free(msg)
    assert text.startswith("group_by: ") or text.startswith("group_size: "), text


def test_limits_and_statuses(libs):
    s = _open(libs["new"], n=N + 40)
    try:
        st, out, _ = s.handle("POST", "/search", _body(129, group_by="document_id"))
        assert st == 400 and json.loads(out)["error"] == "top_k must not exceed 128 with group_by"
        assert _calls(libs["new"]) == []
        st, out, _ = s.handle("POST", "/search", _body(128, group_by="document_id"))
        assert st == 200 and len(json.loads(out)["groups"]) == \
            len(_want(N + 40, "document_id", 128, 1))
        _calls(libs["new"])
        # as a plain /search answers them
        assert s.handle("POST", "/search", _body(-1, group_by="document_id"))[0] == 400
        bad = _body(5, group_by="document_id")
        bad["query"] = bad["query"][:3]
        assert s.handle("POST", "/search", bad) == s.handle(
            "POST", "/search", {k: v for k, v in bad.items() if k != "group_by"})
        assert s.handle("POST", "/search", dict(_body(5, group_by="x"), collection="nope"))[0] == 500
        assert s.handle("GET", "/search")[0] == 405
        # a key nobody has: no groups, an empty answer
        st, out, _ = s.handle("POST", "/search", _body(5, group_by="nobody"))
        assert st == 200 and json.loads(out) == {"results": [], "count": 0, "groups": []}
        # bulk-generated points have no payloads
        assert libs["new"].vsvc_bulk_generate(s.svc, b"bulk", 50, 1) == 0
        q = dict(_body(5, group_by="document_id"), collection="bulk")
        st, out, _ = s.handle("POST", "/search", q)
        assert st == 400 and json.loads(out)["error"] == "collection holds bulk-generated points"
    finally:
        s.close()


def test_request_without_group_by_is_unchanged(libs):
    for batching in (True, False):
        s = _open(libs["new"], batching={"enabled": batching, "max_batch": 64})
        try:
            st, plain, _ = s.handle("POST", "/search", _body(8))
            first = _calls(libs["new"])
            assert st == 200 and len(first) == 1
            q = first[0].split(" q=")[1]
            assert first[0] == f"vs_search docs nq=1 dim=16 k=8 q={q}", first
            assert list(json.loads(plain)) == ["results", "count"]
            for extra in ({"group_by": None}, {"group_by": None, "group_size": None},
                          {"group_size": 4}):
                st, again, _ = s.handle("POST", "/search", _body(8, **extra))
                assert st == 200 and again == plain and _calls(libs["new"]) == first, extra
            # the grouped request carries the same query bytes to the engine
            assert s.handle("POST", "/search", _body(8, group_by="document_id"))[0] == 200
            assert _calls(libs["new"])[-1].split(" q=")[1].split()[0] == q
        finally:
            s.close()


def test_group_by_with_a_payload_filter(libs):
    s = _open(libs["new"], filter="match")
    try:
        st, out, _ = s.handle("POST", "/search", _body(6, filter={"page": 2},
                                                      group_by="document_id", group_size=4))
        assert st == 200, out
        log = _calls(libs["new"])
        line = [x for x in log if x.startswith("vs_search_groups")]
        assert len(line) == 1 and not line[0].endswith("filter=0"), log
        allow = np.array([i % 7 == 2 for i in range(N)])
        _assert_reply(out, _want(N, "document_id", 6, 4, allow))
    finally:
        s.close()
    s = _open(libs["new"])   # "filter":"ignore", the default: dropped, as for plain search
    try:
        st, out, _ = s.handle("POST", "/search", _body(6, filter={"page": 2},
                                                      group_by="document_id", group_size=4))
        assert st == 200 and _calls(libs["new"])[-1].endswith(" filter=0")
        _assert_reply(out, _want(N, "document_id", 6, 4))
    finally:
        s.close()


def test_501_without_the_engine_symbols(libs):
    s = _Svc(libs["old"])
    try:
        st, body, _ = s.handle("POST", "/upsert", {"collection": "docs",
                                                   "points": [_point(i) for i in range(6)]})
        assert st == 200, body
        st, out, _ = s.handle("POST", "/search", _body(3, group_by="document_id"))
        assert st == 501 and "error" in json.loads(out)
        assert s.handle("POST", "/search", _body(3, group_by=7))[0] == 400   # request checks first
        assert len(s.search(QUERY, 3)) == 3                                   # plain search is served
        assert len(json.loads(s.handle("POST", "/search", _body(3, group_by=None))[1])["results"]) == 3
    finally:
        s.close()


def test_groups_under_tsan(tmp_path):
    """Grouped searches race /upsert and /delete on one collection: every answer
    belongs to one version and no stale grouping id reaches the engine
    (tests/groups/tsan_groups_driver.cpp states the checks). A stand-alone
    program; pass = exit 0 and no TSAN report."""
    exe = str(tmp_path / "tsan_groups_driver")
    subprocess.run([CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=thread", "-pthread", "-I" + SVC,
                    *SOURCES, FAKE, DRIVER, "-o", exe], check=True, capture_output=True,
                   timeout=600)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    res = subprocess.run([exe, "8", "90"], capture_output=True, text=True, timeout=300, env=env)
    out = res.stdout + res.stderr
    assert "ThreadSanitizer" not in out, out[-4000:]
    assert res.returncode == 0, out[-4000:]
    assert "ok 8 threads" in res.stdout
