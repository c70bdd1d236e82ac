#!/usr/bin/env python3
"""What grouped search costs at C3's shape (DESIGN.md "Grouped search"):
10M x 768 bf16 rows, one query, limit = 10 groups of group_size = 3, at three
id layouts: document-like (contiguous runs, mean 40 rows), one group per row,
and a single group holding every row.

    python tools/groups_bench.py --out profiles/groups_c3.json

Per layout, from one process and one build:
  * host latency of search_groups beside search(k = 1025) -- the cheapest exact
    path with the same score pass, which is existing code this change does not
    touch, and what a caller pays today before regrouping on the host -- taken
    in alternation over fresh queries (host clocks around calls that end in a
    device synchronise);
  * device time of the score pass and of the group stages together, from an
    engine opened with VS_FLAG_TIMING | VS_FLAG_TIMING_MERGE;
  * device time of each group stage (HIP events around the launchers, through
    the test shim lib/libvs_kprobe_groups.so) on score images with the
    distribution the score pass leaves for this corpus: cosines of random unit
    vectors, N(0, 1/768).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIM, SEED, LIMIT, SIZE, K_PLAIN = 768, 0x5EED, 10, 3, 1025


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "p10_ms": round(ms[len(ms) // 10], 4),
            "p90_ms": round(ms[(len(ms) * 9) // 10], 4), "steps": len(ms)}


def _layouts(n, rng):
    lens = rng.integers(1, 80, n // 40 + 1000)   # mean 40
    doc = np.repeat(np.arange(lens.size, dtype=np.uint32), lens)[:n]
    assert doc.size == n
    return {"documents": (doc, int(doc.max()) + 1),
            "own_group": (np.arange(n, dtype=np.uint32), n),
            "one_group": (np.zeros(n, np.uint32), 1)}


def _stages(torch, kg, sc, gor, ng, steps, warmup):
    """Median device ms of every stage launch, in the engine's order."""
    n = sc.numel()
    L, T = kg.group_lists(n), LIMIT * SIZE
    z64 = lambda m: torch.zeros(m, dtype=torch.int64, device="cuda")
    d_gid = torch.from_numpy(gor.view(np.int32)).cuda()
    best, lists, heads, out = z64(ng), z64(L * max(T, LIMIT)), z64(LIMIT), z64(T)
    groups = torch.zeros(LIMIT, dtype=torch.int32, device="cuda")
    hist = torch.zeros(kg.rsel_bins, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    calls = [
        ("group_best", lambda: kg.group_best(p(sc), p(d_gid), n, 0, ng, p(best), p(hist))),
        ("group_heads", lambda: kg.group_heads(p(sc), p(d_gid), p(best), n, 0, ng, LIMIT, p(lists))),
        ("merge_heads", lambda: kg.merge(p(lists), L, LIMIT, 0, 1, LIMIT, LIMIT, p(heads))),
        ("group_members", lambda: kg.group_members(p(sc), p(d_gid), p(best), n, 0, ng, p(heads),
                                                   LIMIT, SIZE, p(lists), p(groups))),
        ("merge_members", lambda: kg.merge(p(lists), L, T, SIZE, LIMIT, SIZE, SIZE, p(out))),
        ("group_clear", lambda: kg.group_clear(p(best), ng)),
    ]
    ms = {name: [] for name, _ in calls}
    for i in range(warmup + steps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        evs[0].record()
        for j, (_, fn) in enumerate(calls):
            kg.check(fn())
            evs[j + 1].record()
        evs[-1].synchronize()
        if i >= warmup:
            for j, (name, _) in enumerate(calls):
                ms[name].append(evs[j].elapsed_time(evs[j + 1]))
    return {name: round(statistics.median(v), 4) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from kprobe import groups as kgroups
    from oracle import oracle as orc
    pkg = ge.load_package()
    kg = kgroups.load()
    rng = np.random.default_rng(1)
    Q = orc.generate(orc.SEED_QUERY, 0, 64, DIM)
    layouts = _layouts(a.rows, rng)
    res = {"build_id": pkg.build_id(), "rows": a.rows, "dim": DIM, "dtype": "bf16", "metric": "dot",
           "nq": 1, "limit": LIMIT, "group_size": SIZE, "plain_k": K_PLAIN,
           "data": "synthetic unit-norm generator rows (bench.py's C3 corpus), a fresh query a step",
           "plain_search": "search(k = 1025) of this build: code this change does not touch",
           "layouts": {}}
    # the stages on their own: images ~ cosines of random unit vectors
    import groups_ref as G
    sc_np = G.score_image((rng.standard_normal(a.rows) / np.sqrt(DIM)).astype(np.float32))
    sc = torch.from_numpy(sc_np.view(np.int32)).cuda()
    for name, (gor, ng) in layouts.items():
        res["layouts"][name] = {"n_groups": ng,
                                "stage_device_ms": _stages(torch, kg, sc, gor, ng, a.steps, a.warmup)}
    del sc
    with pkg.VectorEngine(device=0, timing=True, timing_merge=True) as eng:
        eng.create_collection("c3", DIM, pkg.METRIC_DOT, pkg.DTYPE_BF16, a.rows)
        eng.generate("c3", a.rows, SEED)
        for name, (gor, ng) in layouts.items():
            gid = eng.grouping_create("c3", gor, ng)
            t = {"search_groups": [], "search_k1025": []}
            dev = {}
            for i in range(a.warmup + a.steps):
                q = Q[i % len(Q)]
                for what, fn in (("search_groups", lambda: eng.search_groups("c3", q, LIMIT, SIZE, gid)),
                                 ("search_k1025", lambda: eng.search("c3", q, K_PLAIN))):
                    if i == a.warmup:
                        eng.timing(reset=True)
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if i >= a.warmup:
                        t[what].append(dt)
                        tm = eng.timing(reset=True)
                        dev.setdefault(what, []).append((tm["scan_ms"], tm["merge_ms"]))
            eng.grouping_drop(gid)
            r = res["layouts"][name]
            r["host"] = {k: _stats(v) for k, v in t.items()}
            for what, v in dev.items():
                r[what + "_device_ms"] = {
                    "score_pass": round(statistics.median(x[0] for x in v), 4),
                    "after_the_score_pass": round(statistics.median(x[1] for x in v), 4)}
            sp = r["search_groups_device_ms"]["score_pass"]
            st = r["stage_device_ms"]
            r["stage_share_of_score_pass"] = {k: round(v / sp, 4) for k, v in st.items()}
            r["groups_minus_k1025_ms"] = round(r["host"]["search_groups"]["median_ms"] -
                                               r["host"]["search_k1025"]["median_ms"], 4)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
