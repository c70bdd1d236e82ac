#!/usr/bin/env python3
"""What the MMR selection stage costs at C3's shape (DESIGN.md "MMR search"):
10M x 768 bf16 rows, 256-query batches, k = 10 out of F = 128 candidates.

    python tools/mmr_bench.py --out profiles/mmr_c3.json

Three numbers from one process and one build: the median step of
search_mmr(k, F) beside the median step of search(k = F) -- the candidate
search it runs, which is existing code -- taken in alternation over fresh query
batches (host clocks around calls that end in a device synchronise), and the
selection launch's own device time (HIP events around vs_mmr_keys on the
caller's stream, over candidate lists from vs_search_keys).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, SEED, NQ, K, F, D = 768, 0x5EED, 256, 10, 128, 0.5


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "p10_ms": round(ms[len(ms) // 10], 4),
            "p90_ms": round(ms[(len(ms) * 9) // 10], 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from oracle import oracle as orc
    pkg = ge.load_package()
    batches = [orc.generate(orc.SEED_QUERY, i * NQ, NQ, DIM) for i in range(8)]
    res = {"build_id": pkg.build_id(), "rows": a.rows, "dim": DIM, "dtype": "bf16", "metric": "dot",
           "nq": NQ, "k": K, "candidates_limit": F, "diversity": D,
           "data": "synthetic unit-norm generator rows (bench.py's C3 corpus), fresh batches"}
    with pkg.VectorEngine(device=0) as eng:
        eng.create_collection("c3", DIM, pkg.METRIC_DOT, pkg.DTYPE_BF16, a.rows)
        eng.generate("c3", a.rows, SEED)
        t = {"search_k128": [], "search_mmr": [], "search_k10": []}
        for i in range(a.warmup + a.steps):
            Q = batches[i % len(batches)]
            for name, fn in (("search_k128", lambda: eng.search("c3", Q, F)),
                             ("search_mmr", lambda: eng.search_mmr("c3", Q, K, F, D)),
                             ("search_k10", lambda: eng.search("c3", Q, K))):
                t0 = time.perf_counter()
                fn()
                if i >= a.warmup:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        res["step"] = {k: _stats(v) for k, v in t.items()}
        # the stage alone, on the device
        st = torch.cuda.current_stream().cuda_stream
        d_q = torch.from_numpy(batches[0]).cuda()
        d_cand = torch.zeros((NQ, F), dtype=torch.int64, device="cuda")
        d_out = torch.zeros((NQ, K), dtype=torch.int64, device="cuda")
        eng.search_keys("c3", d_q.data_ptr(), NQ, DIM, F, d_cand.data_ptr(), st)
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.mmr_keys("c3", d_cand.data_ptr(), NQ, F, K, D, d_out.data_ptr(), st)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        res["stage_device"] = _stats(ms)
        bytes_read = NQ * F * DIM * 2
        res["stage_device"]["rows_read_bytes"] = bytes_read
        res["stage_device"]["read_gbps"] = round(bytes_read / (res["stage_device"]["median_ms"] * 1e6), 1)
    s = res["step"]
    res["stage_share_of_candidate_search"] = round(
        res["stage_device"]["median_ms"] / s["search_k128"]["median_ms"], 4)
    res["mmr_minus_k128_ms"] = round(s["search_mmr"]["median_ms"] - s["search_k128"]["median_ms"], 4)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
