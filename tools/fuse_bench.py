#!/usr/bin/env python3
"""What the fusion stage costs at C3's shape (DESIGN.md "Fused search"):
10M x 768 bf16 rows, 32 fused queries x 8 rewrites = one 256-query batch,
prefetch_limit F = 128, k = 10.

    python tools/fuse_bench.py --out profiles/fuse_c3.json

From one process and one build: the median step of search_fused(k, F) beside
the median step of search(k = F) over the same 256 queries -- the candidate
search it runs, which is existing code -- taken in alternation over fresh query
batches (host clocks around calls that end in a device synchronise), and the
fusion launch's own device time (HIP events around vs_fuse_keys on the caller's
stream, over candidate lists from vs_search_keys): one launch between two
events, and 20 launches back to back between two events divided by 20, which
leaves the launch gap out.
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

DIM, SEED, NQ, NSUB, K, F, TRAIN = 768, 0x5EED, 32, 8, 10, 128, 20


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
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from oracle import oracle as orc
    pkg = ge.load_package()
    rng = np.random.default_rng(1)

    def rewrites(i):
        """32 questions x 8 rewrites: a generator query plus noise of a third of its norm."""
        base = orc.generate(orc.SEED_QUERY, i * NQ, NQ, DIM)
        noise = rng.standard_normal((NQ, NSUB, DIM)).astype(np.float32) / np.sqrt(DIM) / 3
        return np.ascontiguousarray(base[:, None, :] + noise)

    batches = [rewrites(i) for i in range(8)]
    res = {"build_id": pkg.build_id(), "rows": a.rows, "dim": DIM, "dtype": "bf16", "metric": "dot",
           "nq": NQ, "n_sub": NSUB, "k": K, "prefetch_limit": F,
           "data": "synthetic unit-norm generator rows (bench.py's C3 corpus); fresh batches of "
                   "generator queries, each with 8 noisy rewrites"}
    with pkg.VectorEngine(device=0) as eng:
        eng.create_collection("c3", DIM, pkg.METRIC_DOT, pkg.DTYPE_BF16, a.rows)
        eng.generate("c3", a.rows, SEED)
        t = {"search_k128": [], "search_fused_rrf": [], "search_fused_dbsf": [], "search_k10": []}
        for i in range(a.warmup + a.steps):
            Q = batches[i % len(batches)]
            flat = Q.reshape(NQ * NSUB, DIM)
            for name, fn in (("search_k128", lambda: eng.search("c3", flat, F)),
                             ("search_fused_rrf", lambda: eng.search_fused("c3", Q, K, F)),
                             ("search_fused_dbsf",
                              lambda: eng.search_fused("c3", Q, K, F, pkg.FUSION_DBSF)),
                             ("search_k10", lambda: eng.search("c3", flat, K))):
                t0 = time.perf_counter()
                fn()
                if i >= a.warmup:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        res["step"] = {k: _stats(v) for k, v in t.items()}
        # the stage alone, on the device
        st = torch.cuda.current_stream().cuda_stream
        d_q = torch.from_numpy(batches[0].reshape(NQ * NSUB, DIM)).cuda()
        d_lists = torch.zeros((NQ, NSUB, F), dtype=torch.int64, device="cuda")
        d_out = torch.zeros((NQ, K), dtype=torch.int64, device="cuda")
        eng.search_keys("c3", d_q.data_ptr(), NQ * NSUB, DIM, F, d_lists.data_ptr(), st)
        torch.cuda.synchronize()
        rows = (0xFFFFFFFF - (d_lists.cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF)))
        res["distinct_rows_per_fused_query"] = round(
            float(np.mean([len(np.unique(r)) for r in rows.reshape(NQ, -1)])), 1)
        for label, fusion in (("rrf", pkg.FUSION_RRF), ("dbsf", pkg.FUSION_DBSF)):
            def launch():
                eng.fuse_keys(d_lists.data_ptr(), NQ, NSUB, F, K, fusion, 0, d_out.data_ptr(), st)
            one, train = [], []
            for i in range(a.warmup + a.steps):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                launch()
                e[1].record()
                for _ in range(TRAIN):
                    launch()
                e[2].record()
                e[2].synchronize()
                if i >= a.warmup:
                    one.append(e[0].elapsed_time(e[1]))
                    train.append(e[1].elapsed_time(e[2]) / TRAIN)
            res["stage_device_" + label] = {"one_launch": _stats(one),
                                            "back_to_back_per_launch": _stats(train)}
    s = res["step"]
    res["stage_share_of_candidate_search"] = round(
        res["stage_device_rrf"]["one_launch"]["median_ms"] / s["search_k128"]["median_ms"], 4)
    res["fused_minus_k128_ms"] = round(
        s["search_fused_rrf"]["median_ms"] - s["search_k128"]["median_ms"], 4)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
