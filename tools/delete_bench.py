#!/usr/bin/env python3
"""vs_delete on 1M x 768 bf16 rows with an int8 copy: what a delete of a random
1% costs, and whether the 256-query batch step afterwards is the step of a
freshly generated collection of the same size (DESIGN.md §8 "Delete").

    python tools/delete_bench.py --out profiles/delete_1m.json          # profiler off
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o run -- \\
        python tools/delete_bench.py --profile-run                      # one delete, traced
    python tools/delete_bench.py --split DIR --out profiles/delete_1m_phases.json

End-to-end numbers are host clocks around calls that end in a device
synchronise, taken with the profiler off. The phase split (plan, move,
requantise, D2H) comes from the traced run: the kernels and copies of the
last delete in the trace, summed per phase by kernel name and order.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, DIM, SEED, NQ, K = 1_000_000, 768, 0x5EED, 256, 10


def _setup():
    import __graft_entry__ as ge
    from oracle import oracle
    pkg = ge.load_package()
    return pkg, oracle


def _delete_rows(rng):
    return rng.choice(N, N // 100, replace=False).astype(np.uint64)


def _step_ms(eng, name, Q, steps):
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        eng.search(name, Q, K)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def run(a):
    pkg, orc = _setup()
    Q = orc.generate(orc.SEED_QUERY, 0, NQ, DIM)
    res = {"build_id": pkg.build_id(), "rows": N, "dim": DIM, "dtype": "bf16", "deleted": N // 100,
           "nq": NQ, "k": K, "delete_ms": [], "rounds": []}
    with pkg.VectorEngine(device=0) as eng:
        # code objects of every delete kernel, on a small collection with an int8 copy
        eng.create_collection("warm", DIM, 1, 1, 80_000)
        eng.generate("warm", 80_000, 1)
        eng.delete("warm", np.arange(0, 80_000, 100))
        eng.drop_collection("warm")
        for r in range(a.rounds):
            rng = np.random.default_rng(100 + r)
            d = _delete_rows(rng)
            eng.create_collection("del", DIM, 1, 1, N)
            eng.generate("del", N, SEED)
            assert eng.prefilter_bytes("del") > 0
            eng.search("del", Q, K)
            t0 = time.perf_counter()
            frm, to = eng.delete("del", d)
            res["delete_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
            nn = eng.collection_info("del")["rows"]
            assert nn == N - len(d)
            eng.create_collection("fresh", DIM, 1, 1, N)
            eng.generate("fresh", nn, SEED + 1)
            for name in ("del", "fresh"):  # warm-up: the speculative bound learns its ratio
                _step_ms(eng, name, Q, a.warmup)
            st0 = {n: eng.spec_stats(n) for n in ("del", "fresh")}
            t = {"del": [], "fresh": []}
            for _ in range(a.windows):  # alternating windows of the two collections
                for name in ("del", "fresh"):
                    t[name] += _step_ms(eng, name, Q, a.steps)
            st1 = {n: eng.spec_stats(n) for n in ("del", "fresh")}
            rec = {"moved": int(len(frm)), "rows_after": int(nn)}
            for name in ("del", "fresh"):
                rec[name] = {"step_ms_median": round(statistics.median(t[name]), 4),
                             "step_ms_p10": round(float(np.percentile(t[name], 10)), 4),
                             "step_ms_p90": round(float(np.percentile(t[name], 90)), 4),
                             "steps": len(t[name]),
                             "prefilter_bytes": eng.prefilter_bytes(name),
                             "spec_tries": st1[name]["tries"] - st0[name]["tries"],
                             "spec_fallbacks": st1[name]["fallbacks"] - st0[name]["fallbacks"],
                             "spec_skipped": st1[name]["skipped"] - st0[name]["skipped"]}
            res["rounds"].append(rec)
            eng.drop_collection("del")
            eng.drop_collection("fresh")
    res["delete_ms_median"] = statistics.median(res["delete_ms"])
    med = {n: [r[n]["step_ms_median"] for r in res["rounds"]] for n in ("del", "fresh")}
    res["step_ms_after_delete"] = statistics.median(med["del"])
    res["step_ms_fresh"] = statistics.median(med["fresh"])
    res["step_ms_spread_fresh"] = round(max(med["fresh"]) - min(med["fresh"]), 4)
    return res


def profile_run():
    pkg, orc = _setup()
    with pkg.VectorEngine(device=0) as eng:
        eng.create_collection("warm", DIM, 1, 1, 80_000)
        eng.generate("warm", 80_000, 1)
        eng.delete("warm", np.arange(0, 80_000, 100))
        eng.create_collection("del", DIM, 1, 1, N)
        eng.generate("del", N, SEED)
        eng.search("del", orc.generate(orc.SEED_QUERY, 0, NQ, DIM), K)
        frm, to = eng.delete("del", _delete_rows(np.random.default_rng(100)))
        print(json.dumps({"build_id": pkg.build_id(), "moved": int(len(frm))}))


def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def split(trace_dir):
    kt = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    mt = sorted(glob.glob(os.path.join(trace_dir, "**", "*memory_copy_trace.csv"), recursive=True))
    if not kt:
        sys.exit("no kernel trace under " + trace_dir)
    ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                 for r in _rows(kt[-1])))
    marks = [i for i, k in enumerate(ks) if "delete_mark_kernel" in k[2]]
    if not marks:
        sys.exit("no delete in the trace")
    seg = ks[marks[-1]:]
    phase = {"plan": 0, "move": 0, "requantise": 0}
    counts = {"plan": 0, "move": 0, "requantise": 0}
    cur = "plan"
    end = seg[0][1]
    for s, e, n in seg:
        if "move_rows_kernel" in n:
            cur = "move"
        elif cur == "move":
            cur = "requantise"
        if cur == "requantise" and not any(x in n for x in ("mark_tiles", "range_", "q8_quantize")):
            break  # the next call's kernels
        phase[cur] += e - s
        counts[cur] += 1
        end = e
    out = {"kernel_us": {p: round(v / 1e3, 2) for p, v in phase.items()}, "launches": counts,
           "device_span_us": round((end - seg[0][0]) / 1e3, 2)}
    if mt:
        d2h = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in _rows(mt[-1])
               if "DEVICE_TO_HOST" in str(r.get("Direction", "")).upper()
               and seg[0][0] <= int(r["Start_Timestamp"]) <= end + 5_000_000]
        out["d2h_us"] = round(sum(e - s for s, e in d2h) / 1e3, 2)
        out["d2h_copies"] = len(d2h)
        out["d2h_note"] = ("vs_delete issues three D2H copies: moved_from, moved_to and a 24-byte "
                           "header of counts. The copy trace lists the two pair arrays only (the "
                           "header copy does not appear in it as a memory copy), so d2h_us is the "
                           "pairs alone.")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--split")
    ap.add_argument("--build-id")
    a = ap.parse_args()
    if a.profile_run:
        return profile_run()
    res = split(a.split) if a.split else run(a)
    if a.split and a.build_id:
        res["build_id"] = a.build_id
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
