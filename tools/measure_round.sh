#!/bin/bash
# Round measurement batch on one MI355X: the default bench line (C3, --full)
# with its CPU baseline and oracle parity, the same bench
# under rocprofv3 (kernel trace + stats; the benched binary's build id in the
# file names), C1 over HTTP for both backends + the dispatch floor, and the
# concurrency-overlap trials; EXTRA="c2 c5b256 ..." adds bench configs; C3=0,
# PMC=0, C1=0, CONC=0 skip those parts (to split the batch over calls). Raw
# output goes to $OUT (default: bench_out/ in the repository, git-ignored);
# tools/collect_round.py copies the records into profiles/. Every GPU step
# has its own limit; the first failure stops it.
#   [OUT=DIR] bash tools/measure_round.sh TAG
set -o pipefail
TAG="${1:-rNN}"
cd "${GRAFT_REPO_ROOT:-$(pwd)}"
R="$PWD"
OUT="${OUT:-$R/bench_out}"
mkdir -p "$OUT"
export TMPDIR=/tmp
if [ "${C3:-1}" = 1 ]; then
  timeout -k 10 400 python -u bench.py --full > "$OUT/${TAG}_bench_c3.json" 2> "$OUT/${TAG}_bench_c3.err" || exit 1
  cat "$OUT/${TAG}_bench_c3.json"
  cd /tmp
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/${TAG}_prof_c3" -o run --output-format csv \
    -- python3 "$R/bench.py" --full --no-cpu-baseline > "$OUT/${TAG}_prof_c3.json" 2> "$OUT/${TAG}_prof_c3.err" || exit 1
  cd "$R"
fi
if [ "${PMC:-1}" = 1 ]; then
  # counters in passes of their own (no trace domains), each under a hard limit:
  # HBM bytes of the C3 main pass and the C3 single-query scan, then the MFMA
  # pipe's busy cycles and the clock of the C3 main pass
  B="--steps 10 --warmup 3 --no-cpu-baseline"
  cd /tmp
  timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d "$OUT/${TAG}_pmc_fetch_c3" -o run --output-format csv \
    -- python3 "$R/bench.py" $B --no-secondary > "$OUT/${TAG}_pmc_fetch_c3.log" 2>&1 || exit 1
  timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d "$OUT/${TAG}_pmc_fetch_c3b1" -o run --output-format csv \
    -- python3 "$R/bench.py" $B --config c3b1 > "$OUT/${TAG}_pmc_fetch_c3b1.log" 2>&1 || exit 1
  # (r05) the int8 pass at the N = 8 share's size (rows_per_gpu 1.25M)
  timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d "$OUT/${TAG}_pmc_fetch_c3_s125" -o run --output-format csv \
    -- python3 "$R/bench.py" $B --no-secondary --rows 1250000 > "$OUT/${TAG}_pmc_fetch_c3_s125.log" 2>&1 || exit 1
  timeout -s KILL 120 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES \
    -d "$OUT/${TAG}_pmc_mfma_c3" -o run --output-format csv \
    -- python3 "$R/bench.py" $B --no-secondary > "$OUT/${TAG}_pmc_mfma_c3.log" 2>&1 || exit 1
  cd "$R"
fi
for c in ${EXTRA:-}; do
  timeout -k 10 400 python -u bench.py --full --config "$c" --no-cpu-baseline > "$OUT/${TAG}_bench_$c.json" 2> "$OUT/${TAG}_bench_$c.err" || exit 1
  cat "$OUT/${TAG}_bench_$c.json"
done
if [ "${C1:-1}" = 1 ]; then
  timeout -k 10 300 python -u tools/c1_http.py --backend both --seconds 3 > "$OUT/${TAG}_c1_http.jsonl" 2> "$OUT/${TAG}_c1_http.err" || exit 1
  cat "$OUT/${TAG}_c1_http.jsonl"
  timeout -k 10 120 tools/rt_floor > "$OUT/${TAG}_rt_floor.json" 2> "$OUT/${TAG}_rt_floor.err" || exit 1
  cat "$OUT/${TAG}_rt_floor.json"
fi
if [ "${CONC:-1}" = 1 ]; then
  timeout -k 10 200 python -u tools/concurrency_overlap.py --out "$OUT/${TAG}_concurrency_overlap.json" > "$OUT/${TAG}_conc.out" 2>&1 || exit 1
  tail -1 "$OUT/${TAG}_conc.out"
fi
