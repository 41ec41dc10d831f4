#!/bin/bash
# Headline evidence on one box: rocprofv3 kernel stats of one batch, then the whole bench
# (20 timed steps + 5 warm-up, --full: latency points, search latency).  Results go to $OUT.
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
rm -rf "$OUT/prof"
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- \
  python bench.py --steps 1 --warmup 0 > "$OUT/prof_bench.log" 2>&1 || { tail -5 "$OUT/prof_bench.log"; exit 1; }
python scripts/prof_summary.py "$OUT/prof" "$OUT/prof_full_bench.txt" > /dev/null
find "$OUT/prof" -name '*kernel_trace.csv' -delete
head -16 "$OUT/prof_full_bench.txt" | cut -c1-150
timeout -k 10 650 python -u bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/bench_20steps.out" 2> "$OUT/bench_20steps.err" || { tail -5 "$OUT/bench_20steps.err"; exit 1; }
tail -1 "$OUT/bench_20steps.out"
