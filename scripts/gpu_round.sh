#!/bin/bash
# One GPU-box pass: parity tests, headline bench, rocprofv3 kernel trace of a shorter bench.
set -o pipefail
OUT=${OUT:-results}      # where this pass writes its logs and lines
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT"/pytest_gpu.log 2>&1; echo "pytest exit=$?"
tail -5 "$OUT"/pytest_gpu.log
timeout -k 10 600 python bench.py --full --steps 3 --warmup 1 > "$OUT"/bench.log 2>&1; echo "bench exit=$?"
tail -3 "$OUT"/bench.log
export TMPDIR=/tmp
rm -rf "$OUT"/prof
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > "$OUT"/prof_bench.log 2>&1; echo "rocprof exit=$?"
tail -2 "$OUT"/prof_bench.log
find "$OUT"/prof -name "*kernel_stats.csv" | head -1 | xargs -r head -30
