#!/bin/bash
# Round 3 evidence pass: in-situ encoder counters (configs[1] and configs[2]), the headline bench line, rocprofv3 kernel stats of the same command
set -o pipefail
OUT=${OUT:-results}      # where this pass writes its logs and lines
mkdir -p "$OUT"
export TMPDIR=/tmp
bash scripts/gpu_r03_pmc_encoder.sh > "$OUT"/r03_pmc_encoder.log 2>&1; echo "pmc encoder exit=$?"; tail -3 "$OUT"/r03_pmc_encoder.log
timeout -k 10 400 python bench.py --full --steps 3 --warmup 1 > "$OUT"/r03_bench.log 2>&1; echo "bench exit=$?"
tail -1 "$OUT"/r03_bench.log > "$OUT"/r03_bench_line.json
rm -rf "$OUT"/prof
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > "$OUT"/r03_prof_bench.log 2>&1; echo "rocprof exit=$?"
find "$OUT"/prof -name "*kernel_stats.csv" | head -1 | xargs -r -I{} cp {} "$OUT"/r03_bench_kernel_stats.csv
rm -rf "$OUT"/prof
head -12 "$OUT"/r03_bench_kernel_stats.csv
python3 -c "import json; d=json.load(open('$OUT/r03_bench_line.json')); print({k: d[k] for k in ('value','ms_per_step','p50_segment_latency_ms')}); print(d['roofline']['frac'], d['roofline_path']['frac'], d['mfma_util']['encoder_whole'])"
