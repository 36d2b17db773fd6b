#!/bin/bash
# round 2 evidence pass: parity suite, headline bench line, rocprofv3 per-kernel stats of the same command, all BASELINE configs
set -o pipefail
OUT=${OUT:-results}      # where this pass writes its logs and lines
mkdir -p "$OUT"
timeout -k 10 1100 python -m pytest tests -m gpu -x -q > "$OUT"/pytest_gpu.log 2>&1; echo "pytest exit=$?"
tail -4 "$OUT"/pytest_gpu.log
timeout -k 10 600 python bench.py --full > "$OUT"/r02_bench_line.json 2> "$OUT"/bench.err; echo "bench exit=$?"
python -c "import json; d=json.loads(open('$OUT/r02_bench_line.json').read().strip().splitlines()[-1]); print({k: d[k] for k in ('value','ms_per_step','p50_segment_latency_ms')}, d['roofline']['frac'], d['roofline_path']['frac'], (d['roofline_kernels']['cross_attn'] or {}).get('frac'), d['mfma_util']['encoder_whole'], d['cpu_baseline']['value'])"
export TMPDIR=/tmp
rm -rf "$OUT"/prof
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > "$OUT"/prof_bench.log 2>&1; echo "rocprof exit=$?"
f=$(find "$OUT"/prof -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT"/r02_bench_kernel_stats.csv; cut -d, -f1-4,7 "$f" | head -14 | cut -c1-170; rm -rf "$OUT"/prof
timeout -k 10 600 python scripts/gpu_configs.py > "$OUT"/r02_all_configs.json 2> "$OUT"/all_configs.err; echo "configs exit=$?"; cat "$OUT"/r02_all_configs.json
