"""Sequence scoring: the one-pass call (ymt3_score_tokens, YourMT3.decode_score) against the sequential route that was the only one before
it, decode(forced=ids, return_scores=True), on ONE handle.  BASELINE configs[1] shapes (256 frames, dense FFN), two workloads: 64 segments
x 1024 tokens and 8 segments x 256 tokens.  Per workload: both calls warmed up (graphs captured, code objects loaded), then REPS
interleaved repetitions timed with a host clock around a device synchronise; medians.  The scores of the two routes are compared at the
sizes timed.  Then ONE `rocprofv3 --kernel-trace --stats` run of a fresh child process (this script with --trace: the one-pass call only,
at 64 x 1024) gives the per-kernel share; the attention and lm_head kernels' time is set against their own rooflines (operations and
bytes from the shapes, peaks: 2.5 PFLOP/s dense bf16 MFMA, 8 TB/s HBM).  Output: JSON (profiles/score_pass_bench.json)."""
import csv, dataclasses, glob, json, os, socket, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from yourmt3_amd.config import baseline_config
from yourmt3_amd.model import YourMT3
from yourmt3_amd.audio import synthetic_segments

REPS = int(os.environ.get("REPS", 5))
SHAPES = [(64, 1024), (8, 256)]
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12
cfg = dataclasses.replace(baseline_config(1), eos_id=-1)
m = YourMT3(cfg, max_batch=64)
audio = torch.from_numpy(synthetic_segments(64, cfg.segment_samples)).cuda()
enc = m.encode(m.logmel(audio))
g = torch.Generator().manual_seed(0)
ids_all = torch.randint(0, cfg.vocab, (64, 1, 1024), generator=g, dtype=torch.int32).cuda()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


if "--trace" in sys.argv:                                   # the child under rocprofv3: the one-pass call alone
    for _ in range(3):
        m.decode_score(enc, ids_all)
    torch.cuda.synchronize()
    m.close()
    sys.exit(0)

res = {}
for B, n in SHAPES:
    e, ids = enc[:B].contiguous(), ids_all[:B, :, :n].contiguous()
    seq = lambda: m.decode(e, n, forced=ids, return_scores=True)[1]
    one = lambda: m.decode_score(e, ids)
    t_seq, t_one = [], []
    for rep in range(REPS + 2):                             # (the first two passes warm up)
        ts, s_seq = wall(seq)
        to, s_one = wall(one)
        if rep >= 2:
            t_seq.append(ts)
            t_one.append(to)
    d = (s_one - s_seq).abs()
    ms_seq, ms_one = 1e3 * float(np.median(t_seq)), 1e3 * float(np.median(t_one))
    res[f"{B}_segments_x_{n}_tokens"] = {
        "sequential_decode_forced_ms": round(ms_seq, 3), "sequential_ms_all": [round(1e3 * x, 3) for x in t_seq],
        "one_pass_decode_score_ms": round(ms_one, 3), "one_pass_ms_all": [round(1e3 * x, 3) for x in t_one],
        "ratio_sequential_over_one_pass": round(ms_seq / ms_one, 2), "one_pass_is_faster": bool(ms_one < ms_seq),
        "scores_abs_difference": {"max": round(float(d.max()), 5), "mean": round(float(d.mean()), 6)},
        "tokens_per_s_one_pass": round(B * n / (ms_one * 1e-3)),
    }
m.close()

# per-kernel share of the one-pass call at 64 x 1024: one profiler run of a fresh process
kernels, note = [], None
with tempfile.TemporaryDirectory() as td:
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable,
                        os.path.abspath(__file__), "--trace"], capture_output=True, text=True, timeout=400)
    files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        note = f"rocprofv3 run failed (exit {r.returncode}): {r.stderr[-300:]}"
    else:
        rows = list(csv.DictReader(open(files[0])))
        total = sum(float(x["TotalDurationNs"]) for x in rows)
        for x in rows:
            name = x["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            kernels.append({"kernel": name, "calls": int(x["Calls"]), "total_ms": round(float(x["TotalDurationNs"]) / 1e6, 3),
                            "average_us": round(float(x["AverageNs"]) / 1e3, 2), "share_percent": round(100 * float(x["TotalDurationNs"]) / total, 2)})
        kernels.sort(key=lambda k: -k["total_ms"])

# rooflines of the new kernels at 64 x 1024 (per call of the kernel: one chunk of 16 rows x 1024 positions, act_rows = 64 x 256)
B, n = SHAPES[0]
rows_chunk = (64 * cfg.n_frames) // n
H, T, V, d = cfg.n_heads, cfg.n_frames, cfg.vocab, cfg.d_model
roof = {
    "dec_seq_attn_kernel<true>": {            # causal: half of the n x n scores (plus the diagonal tiles), QK^T and PV
        "flops": rows_chunk * H * 4 * 64 * n * (n + 64) / 2, "bytes": rows_chunk * n * (3 + 1) * H * 64 * 2},
    "dec_seq_attn_kernel<false>": {
        "flops": rows_chunk * H * 4 * 64 * n * T, "bytes": rows_chunk * n * 2 * H * 64 * 2 + rows_chunk * 2 * H * T * 64 * 2},
    "seq_lm_head_score_kernel": {
        "flops": 2.0 * rows_chunk * n * V * d, "bytes": rows_chunk * n * (d * 2 + 8) + V * d * 2},
}
for k in kernels:
    for name, rf in roof.items():
        if k["kernel"].replace(" ", "") == name.replace(" ", ""):
            floor_us = 1e6 * max(rf["flops"] / PEAK_FLOPS, rf["bytes"] / PEAK_BYTES)
            k["roofline"] = {"flops": rf["flops"], "bytes": rf["bytes"], "bound": "MFMA" if rf["flops"] / PEAK_FLOPS > rf["bytes"] / PEAK_BYTES else "HBM",
                             "floor_us": round(floor_us, 2), "achieved_fraction": round(floor_us / k["average_us"], 4),
                             "achieved_tflops": round(rf["flops"] / (k["average_us"] * 1e-6) / 1e12, 1)}

print(json.dumps({
    "box": f"{socket.gethostname()}: {torch.cuda.get_device_name(0)}",
    "workload": f"BASELINE configs[1] shapes ({T} frames, dense FFN, vocab {V}), one handle (max_batch 64), random ids, {REPS} interleaved "
                "repetitions after 2 warm-up passes, medians; host clock around a device synchronise",
    "runs": res,
    "one_pass_kernels_64x1024": kernels,
    "profiler": note or "one rocprofv3 --kernel-trace --stats run of a fresh process: 3 one-pass calls at 64 x 1024 (plus the set-up's log-mel and encoder)",
    "peaks_used": {"bf16_mfma_flops": PEAK_FLOPS, "hbm_bytes_per_s": PEAK_BYTES},
}, indent=1))
