"""Beam search under continuous batching (ymt3_transcribe_stream_beam) against lock-step beam batches on a queue of segments whose
groups are done at different lengths.  BASELINE configs[1] shapes, 256 synthetic segments, W = 4, 16 slots (64 rows), L = 1024.  The EOS id
is chosen by scripts/gpu_stream_bench.py's rule from a free-running greedy decode.  Three interleaved repetitions of: lock-step batches of
16 at full length, the same with ymt3_set_early_stop(8), the stream at intervals 4, 8, 16 and 32.  Launched steps come from
ymt3_last_decode_steps; the admission work of a refill (log-mel, encoder, cross-K/V) is timed by itself so that the stream's time per
launched step can be set against the lock-step one.  Output: JSON (profiles/beam_stream_bench.json)."""
import dataclasses, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from yourmt3_amd.config import baseline_config
from yourmt3_amd.model import YourMT3
from yourmt3_amd.audio import synthetic_segments

N, W, SLOTS, REPS = int(os.environ.get("N_SEGMENTS", 256)), 4, 16, 3
base = baseline_config(1)
L = base.max_decode_len
audio = torch.from_numpy(synthetic_segments(N, base.segment_samples)).cuda()

free = YourMT3(dataclasses.replace(base, eos_id=-1), max_batch=SLOTS * W)
toks = np.concatenate(free.inference_file(SLOTS * W, audio), 0).reshape(N, L)
free.close()
best, best_score = None, -1.0
for cand in np.unique(toks):
    hit = toks == cand
    first = np.where(hit.any(1), hit.argmax(1), L)
    score = np.std(first) - abs(first.mean() - L / 3)       # a wide spread of stop lengths with a mean near L / 3
    if score > best_score:
        best, best_score = int(cand), score

cfg = dataclasses.replace(base, eos_id=best)
m = YourMT3(cfg, max_batch=SLOTS * W)
kw = dict(num_beams=W, num_return_sequences=1, length_penalty=1.0)


def lockstep():
    out, steps = [], 0
    for i in range(0, N, SLOTS):
        out.append(m.inference(audio[i:i + SLOTS], **kw).cpu().numpy())
        steps += m.last_decode_steps
    return np.concatenate(out, 0), steps


def stream(interval):
    out = m.inference_stream(audio, slots=SLOTS, interval=interval, **kw).cpu().numpy()
    return out, m.last_decode_steps


def front(bsz):
    """log-mel + encoder of the whole queue in batches of bsz (what a lock-step call runs before its first step, less the cross-K/V GEMM)"""
    for i in range(0, N, bsz):
        m.encode(m.logmel(audio[i:i + bsz]))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


runs = {"lockstep_full_length": lockstep, "lockstep_early_stop_8": lockstep}
for iv in (4, 8, 16, 32):
    runs[f"stream_interval_{iv}"] = (lambda iv=iv: stream(iv))
times = {k: [] for k in runs}
steps, outs = {}, {}
for rep in range(REPS + 1):                                 # (the first pass warms up: graphs are captured, nothing is recorded)
    for name, fn in runs.items():
        m.set_early_stop(8 if name == "lockstep_early_stop_8" else 0)
        t, (out, n) = wall(fn)
        m.set_early_stop(0)
        if rep:
            times[name].append(t)
        steps[name], outs[name] = n, out
ref = outs["lockstep_full_length"]
stops = np.array([int(np.argmax(r == best)) + 1 if (r == best).any() else L for r in ref.reshape(N, L)])

# the admission work, by itself: per segment at the batch sizes refills come in, and the cross-K/V GEMM's shape through the plain GEMM
adm = {}
for bsz in (1, 2, 4, 16):
    front(bsz)
    t_mel, _ = wall(lambda: [m.logmel(audio[i:i + bsz]) for i in range(0, N, bsz)])
    mels = [m.logmel(audio[i:i + bsz]) for i in range(0, N, bsz)]
    t_enc, _ = wall(lambda: [m.encode(x) for x in mels])
    adm[f"batch_{bsz}"] = {"logmel_ms_per_segment": round(1e3 * t_mel / N, 4), "encoder_ms_per_segment": round(1e3 * t_enc / N, 4)}
a_kv = torch.randn(cfg.n_frames, cfg.d_model, device="cuda").bfloat16()
w_kv = torch.randn(cfg.n_dec_layers * 2 * cfg.n_heads * 64, cfg.d_model, device="cuda").bfloat16()
m.test_gemm(a_kv, w_kv)
t_kv, _ = wall(lambda: [m.test_gemm(a_kv, w_kv) for _ in range(N)])
adm["cross_kv_gemm_ms_per_segment"] = round(1e3 * t_kv / N, 4)
t_front16 = min(wall(lambda: front(SLOTS))[0] for _ in range(3))

sec = N * cfg.segment_seconds
full_t = float(np.median(times["lockstep_full_length"]))
step_ms_lock = 1e3 * (full_t - t_front16 - t_kv) / steps["lockstep_full_length"]      # decode time per launched lock-step step
res = {}
for name in runs:
    t = float(np.median(times[name]))
    rec = {"s": round(t, 4), "s_all": [round(x, 4) for x in times[name]], "launched_steps": int(steps[name]),
           "audio_s_per_s": round(sec / t, 1), "ids_equal_lockstep": bool(np.array_equal(outs[name], ref))}
    if name.startswith("stream"):
        rec["ms_per_launched_step"] = round(1e3 * t / steps[name], 4)
        rec["ms_beyond_lockstep_step_rate"] = round(1e3 * t - step_ms_lock * steps[name], 1)
    res[name] = rec
one = adm["batch_1"]
print(json.dumps({
    "workload": f"{N} segments x {cfg.segment_seconds:.3f} s, W = {W}, {SLOTS} slots ({SLOTS * W} rows), L = {L}, eos id {best}, "
                f"{REPS} interleaved repetitions (medians)",
    "stop_length_of_the_best_hypothesis": {"mean": round(float(stops.mean()), 1), "p10": int(np.percentile(stops, 10)),
                                           "p50": int(np.percentile(stops, 50)), "p90": int(np.percentile(stops, 90)), "max": int(stops.max()),
                                           "without_eos": int((stops == L).sum() - ((ref.reshape(N, L)[:, -1] == best).sum()))},
    "runs": res,
    "lockstep_decode_ms_per_step": round(step_ms_lock, 4),
    "front_end_of_the_queue_in_batches_of_16_s": round(t_front16, 4),
    "admission_work": adm,
    "admission_ms_of_the_refills_one_at_a_time": round((N - SLOTS) * (one["logmel_ms_per_segment"] + one["encoder_ms_per_segment"]
                                                                      + adm["cross_kv_gemm_ms_per_segment"]), 1),
}, indent=1))
m.close()
