"""Per-push overhead of live transcription (include/ymt3.h: streaming ingest, incremental detokeniser; LiveTranscriber).

Two configurations, the headline one (BASELINE configs[1]: 32767-sample segments, L = 1024, 1 channel) and the 13-channel one (configs[3],
L = 256).  Input: 64 segments' worth of 2-channel int16 PCM at 44.1 kHz, pushed in 100 ms chunks (4410 frames), generator seed 20261018.
Measured in one process per configuration:
  ingest      device time of every IngestStream.push (mix + resample launches) by events around the call, their median and their sum over
              the file, beside ONE ymt3_ingest of the whole file on the same build;
  detok       the same for every ymt3_detokenize_push, one segment per push (the ids: encode_segment rows of random events, as
              scripts/gpu_detok_bench.py builds them), beside ONE ymt3_detokenize of all 64 segments;
  session     a whole LiveTranscriber run: the wall time of every push that completed a segment, from the arrival of the segment's last
              chunk to its notes on the host (ingest, one decode of L steps, detokeniser push, copy back), and of the other pushes.
Run without arguments this file is the launcher: every configuration is a fresh process under its own `timeout`; a step that fails ends
the run.  Output: profiles/live_bench.json (OUT=... for another path)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SEED = 20261018
N_SEG, SR, CHUNK = 64, 44100, 4410
CONFIGS = {"one_channel": dict(baseline=1, task="mt3_full_plus", events=150), "mc13": dict(baseline=3, task="mc13_full_plus_256", events=40)}


def child(name):
    import numpy as np
    import torch
    import gpu_detok_bench as DB
    from yourmt3_amd.config import baseline_config
    from yourmt3_amd.model import YourMT3
    from yourmt3_amd.task_manager import TaskManager
    from yourmt3_amd.transcribe import LiveTranscriber
    c = CONFIGS[name]
    cfg = baseline_config(c["baseline"])
    tm = TaskManager(c["task"])
    L = min(tm.max_note_token_length, cfg.max_decode_len)
    m = YourMT3(cfg, max_batch=1)
    S = cfg.segment_samples
    n_frames = (N_SEG * S * SR) // cfg.sample_rate - 500           # a little short of 64 whole segments: the last one is padded
    rng = np.random.default_rng(SEED)
    t = np.arange(n_frames)[:, None] / SR
    x = 0.4 * np.sin(2 * np.pi * 440.0 * (1 + np.arange(2)[None, :]) * t) + 0.1 * rng.standard_normal((n_frames, 2))
    pcm = torch.from_numpy((np.clip(x, -1, 1) * 32767).astype(np.int16)).cuda()
    chunks = [(a, min(a + CHUNK, n_frames)) for a in range(0, n_frames, CHUNK)]

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        return out, (e0, e1)

    def ms(pairs):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in pairs]

    # ---- ingest
    ing = m.compile_ingest_stream(SR, 2, torch.int16, max_chunk_frames=CHUNK)
    one_shot_ms, stream_ms = [], []
    for rep in range(4):                                                             # (the first pass warms up)
        ing.reset()
        rows, pairs = [], []
        for a, b in chunks:
            got, ev = events(lambda: ing.push(pcm[a:b]))
            rows.append(got)
            pairs.append(ev)
        last, ev = events(lambda: ing.finish()[0])
        pairs.append(ev)
        ref, ev1 = events(lambda: m.ingest(pcm, SR))
        if rep:
            stream_ms.append(ms(pairs))
            one_shot_ms.append(ms([ev1])[0])
    same_ingest = bool(torch.equal(torch.cat(rows + [last]), ref))
    ing.close()
    per_push = np.median(np.array(stream_ms), axis=0)
    res = {"input": f"{n_frames} frames of 2-channel int16 at {SR} Hz = {ref.shape[0]} segments of {S} samples, {len(chunks)} pushes of {CHUNK} frames, seed {SEED}",
           "ingest": {"push_device_ms_median": round(float(np.median(per_push[:-1])), 4), "push_device_ms_max": round(float(per_push[:-1].max()), 4),
                      "finish_device_ms": round(float(per_push[-1]), 4), "sum_over_file_ms": round(float(per_push.sum()), 3),
                      "one_shot_ingest_ms": round(float(np.median(one_shot_ms)), 4), "launches": 2 * len(chunks) + 1, "bits_equal_one_shot": same_ingest}}

    # ---- detokeniser
    w = dict(n=N_SEG, L=L, channels=cfg.n_channels, events=c["events"])
    tokens_np, starts, end_sec, used = DB.build_tokens(tm, w)
    tokens = torch.from_numpy(tokens_np).cuda()
    starts_dev = torch.tensor(starts, dtype=torch.float64).cuda()
    d = m.compile_detokenizer(tm, N_SEG, L)
    st = d.new_state()
    push_ms, shot_ms = [], []
    for rep in range(4):
        st.reset()
        pairs, n_notes = [], 0
        for s in range(N_SEG):
            hz = starts[s + 1] if s + 1 < N_SEG else float("inf")
            (_, cnt), ev = events(lambda: d.push_device(st, tokens[s:s + 1], None, starts_dev[s:s + 1], hz))
            n_notes += int(cnt[0])                                                   # (a copy back per push, as a session does)
            pairs.append(ev)
        (_, cnt), ev = events(lambda: d.finish_device(st, end_sec))
        n_notes += int(cnt[0])
        pairs.append(ev)
        (_, cnt1), ev1 = events(lambda: d.run_device(tokens, None, starts_dev, end_sec))
        if rep:
            push_ms.append(ms(pairs))
            shot_ms.append(ms([ev1])[0])
    per = np.median(np.array(push_ms), axis=0)
    res["detok"] = {"tokens_before_padding": int(used), "push_device_ms_median": round(float(np.median(per[:-1])), 4),
                    "push_device_ms_max": round(float(per[:-1].max()), 4), "finish_device_ms": round(float(per[-1]), 4),
                    "sum_over_file_ms": round(float(per.sum()), 3), "one_shot_detokenize_ms": round(float(np.median(shot_ms)), 4),
                    "launches": 2 * N_SEG + 1, "notes_streamed": n_notes, "notes_one_shot": int(cnt1[0]), "state_carry_records": st.carry}
    st.close()
    d.close()

    # ---- the session
    host = pcm.cpu()
    walls = {"completing": [], "other": []}
    with LiveTranscriber(m, SR, 2, torch.int16, task_manager=tm, max_chunk_frames=CHUNK, bsz=1) as live:
        for a, b in chunks:
            before = live.n_segments
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            live.push(host[a:b])
            torch.cuda.synchronize()
            walls["completing" if live.n_segments > before else "other"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        live.finish()
        t_finish = time.perf_counter() - t0
        n_live = len(live.notes)
    comp = np.array(walls["completing"][1:])                                         # (the first decode builds its graphs)
    res["session"] = {"decode_steps_per_segment": L, "pushes_completing_a_segment": len(walls["completing"]),
                      "last_chunk_to_notes_ms_median": round(float(np.median(comp)) * 1e3, 3), "last_chunk_to_notes_ms_max": round(float(comp.max()) * 1e3, 3),
                      "other_push_ms_median": round(float(np.median(walls["other"])) * 1e3, 4), "finish_ms": round(t_finish * 1e3, 3), "notes": n_live}
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if same_ingest else 3


def launcher():
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "live_bench.json"))
    results = {}
    me = os.path.abspath(__file__)
    for name in CONFIGS:
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, me, "--config", name], capture_output=True, text=True, cwd=ROOT)
        line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(r.stdout[-4000:], r.stderr[-4000:], sep="\n")
            print(f"{name}: exit status {r.returncode}; nothing further is started")
            return r.returncode or 1
        results[name] = json.loads(line[len("RESULT "):])
        print(name, json.dumps(results[name]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(results, open(out_path, "w"), indent=1)
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    sys.exit(child(sys.argv[sys.argv.index("--config") + 1]) if "--config" in sys.argv else launcher())
