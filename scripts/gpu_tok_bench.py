"""Host tokeniser against the device tokeniser (include/ymt3.h, device tokeniser), and score_notes end to end next to the scoring pass alone.

Two workloads, the detokeniser benchmark's (scripts/gpu_detok_bench.py, generator seed 20261017):
  one_channel   256 one-channel segments of 1024 columns;
  mc13          64 segments x 13 channels of 256 columns.
The notes are what the host detokeniser makes of those seeded grammar-valid ids.  Timed in one process per workload, 5 interleaved
repetitions after a warm-up, medians, a host clock around a device synchronise:
  host     TaskManager.notes_to_tokens
  device   TaskManager.notes_to_tokens_device from the Note list with a tokeniser compiled beforehand; its parts are timed as well:
           building and uploading the records, the C call's kernels (records already on the device), the copy back of the lengths.
The `score` workload: the first 64 segments of one_channel on the default one-channel model -- score_notes (ingest, tokenise, encode,
scoring pass, copy back) next to YourMT3.decode_score alone on the same ids.

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout`; a step that fails ends the
run.  Output: profiles/tok_bench.json (OUT=... for another path)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

REPS = 5


def workload_notes(name):
    from gpu_detok_bench import WORKLOADS, build_tokens
    from yourmt3_amd.task_manager import TaskManager
    w = WORKLOADS[name]
    tm = TaskManager(w["task"])
    tokens, starts, end_sec, used = build_tokens(tm, w)
    return tm, w, tm.tokens_to_notes([tokens], starts, end_sec), starts, end_sec


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def child(name):
    import numpy as np
    import torch
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.model import NOTE_RECORD, YourMT3
    tm, w, notes, starts, end_sec = workload_notes(name)
    n, L = w["n"], w["L"]
    cfg = YMT3Config(segment_samples=8191, max_decode_len=L, n_channels=w["channels"], n_enc_layers=1, n_dec_layers=1)   # only vocab and n_channels matter here
    m = YourMT3(cfg, max_batch=1)
    t = m.compile_tokenizer(tm, n, L)
    starts_dev = torch.tensor(starts, dtype=torch.float64).cuda()

    def records():
        rec = np.zeros(len(notes), NOTE_RECORD)
        rec["onset"] = [x.onset for x in notes]; rec["offset"] = [x.offset for x in notes]; rec["program"] = [x.program for x in notes]
        rec["pitch"] = [x.pitch for x in notes]; rec["is_drum"] = [x.is_drum for x in notes]
        return torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()

    rec_dev = records()
    times = {"host": [], "device": [], "records_and_upload": [], "kernels": [], "lengths_copy_back": []}
    reps = int(os.environ.get("REPS", REPS))
    equal = True
    for rep in range(reps + 1):                                   # (the first pass warms up)
        th, ref = wall(lambda: tm.notes_to_tokens(notes, starts, end_sec, max_len=L))
        td, got = wall(lambda: tm.notes_to_tokens_device(m, notes, starts, end_sec, max_len=L, tokenizer=t))
        tu, _ = wall(records)
        tk, out = wall(lambda: t.run(rec_dev, starts_dev, end_sec, L))
        tc, _ = wall(lambda: out[1].cpu())
        equal = equal and bool(np.array_equal(got[0].cpu().numpy(), ref[0])) and bool(np.array_equal(out[0].cpu().numpy(), ref[0]))
        if rep:
            for k, v in zip(times, (th, td, tu, tk, tc)):
                times[k].append(v)
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"workload": f"{n} segments x {w['channels']} channels x {L} columns ({w['task']}), {reps} interleaved repetitions (medians)",
           "notes": len(notes), "tokens_before_padding": int(ref[1].sum()), "ids_equal_host": equal,
           "host_s": round(med["host"], 5), "device_s": round(med["device"], 5), "host_over_device": round(med["host"] / med["device"], 2),
           "device_parts_s": {k: round(med[k], 6) for k in ("records_and_upload", "kernels", "lengths_copy_back")},
           "host_s_all": [round(x, 4) for x in times["host"]], "device_s_all": [round(x, 5) for x in times["device"]]}
    t.close()
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if equal else 3


def child_score():
    import numpy as np
    import torch
    from oracle import ymt3_oracle as O
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.model import YourMT3
    from yourmt3_amd.transcribe import score_notes
    tm, w, notes, starts, end_sec = workload_notes("one_channel")
    n = 64
    cfg = YMT3Config(max_decode_len=1024)
    end_sec = n * cfg.segment_samples / cfg.sample_rate
    notes = [x for x in notes if x.onset < end_sec]
    m = YourMT3(cfg, max_batch=n)
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=n * cfg.segment_samples))[0].numpy()
    res0 = score_notes(m, audio, notes, task_manager=tm, bsz=n)
    tokens = res0["tokens"]
    segments = m.ingest(torch.from_numpy(audio), cfg.sample_rate)
    enc = m.encode(m.logmel(segments))
    times = {"score_notes": [], "decode_score": [], "host_tokenize": []}
    reps = int(os.environ.get("REPS", REPS))
    for rep in range(reps + 1):
        ta, _ = wall(lambda: score_notes(m, audio, notes, task_manager=tm, bsz=n))
        tb, _ = wall(lambda: m.decode_score(enc, tokens, lengths="eos"))
        tc, _ = wall(lambda: tm.notes_to_tokens(notes, starts[:n], end_sec))
        if rep:
            times["score_notes"].append(ta); times["decode_score"].append(tb); times["host_tokenize"].append(tc)
    med = {k: round(float(np.median(v)), 5) for k, v in times.items()}
    res = {"workload": f"{n} segments x 1 channel x 1024 columns, default model, {len(notes)} notes, {res0['n_tokens']} tokens, {reps} interleaved repetitions (medians)",
           "score_notes_s": med["score_notes"], "decode_score_alone_s": med["decode_score"], "host_notes_to_tokens_s": med["host_tokenize"],
           "log_likelihood": res0["log_likelihood"]}
    m.close()
    print("RESULT " + json.dumps(res))
    return 0


def launcher():
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "tok_bench.json"))
    results = {}
    me = os.path.abspath(__file__)
    for name in ("one_channel", "mc13", "score"):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, me, "--workload", name], capture_output=True, text=True, cwd=ROOT)
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
    if "--workload" in sys.argv:
        name = sys.argv[sys.argv.index("--workload") + 1]
        sys.exit(child_score() if name == "score" else child(name))
    sys.exit(launcher())
