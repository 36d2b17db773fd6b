"""Host detokeniser against the device detokeniser (include/ymt3.h, device detokeniser) on ids that are already on the GPU.

Two workloads, generator seed 20261017:
  one_channel   256 one-channel segments of 1024 columns; every segment is encode_segment of 150 random events (10 % drum hits, the others
                onsets / offsets of 4 programs x 48 pitches at random 10 ms steps of the segment) and 2 tied notes;
  mc13          64 segments x 13 channels of 256 columns; every row is encode_segment of 40 random events of the channel's instrument group
                and 2 tied notes.
Timed in one process per workload, 5 interleaved repetitions after a warm-up, medians:
  host     tokens.cpu() + TaskManager.tokens_to_notes
  device   TaskManager.tokens_to_notes_device with a detokeniser compiled beforehand: kernels + copy of the counters and records + the Note
           list; its parts are timed as well (kernels by device events around the C call, the copy, Note construction and sort).

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout` (one model handle each), then --
unless NO_PROFILE=1 -- one more under `rocprofv3 --kernel-trace --stats` for the kernels' own times; a step that fails ends the run.
Output: profiles/detok_bench.json (OUT=... for another path); the profiler's files stay under results/."""
import json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261017
WORKLOADS = {"one_channel": dict(task="mt3_full_plus", n=256, L=1024, events=150, channels=1),
             "mc13": dict(task="mc13_full_plus_256", n=64, L=256, events=40, channels=13)}
REPS = 5


def build_tokens(tm, w):
    import numpy as np
    from yourmt3_amd.task_manager import DRUM_PROGRAM, MC13_GROUPS, NoteEvent
    rng = np.random.default_rng(SEED)
    n, L, K = w["n"], w["L"], w["channels"]
    starts = [i * 32767 / 16000 for i in range(n)]
    out = np.zeros((n, K, L), np.int32)
    used = 0
    for s in range(n):
        for ch in range(K):
            progs = [0, 24, 40, 129] if K == 1 else [p for p in MC13_GROUPS[ch][1]][:4]
            pitched = [p for p in progs if p != DRUM_PROGRAM]
            events = []
            for _ in range(w["events"]):
                t = starts[s] + int(rng.integers(0, 205)) / tm.codec.steps_per_second
                if not pitched or (DRUM_PROGRAM in progs or K == 1) and rng.random() < 0.1:
                    events.append(NoteEvent(t, True, DRUM_PROGRAM, 1, int(rng.integers(35, 60))))
                else:
                    events.append(NoteEvent(t, False, int(rng.choice(pitched)), int(rng.integers(0, 2)), int(rng.integers(36, 84))))
            ties = [(p, int(rng.integers(36, 84))) for p in (pitched[:1] * 2)]
            row = tm.tokenizer.encode_segment(events, ties, starts[s])[:L]
            out[s, ch, :len(row)] = row
            used += len(row)
    return out, starts, starts[-1] + 1.5, used


def child(name):
    import numpy as np
    import torch
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.model import YourMT3
    from yourmt3_amd.task_manager import TaskManager
    w = WORKLOADS[name]
    tm = TaskManager(w["task"])
    tokens_np, starts, end_sec, used = build_tokens(tm, w)
    cfg = YMT3Config(segment_samples=8191, max_decode_len=w["L"], n_channels=w["channels"])    # only vocab and n_channels matter here
    m = YourMT3(cfg, max_batch=1)
    d = m.compile_detokenizer(tm, w["n"], w["L"])
    tokens = torch.from_numpy(tokens_np).cuda()
    starts_dev = torch.tensor(starts, dtype=torch.float64).cuda()

    def host():
        return tm.tokens_to_notes([tokens.cpu().numpy()], starts, end_sec)

    def device():
        return tm.tokens_to_notes_device(m, tokens, starts, end_sec, detokenizer=d)[0]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    times = {"host": [], "device": [], "device_kernels_and_copy": [], "kernels_by_events": []}
    reps = int(os.environ.get("REPS", REPS))
    for rep in range(reps + 1):                                   # (the first pass warms up)
        th, ref = wall(host)
        td, got = wall(device)
        trun, _ = wall(lambda: d.run(tokens, None, starts_dev, end_sec))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d.run(tokens, None, starts_dev, end_sec)                  # (its copy back waits for the kernels; the events bracket the stream work)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            times["host"].append(th); times["device"].append(td); times["device_kernels_and_copy"].append(trun)
            times["kernels_by_events"].append(e0.elapsed_time(e1) / 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"workload": f"{w['n']} segments x {w['channels']} channels x {w['L']} columns ({w['task']}), seed {SEED}, {reps} interleaved repetitions (medians)",
           "tokens_before_padding": int(used), "notes": len(ref), "notes_equal_host": bool(got == ref),
           "host_s": round(med["host"], 5), "device_s": round(med["device"], 5), "host_over_device": round(med["host"] / med["device"], 2),
           "device_parts_s": {"kernels_and_copy_back": round(med["device_kernels_and_copy"], 5),
                              "stream_work_by_device_events": round(med["kernels_by_events"], 5),
                              "note_list_and_sort": round(med["device"] - med["device_kernels_and_copy"], 5)},
           "host_s_all": [round(x, 4) for x in times["host"]], "device_s_all": [round(x, 5) for x in times["device"]]}
    d.close()
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if res["notes_equal_host"] else 3


def kernel_stats(outdir):
    """kernel name -> {calls, total_us, mean_us} from rocprofv3's kernel stats CSV"""
    import csv, glob
    stats = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            hit = re.search(r"detok_\w+", row.get("Name", ""))
            if hit:
                stats[hit.group(0)] = {"calls": int(row["Calls"]), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1),
                                             "mean_us": round(float(row["AverageNs"]) / 1e3, 2)}
    return stats


def launcher():
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "detok_bench.json"))
    results = {}
    me = os.path.abspath(__file__)
    for name in WORKLOADS:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, me, "--workload", name], capture_output=True, text=True, cwd=ROOT)
        line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(r.stdout[-4000:], r.stderr[-4000:], sep="\n")
            print(f"{name}: exit status {r.returncode}; nothing further is started")
            return r.returncode or 1
        results[name] = json.loads(line[len("RESULT "):])
        print(name, json.dumps(results[name]))
    if os.environ.get("NO_PROFILE") != "1":
        for name in WORKLOADS:
            pdir = os.path.join(ROOT, "results", f"detok_prof_{name}")
            env = dict(os.environ, REPS="2")
            r = subprocess.run(["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "--", sys.executable, me,
                                "--workload", name], capture_output=True, text=True, cwd=ROOT, env=env)
            if r.returncode != 0:
                print(r.stdout[-3000:], r.stderr[-3000:], sep="\n")
                print(f"profile of {name}: exit status {r.returncode}; nothing further is started")
                results[name]["kernel_trace"] = f"failed with exit status {r.returncode}"
                break
            results[name]["kernel_trace_us"] = kernel_stats(pdir)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(results, open(out_path, "w"), indent=1)
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    sys.exit(child(sys.argv[sys.argv.index("--workload") + 1]) if "--workload" in sys.argv else launcher())
