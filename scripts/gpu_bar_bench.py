"""Host bar tracking (track_bars of yourmt3_amd/bars.py, the specification) against the device call (BarTracker.track; include/ymt3.h, bars
and key) on the same records and beats, at the default parameters (100 frames per second).

Two workloads of synthetic notes, those of scripts/gpu_beat_bench.py given a metre: a tempo that wanders between 90 and 130 bpm, 4/4 with
a stretch of 3/4 in the middle third, a chord on every beat whose root changes each bar, a long bass note and a kick on every downbeat, a
snare on odd beats, an off-beat eighth on most beats, 10 ms jitter, and two stray notes a second (seed 20261020):
  3_minutes    18 000 frames
  10_minutes   60 000 frames
The beats are the device beat tracker's, left on the device.  Timed in one process per workload after a warm-up:
  host     track_bars(records, beats, n_frames): a host clock, median of HOST_REPS
  device   BarTracker.track: device events around CALLS back-to-back calls, divided by CALLS; medians of REPS
The only comparison is host specification against device path: the parent commit has no such call.  No ratio is promised.

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout`; a step that fails ends the run.
BENCH_THIS / BENCH_PARENT: files holding bench.py's JSON lines of this commit and of its parent (runs taken in turn on one machine); their
time per step and headline value are recorded beside the timings as "bench".
Output: profiles/bar_bench.json (OUT=... for another path)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261020
REPS = 5
CALLS = 10
HOST_REPS = 3
FPS = 100.0
WORKLOADS = {"3_minutes": (180.0, 300), "10_minutes": (600.0, 600)}          # name -> (seconds, timeout)
ROOTS = (0, 5, 7, 9, 2, 4)


def notes_of(seconds, seed=SEED):
    """-> (NOTE_RECORD array, shuffled; the downbeats' times; the metre runs [(m, bars)])"""
    import numpy as np
    from yourmt3_amd.task_manager import NOTE_RECORD
    rng = np.random.default_rng(seed)
    rows, downs, runs, t, k, bar, m = [], [], [], 0.5, 0, 0, 4
    while t < seconds - 1.0:
        bpm = 110.0 + 20.0 * np.sin(2.0 * np.pi * t / 97.0)
        period = 60.0 / bpm
        if k == 0:
            m = 3 if seconds / 3.0 <= t < 2.0 * seconds / 3.0 else 4
            root = ROOTS[bar % len(ROOTS)]
            downs.append(t)
            if runs and runs[-1][0] == m:
                runs[-1][1] += 1
            else:
                runs.append([m, 1])
            rows.append((t + rng.normal(0, 0.01), 0.95 * m * period, 0, 36 + root, False))
            rows.append((t + rng.normal(0, 0.01), 0.0, 128, 36, True))
        for step in (0, 4, 7):
            rows.append((t + rng.normal(0, 0.01), 0.8 * period, 0, 60 + (root + step) % 12, False))
        if k % 2 == 1:
            rows.append((t + rng.normal(0, 0.01), 0.0, 128, 38, True))
        if rng.random() < 0.7:
            rows.append((t + period / 2 + rng.normal(0, 0.01), 0.2, 0, 72 + (root + 7) % 12, False))
        t, k = t + period, k + 1
        if k == m:
            k, bar = 0, bar + 1
    for _ in range(int(2 * seconds)):
        rows.append((float(rng.uniform(0, seconds - 1.0)), 0.3, int(rng.integers(0, 8)), int(rng.integers(36, 96)), False))
    rec = np.zeros(len(rows), NOTE_RECORD)
    for i, j in enumerate(rng.permutation(len(rows))):
        on, length, prog, pitch, drum = rows[j]
        rec[i] = (on, on + length, prog, pitch, drum, np.nan)
    return rec, downs, [tuple(r) for r in runs]


def f_measure(est, ref, tol=0.07):
    i = j = hits = 0
    while i < len(est) and j < len(ref):
        if abs(est[i] - ref[j]) <= tol:
            hits, i, j = hits + 1, i + 1, j + 1
        elif est[i] < ref[j]:
            i += 1
        else:
            j += 1
    return 2.0 * hits / (len(est) + len(ref)) if est and ref else 0.0


def child(name):
    import numpy as np
    import torch
    from yourmt3_amd.bars import key_name, metre_runs, track_bars
    from yourmt3_amd.beats import max_beats
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.model import YourMT3
    seconds = WORKLOADS[name][0]
    (rec, downs, runs), n_frames = notes_of(seconds), int(seconds * FPS)
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_enc_layers=1, n_dec_layers=1)    # only the handle matters here
    m = YourMT3(cfg, max_batch=1)
    bt = m.compile_beat_tracker(n_frames)
    br = m.compile_bar_tracker(max_beats(n_frames, bt.lag_min), int(rec.size))
    rd = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    beats_dev, _, beat_result = bt.track(rd, n_frames)
    track = lambda: br.track(beats_dev, beat_result, rd, n_frames)
    track()                                                       # warm-up: code objects, the allocator's blocks
    torch.cuda.synchronize()
    reps = int(os.environ.get("REPS", REPS))
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            track()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / CALLS)
    print(f"{name}: device track {sorted(times)} s per call", flush=True)
    k = int(beat_result.cpu()[0])
    beats = beats_dev[:k].cpu().numpy()
    host = []
    for _ in range(int(os.environ.get("HOST_REPS", HOST_REPS))):
        t0 = time.perf_counter()
        want = track_bars(rec, beats, n_frames)
        host.append(time.perf_counter() - t0)
        print(f"{name}: host {host[-1]:.3f} s", flush=True)
    metre_dev, result_dev = track()
    metre, result = metre_dev[:k].cpu().numpy(), result_dev.cpu().numpy()
    equal = metre.tolist() == want[0].tolist() and result.tolist() == want[1].tolist()
    est = [int(b) / FPS for b, v in zip(beats, want[0].tolist()) if v & 255 == 0]
    med = lambda v: float(np.median(v))
    res = {"workload": f"{rec.size} notes, {n_frames} frames at {FPS:g} per second, default parameters, seed {SEED}; device: events around {CALLS} calls, "
                       f"median of {reps}; host: median of {len(host)}",
           "n_notes": int(rec.size), "n_frames": n_frames, "n_beats": k, "n_downbeats": int(want[1][0]), "metre_runs": [list(r) for r in metre_runs(want[0])],
           "generated_runs": [list(r) for r in runs], "downbeat_f_measure": round(f_measure(est, downs), 4), "key": key_name(int(want[1][3])),
           "device_equals_host": equal, "host_s": round(med(host), 4), "device_track_s": round(med(times), 7),
           "host_s_all": [round(x, 4) for x in host], "device_track_s_all": [round(x, 7) for x in times]}
    br.close()
    bt.close()
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if equal else 3


def launcher(out_path):
    results = {}
    me = os.path.abspath(__file__)
    for name in os.environ.get("WORKLOADS", ",".join(WORKLOADS)).split(","):
        r = subprocess.run(["timeout", "-k", "10", str(WORKLOADS[name][1]), sys.executable, me, "--workload", name], capture_output=True, text=True, cwd=ROOT)
        print(r.stdout, r.stderr[-2000:], sep="\n", flush=True)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{name}: exit status {r.returncode}; nothing further is started")
            return r.returncode or 1
        results[name] = json.loads(line[-1][len("RESULT "):])
    bench = {}
    for label, var in (("this_commit", "BENCH_THIS"), ("parent", "BENCH_PARENT")):
        path = os.environ.get(var)
        if path and os.path.exists(path):
            lines = [json.loads(x) for x in open(path).read().splitlines() if x.startswith("{")]
            if lines:
                bench[label] = {"arguments": f"--gpus {lines[0]['n_gpus']} --steps {lines[0]['steps']} --warmup {lines[0]['warmup']}",
                                "ms_per_step": [round(x["ms_per_step"], 2) for x in lines], "audio_s_per_wall_s": [round(x["value"], 1) for x in lines]}
    if bench:
        results["bench"] = bench
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(results, open(out_path, "w"), indent=1)
    print("wrote", out_path, flush=True)
    return 0


if __name__ == "__main__":
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "bar_bench.json"))
    if "--workload" in sys.argv:
        sys.exit(child(sys.argv[sys.argv.index("--workload") + 1]))
    sys.exit(launcher(out))
