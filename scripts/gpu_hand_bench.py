"""Host hand splitting (split_hands of yourmt3_amd/hands.py, the specification) against the device call (HandSplitter.split;
include/ymt3.h, hands) on the same records, at the default parameters (100 frames per second, slices of 4 frames).

The workloads are synthetic piano pieces (piano_piece below; seed 20261021): a left hand of broken chords and octaves, a right hand of a
melody with thirds and some chords, both wandering, a few crossings and rests, 10 ms of jitter:
  3_minutes    18 000 frames
  10_minutes   60 000 frames
Timed in one process per workload after a warm-up:
  host     split_hands(records, n_frames): a host clock, median of HOST_REPS
  device   HandSplitter.split: device events around CALLS back-to-back calls, divided by CALLS; medians of REPS
PARAMS (a JSON object) times another parameter set beside the defaults, e.g. PARAMS='{"slice_frames": 1}'.
The only comparison is host specification against device path: the parent commit has no such call.  No ratio is promised.

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout`; a step that fails ends the run.
BENCH_THIS / BENCH_PARENT: files holding bench.py's JSON lines of this commit and of its parent (runs taken in turn on one machine); their
time per step and headline value are recorded beside the timings as "bench".
Output: profiles/hand_bench.json (OUT=... for another path)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261021
REPS = 5
CALLS = 10
HOST_REPS = 3
FPS = 100.0
WORKLOADS = {"3_minutes": (180.0, 300), "10_minutes": (600.0, 600)}          # name -> (seconds, timeout)


def piano_piece(seconds, seed=SEED):
    """-> a NOTE_RECORD array, shuffled: two hands at about 100 bpm"""
    import numpy as np
    from yourmt3_amd.task_manager import NOTE_RECORD
    rng = np.random.default_rng(seed)
    rows, t, k = [], 0.5, 0
    low, high = 43.0, 72.0
    while t < seconds - 1.0:
        period = 60.0 / (96.0 + 12.0 * np.sin(2.0 * np.pi * t / 83.0)) / 2.0         # eighths
        low = min(60.0, max(28.0, low + rng.normal(0, 0.6)))
        high = min(100.0, max(low + 7.0, high + rng.normal(0, 0.8)))
        jit = lambda: float(rng.normal(0, 0.01))
        if rng.random() > 0.04:                                                   # the left hand: a broken chord, an octave on the bar
            base = int(round(low))
            rows.append((t + jit(), t + period * 0.9, base + (0, 7, 4, 7)[k % 4]))
            if k % 8 == 0:
                rows.append((t + jit(), t + period * 3.5, base - 12))
        if k % 2 == 0 and rng.random() > 0.08:                                   # the right hand: a melody, a third below it at times, a chord now and then
            top = int(round(high)) + int(rng.integers(-2, 3))
            rows.append((t + jit(), t + period * 1.8, top))
            if rng.random() < 0.3:
                rows.append((t + jit(), t + period * 1.8, top - (3 + int(rng.integers(0, 2)))))
            if rng.random() < 0.08:
                rows.append((t + jit(), t + period * 1.8, top - 7))
        if rng.random() < 0.01:
            t += 3.0                                                             # a rest
        t += period
        k += 1
    rec = np.zeros(len(rows), NOTE_RECORD)
    for i, (on, off, pitch) in enumerate(rows):
        rec[i] = (max(on, 0.0), off, 0, min(127, max(0, pitch)), 0, np.nan)
    return rec[rng.permutation(len(rows))]


def child(name):
    import numpy as np
    import torch
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.hands import split_hands
    from yourmt3_amd.model import YourMT3
    seconds = WORKLOADS[name][0]
    rec, n_frames = piano_piece(seconds), int(seconds * FPS)
    params = json.loads(os.environ.get("PARAMS", "{}"))
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_enc_layers=1, n_dec_layers=1)    # only the handle matters here
    m = YourMT3(cfg, max_batch=1)
    hs = m.compile_hand_splitter(n_frames, int(rec.size))
    other = m.compile_hand_splitter(n_frames, int(rec.size), **params) if params else None
    rd = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    calls = {"hands": lambda: hs.split(rd, n_frames)}
    if other is not None:
        calls["hands_params"] = lambda: other.split(rd, n_frames)
    reps = int(os.environ.get("REPS", REPS))
    times = {}
    for label, split in calls.items():
        split()                                                   # warm-up: code objects, the allocator's blocks
        torch.cuda.synchronize()
        times[label] = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                split()
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) / 1e3 / CALLS)
        print(f"{name}: device {label} {sorted(times[label])} s per call", flush=True)
    host, host_params = [], []
    for _ in range(int(os.environ.get("HOST_REPS", HOST_REPS))):
        t0 = time.perf_counter()
        want = split_hands(rec, n_frames)
        host.append(time.perf_counter() - t0)
        print(f"{name}: host {host[-1]:.3f} s", flush=True)
    equal = True
    for label, kw in (("hands", {}), ("hands_params", params)):
        if label not in calls:
            continue
        t0 = time.perf_counter()
        ref = split_hands(rec, n_frames, **kw)
        if kw:
            host_params.append(time.perf_counter() - t0)
        hand_dev, split_dev, result_dev = calls[label]()
        T = int(ref[2][0])
        got = hand_dev.cpu().numpy(), split_dev[:T].cpu().numpy(), result_dev.cpu().numpy()
        equal = equal and all(g.tolist() == w.tolist() for g, w in zip(got, ref))
    med = lambda v: float(np.median(v))
    T = int(want[2][0])
    res = {"workload": f"{rec.size} notes, {n_frames} frames at {FPS:g} per second, default parameters, seed {SEED}; device: events around {CALLS} calls, "
                       f"median of {reps}; host: median of {len(host)}",
           "n_notes": int(rec.size), "n_frames": n_frames, "n_slices": T, "left": int(want[2][2]), "right": int(want[2][3]), "total": int(want[2][4]),
           "hand_overs": int(want[2][6]), "device_equals_host": equal, "host_s": round(med(host), 4), "device_split_s": round(med(times["hands"]), 7),
           "device_us_per_slice": round(med(times["hands"]) * 1e6 / max(T, 1), 4), "host_s_all": [round(x, 4) for x in host],
           "device_split_s_all": [round(x, 7) for x in times["hands"]]}
    if other is not None:
        res.update(params=params, host_params_s=round(med(host_params), 4), device_split_params_s=round(med(times["hands_params"]), 7),
                   device_split_params_s_all=[round(x, 7) for x in times["hands_params"]])
    for o in (other, hs, m):
        if o is not None:
            o.close()
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
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "hand_bench.json"))
    if "--workload" in sys.argv:
        sys.exit(child(sys.argv[sys.argv.index("--workload") + 1]))
    sys.exit(launcher(out))
