"""Host frame metrics and piano roll (yourmt3_amd/metrics.py, the specification) against the device calls (include/ymt3.h, piano roll and
frame metrics) on the same inputs.

Two workloads, 131 rows (130 programs) at 100 frames per second:
  transcription  the notes of the 64-segment, 13-channel synthetic transcription of scripts/gpu_detok_bench.py (its generator and seed,
                 detokenised on the host) as the ESTIMATE, and the perturbed copy of scripts/gpu_metrics_bench.py as the REFERENCE;
                 n_frames = ceil(end_sec * 100)
  random         2^17 random notes per side over 60 000 frames (seed 20261018): uniform onsets, durations of 1 .. 200 frames, uniform
                 programs and pitches; the estimate is the reference with 60 % of the onsets and offsets moved, 10 % dropped and replaced
Timed in one process per workload, the records already on the device, after a warm-up, medians of 5:
  host     frame_metrics(ref, est, ...) and piano_roll(est, ...): a host clock
  device   PianoRoll.metrics, PianoRoll.roll (all rows) and PianoRoll.roll(rows="agnostic"): device events around CALLS back-to-back calls,
           divided by CALLS
The only comparison is host specification against device path: the parent commit has no such call.  No ratio is promised.

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout`; a step that fails ends the run.
`--workload NAME --profile` runs every device call once after a warm-up and nothing else: the process to put under a kernel trace.
Output: profiles/roll_bench.json (OUT=... for another path)."""
import json, math, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SEED = 20261018
REPS = 5
CALLS = 10
N_PROGRAMS = 130
FPS = 100.0
WORKLOADS = ("transcription", "random")


def transcription_notes():
    import numpy as np
    import gpu_detok_bench as DB
    import gpu_metrics_bench as MB
    from yourmt3_amd.metrics import to_records
    from yourmt3_amd.task_manager import TaskManager
    w = DB.WORKLOADS["mc13"]
    tm = TaskManager(w["task"])
    tokens_np, starts, end_sec, _ = DB.build_tokens(tm, w)
    est = to_records(tm.tokens_to_notes([tokens_np], starts, end_sec))
    ref = MB.perturbed(np.random.default_rng(SEED), est)
    return ref, est, max(1, math.ceil(end_sec * FPS)), f"{w['n']} segments x {w['channels']} channels x {w['L']} columns ({w['task']}), detok seed {DB.SEED}"


def random_notes(n=1 << 17, n_frames=60000):
    import numpy as np
    from yourmt3_amd.task_manager import NOTE_RECORD
    rng = np.random.default_rng(SEED)

    def some(k):
        rec = np.zeros(k, NOTE_RECORD)
        rec["onset"] = rng.integers(0, n_frames, k) / 100
        rec["offset"] = rec["onset"] + rng.integers(1, 201, k) / 100
        rec["program"] = rng.integers(0, N_PROGRAMS, k)
        rec["pitch"] = rng.integers(0, 128, k)
        rec["is_drum"] = rec["program"] == 128
        return rec
    ref = some(n)
    est = ref.copy()
    move = rng.random(n) < 0.6
    est["onset"] += np.where(move, rng.integers(-7, 8, n), 0) / 100
    est["offset"] += np.where(move, rng.integers(-30, 31, n), 0) / 100
    new = rng.random(n) < 0.1
    est[new] = some(int(new.sum()))
    return ref, est[rng.permutation(n)], n_frames, f"{n} random notes per side over {n_frames} frames"


def child(name, profile):
    import numpy as np
    import torch
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.metrics import frame_metrics, piano_roll
    from yourmt3_amd.model import YourMT3
    ref, est, n_frames, what = transcription_notes() if name == "transcription" else random_notes()
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_enc_layers=1, n_dec_layers=1)    # only the handle matters here
    m = YourMT3(cfg, max_batch=1)
    pr = m.compile_piano_roll(N_PROGRAMS, n_frames, FPS)
    rd, ed = (torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda() for r in (ref, est))
    calls = {"metrics": lambda: pr.metrics(rd, ed, n_frames), "roll_all_rows": lambda: pr.roll(ed, n_frames),
             "roll_agnostic": lambda: pr.roll(ed, n_frames, rows="agnostic")}
    for fn in calls.values():                                     # warm-up: code objects, the allocator's blocks
        fn()
    torch.cuda.synchronize()
    if profile:
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        pr.close()
        m.close()
        return 0
    reps = int(os.environ.get("REPS", REPS))
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / 1e3 / CALLS)
            del out
    host = {"metrics": [], "roll_all_rows": []}
    for _ in range(reps):
        t0 = time.perf_counter()
        want = frame_metrics(ref, est, n_frames, N_PROGRAMS, frames_per_second=FPS)
        host["metrics"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        want_roll = piano_roll(est, n_frames, N_PROGRAMS, frames_per_second=FPS)
        host["roll_all_rows"].append(time.perf_counter() - t0)
    got = calls["metrics"]().cpu().numpy()
    got_last = calls["roll_agnostic"]().cpu().numpy()
    equal = bool(np.array_equal(got, want.flat())) and bool(np.array_equal(got_last[0], want_roll[-1]))
    med = lambda v: float(np.median(v))
    res = {"workload": f"{what}; {N_PROGRAMS + 1} rows, {n_frames} frames at {FPS:g} per second, reference seed {SEED}; medians of {reps}, "
                       f"device: events around {CALLS} calls",
           "n_ref": int(ref.size), "n_est": int(est.size), "n_frames": n_frames, "device_equals_host": equal,
           "frame_f": round(want.frame_f, 4), "multi_frame_f": round(want.multi_frame_f, 4), "sounding_cells_est_agnostic": int(want_roll[-1].sum()),
           "host_s": {k: round(med(v), 5) for k, v in host.items()},
           "device_s": {k: round(med(v), 7) for k, v in times.items()},
           "host_s_all": {k: [round(x, 4) for x in v] for k, v in host.items()},
           "device_s_all": {k: [round(x, 7) for x in v] for k, v in times.items()}}
    pr.close()
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if equal else 3


def launcher():
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "roll_bench.json"))
    results = {}
    me = os.path.abspath(__file__)
    for name in WORKLOADS:
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, me, "--workload", name], capture_output=True, text=True, cwd=ROOT)
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
        sys.exit(child(sys.argv[sys.argv.index("--workload") + 1], "--profile" in sys.argv))
    sys.exit(launcher())
