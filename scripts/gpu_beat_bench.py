"""Host beat tracking (track_beats of yourmt3_amd/beats.py, the specification) against the device calls (BeatTracker.track and
.positions; include/ymt3.h, beat tracking) on the same records, at the default parameters (100 frames per second).

Two workloads of synthetic notes: a tempo that wanders between 90 and 130 bpm, a chord on every beat, an off-beat eighth on most, a drum
on every second beat, 10 ms jitter, and two stray notes a second (seed 20261019):
  3_minutes    18 000 frames
  10_minutes   60 000 frames
Timed in one process per workload, the records already on the device, after a warm-up:
  host     track_beats(records, n_frames): a host clock, median of HOST_REPS
  device   track, and track + positions: device events around CALLS back-to-back calls, divided by CALLS; medians of REPS
The only comparison is host specification against device path: the parent commit has no such call.  No ratio is promised.

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout`; a step that fails ends the run.
`--workload NAME --profile` runs the device calls once after a warm-up and nothing else: the process to put under a kernel trace.
`--trace` (the launcher's last step, or alone) puts that process for the 10-minute workload under `rocprofv3 --kernel-trace --stats`, a run
of its own under its own `timeout`, and adds the dispatches of the LAST call to the output as "kernels_10_minutes": per kernel the
launches, the summed duration in ns and the workgroups, then the time from the first kernel's start to the last one's end.
Output: profiles/beat_bench.json (OUT=... for another path)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261019
REPS = 5
CALLS = 10
HOST_REPS = 3
FPS = 100.0
WORKLOADS = {"3_minutes": (180.0, 300), "10_minutes": (600.0, 600)}          # name -> (seconds, timeout)


def notes_of(seconds, seed=SEED):
    """-> NOTE_RECORD array, shuffled"""
    import numpy as np
    from yourmt3_amd.task_manager import NOTE_RECORD
    rng = np.random.default_rng(seed)
    rows, t, k = [], 0.5, 0
    while t < seconds - 1.0:
        bpm = 110.0 + 20.0 * np.sin(2.0 * np.pi * t / 97.0)
        for pitch in (48, 60, 64, 67):
            rows.append((t + rng.normal(0, 0.01), 0.4, 0, pitch, False))
        if rng.random() < 0.7:
            rows.append((t + 30.0 / bpm + rng.normal(0, 0.01), 0.2, 0, 72, False))
        if k % 2 == 0:
            rows.append((t + rng.normal(0, 0.01), 0.0, 128, 36, True))
        t, k = t + 60.0 / bpm, k + 1
    for _ in range(int(2 * seconds)):
        rows.append((float(rng.uniform(0, seconds - 1.0)), 0.3, int(rng.integers(0, 8)), int(rng.integers(36, 96)), False))
    rec = np.zeros(len(rows), NOTE_RECORD)
    for i, j in enumerate(rng.permutation(len(rows))):
        on, length, prog, pitch, drum = rows[j]
        rec[i] = (on, on + length, prog, pitch, drum, np.nan)
    return rec


def child(name, profile):
    import numpy as np
    import torch
    from yourmt3_amd.beats import beat_positions, track_beats
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.model import YourMT3
    seconds = WORKLOADS[name][0]
    rec, n_frames = notes_of(seconds), int(seconds * FPS)
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_enc_layers=1, n_dec_layers=1)    # only the handle matters here
    m = YourMT3(cfg, max_batch=1)
    bt = m.compile_beat_tracker(n_frames)
    rd = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    track = lambda: bt.track(rd, n_frames)

    def both():
        b, _, r = bt.track(rd, n_frames)
        return bt.positions(b, r, rd)

    both()                                                        # warm-up: code objects, the allocator's blocks
    torch.cuda.synchronize()
    if profile:
        both()
        torch.cuda.synchronize()
        bt.close()
        m.close()
        return 0
    reps = int(os.environ.get("REPS", REPS))
    times = {"track": [], "track_and_positions": []}
    for label, call in (("track", track), ("track_and_positions", both)):
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                call()
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) / 1e3 / CALLS)
        print(f"{name}: device {label} {sorted(times[label])} s per call", flush=True)
    host = []
    for _ in range(int(os.environ.get("HOST_REPS", HOST_REPS))):
        t0 = time.perf_counter()
        want = track_beats(rec, n_frames)
        host.append(time.perf_counter() - t0)
        print(f"{name}: host {host[-1]:.3f} s", flush=True)
    beats, tempo, result, ticks = bt.run(rd, n_frames)
    equal = (beats.tolist() == want[0].tolist() and tempo.tolist() == want[1].tolist() and result.tolist() == want[2].tolist()
             and ticks.tolist() == beat_positions(rec, want[0]).tolist())
    med = lambda v: float(np.median(v))
    res = {"workload": f"{rec.size} notes, {n_frames} frames at {FPS:g} per second, default parameters, seed {SEED}; device: events around {CALLS} calls, "
                       f"median of {reps}; host: median of {len(host)}",
           "n_notes": int(rec.size), "n_frames": n_frames, "n_beats": int(want[2][0]), "windows": int(want[1].size),
           "tempo_lags": [int(want[1].min()), int(want[1].max())], "dp_blocks": -(-n_frames // 13), "device_equals_host": equal,
           "host_s": round(med(host), 4), "device_track_s": round(med(times["track"]), 7),
           "device_track_and_positions_s": round(med(times["track_and_positions"]), 7), "host_s_all": [round(x, 4) for x in host],
           "device_track_s_all": [round(x, 7) for x in times["track"]]}
    bt.close()
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if equal else 3


def trace(out_path):
    import glob, sqlite3, tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "beats", "--", sys.executable, os.path.abspath(__file__),
               "--workload", "10_minutes", "--profile"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        found = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not found:
            print(r.stdout[-3000:], r.stderr[-3000:], sep="\n")
            print(f"trace: exit status {r.returncode}, {len(found)} database(s)")
            return r.returncode or 1
        db = sqlite3.connect(found[0])
        t0 = db.execute("select max(start) from kernels where name like '%beat_clear_kernel%'").fetchone()[0]      # the call after the warm-up
        rows = db.execute("select name, count(*), sum(end - start), max(grid_x / workgroup_x) from kernels where start >= ? and name like '%beat_%' "
                          "group by name order by min(start)", (t0,)).fetchall()
        span = db.execute("select max(end) - min(start) from kernels where start >= ? and name like '%beat_%'", (t0,)).fetchone()[0]
    results = json.load(open(out_path)) if os.path.exists(out_path) else {}
    results["kernels_10_minutes"] = [{"name": r[0].replace("(anonymous namespace)::", "").split("(")[0], "calls": r[1], "total_ns": r[2], "workgroups": r[3]} for r in rows]
    results["kernels_10_minutes"].append({"name": "first start to last end of the call", "calls": 1, "total_ns": span, "workgroups": None})
    json.dump(results, open(out_path, "w"), indent=1)
    print(json.dumps(results["kernels_10_minutes"], indent=1))
    return 0


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
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(results, open(out_path, "w"), indent=1)
    print("wrote", out_path, flush=True)
    return trace(out_path)


if __name__ == "__main__":
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "beat_bench.json"))
    if "--trace" in sys.argv:
        sys.exit(trace(out))
    if "--workload" in sys.argv:
        sys.exit(child(sys.argv[sys.argv.index("--workload") + 1], "--profile" in sys.argv))
    sys.exit(launcher(out))
