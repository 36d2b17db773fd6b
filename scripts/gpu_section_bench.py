"""Host section tracking (track_sections of yourmt3_amd/sections.py, the specification) against the device call (SectionTracker.track;
include/ymt3.h, sections) on the same records, beats and metre, at the default parameters (100 frames per second), with the chord
tracker's time for the same workload beside it.

The workloads are those of scripts/gpu_bar_bench.py (notes_of there; seed 20261020):
  3_minutes    18 000 frames
  10_minutes   60 000 frames
The beats are the device beat tracker's and the metre the device bar tracker's, both left on the device.  Timed in one process per
workload after a warm-up:
  host     track_sections(records, beats, n_frames, metre): a host clock, median of HOST_REPS
  device   SectionTracker.track (and ChordTracker.track): device events around CALLS back-to-back calls, divided by CALLS; medians of REPS
PARAMS (a JSON object) times another parameter set beside the defaults, e.g. the largest kernel: PARAMS='{"kernel_beats": 64, "context": 16}'.
The only comparison is host specification against device path: the parent commit has no such call.  No ratio is promised.

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout`; a step that fails ends the run.
BENCH_THIS / BENCH_PARENT: files holding bench.py's JSON lines of this commit and of its parent (runs taken in turn on one machine); their
time per step and headline value are recorded beside the timings as "bench".
Output: profiles/section_bench.json (OUT=... for another path)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_bar_bench import CALLS, FPS, HOST_REPS, REPS, SEED, WORKLOADS, notes_of  # noqa: E402


def child(name):
    import numpy as np
    import torch
    from yourmt3_amd.beats import max_beats
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.model import YourMT3
    from yourmt3_amd.sections import section_names, section_segments, track_sections
    seconds = WORKLOADS[name][0]
    rec, n_frames = notes_of(seconds)[0], int(seconds * FPS)
    params = json.loads(os.environ.get("PARAMS", "{}"))
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_enc_layers=1, n_dec_layers=1)    # only the handle matters here
    m = YourMT3(cfg, max_batch=1)
    bt = m.compile_beat_tracker(n_frames)
    cap = max_beats(n_frames, bt.lag_min)
    br, ct, st = m.compile_bar_tracker(cap, int(rec.size)), m.compile_chord_tracker(cap, int(rec.size)), m.compile_section_tracker(cap, int(rec.size))
    wide = m.compile_section_tracker(cap, int(rec.size), **params) if params else None
    rd = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    beats_dev, _, beat_result = bt.track(rd, n_frames)
    metre_dev, _ = br.track(beats_dev, beat_result, rd, n_frames)
    calls = {"sections": lambda: st.track(beats_dev, beat_result, metre_dev, rd, n_frames),
             "chords": lambda: ct.track(beats_dev, beat_result, metre_dev, rd, n_frames)}
    if wide is not None:
        calls["sections_params"] = lambda: wide.track(beats_dev, beat_result, metre_dev, rd, n_frames)
    reps = int(os.environ.get("REPS", REPS))
    times = {}
    for label, track in calls.items():
        track()                                                   # warm-up: code objects, the allocator's blocks
        torch.cuda.synchronize()
        times[label] = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                track()
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) / 1e3 / CALLS)
        print(f"{name}: device {label} {sorted(times[label])} s per call", flush=True)
    k = int(beat_result.cpu()[0])
    beats, metre = beats_dev[:k].cpu().numpy(), metre_dev[:k].cpu().numpy()
    host, host_params = [], []
    for _ in range(int(os.environ.get("HOST_REPS", HOST_REPS))):
        t0 = time.perf_counter()
        want = track_sections(rec, beats, n_frames, metre=metre)
        host.append(time.perf_counter() - t0)
        print(f"{name}: host {host[-1]:.3f} s", flush=True)
    equal = True
    for label, kw in (("sections", {}), ("sections_params", params)):
        if label not in calls:
            continue
        t0 = time.perf_counter()
        ref = track_sections(rec, beats, n_frames, metre=metre, **kw)
        if kw:
            host_params.append(time.perf_counter() - t0)
        section_dev, result_dev, nov_dev = calls[label]()
        got = section_dev[:k].cpu().numpy(), nov_dev[:k].cpu().numpy(), result_dev.cpu().numpy()
        equal = equal and all(g.tolist() == w.tolist() for g, w in zip(got, ref))
    med = lambda v: float(np.median(v))
    res = {"workload": f"{rec.size} notes, {n_frames} frames at {FPS:g} per second, default parameters, seed {SEED}; device: events around {CALLS} calls, "
                       f"median of {reps}; host: median of {len(host)}",
           "n_notes": int(rec.size), "n_frames": n_frames, "n_beats": k, "n_sections": int(want[2][0]), "n_letters": int(want[2][1]), "n_peaks": int(want[2][4]),
           "form": "".join(section_names(label) for _, _, label in section_segments(want[0], beats))[:64],
           "device_equals_host": equal, "host_s": round(med(host), 4), "device_track_s": round(med(times["sections"]), 7),
           "device_track_chords_s": round(med(times["chords"]), 7), "host_s_all": [round(x, 4) for x in host],
           "device_track_s_all": [round(x, 7) for x in times["sections"]], "device_track_chords_s_all": [round(x, 7) for x in times["chords"]]}
    if wide is not None:
        res.update(params=params, host_params_s=round(med(host_params), 4), device_track_params_s=round(med(times["sections_params"]), 7),
                   device_track_params_s_all=[round(x, 7) for x in times["sections_params"]])
    for o in (wide, st, ct, br, bt, m):
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
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "section_bench.json"))
    if "--workload" in sys.argv:
        sys.exit(child(sys.argv[sys.argv.index("--workload") + 1]))
    sys.exit(launcher(out))
