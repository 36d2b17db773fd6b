"""Host note metrics (yourmt3_amd/metrics.py, the specification) against the device call (include/ymt3.h, note metrics) on the same inputs.

The two workloads of scripts/gpu_detok_bench.py (its generator and seed): their ids are detokenised on the host, the notes are the ESTIMATE,
and the REFERENCE is a copy perturbed with seed 20261018 (10 % of the notes dropped, 60 % of the onsets moved by up to 7 grid steps and of
the offsets by up to 30, 5 % re-pitched, 10 % added).  Timed in one process per workload, 5 interleaved repetitions after a warm-up, medians,
the device synchronised inside every timed region:
  host     note_metrics(ref, est, n_programs) on NOTE_RECORD arrays
  device   upload of both record arrays, NoteMetrics.run, copy back of the counts -- each timed separately (a host clock around a device
           synchronise; the kernels also by device events).
The only comparison is host specification against device path: the parent commit has no such call.

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout`; a step that fails ends the run.
Output: profiles/metrics_bench.json (OUT=... for another path)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SEED = 20261018
REPS = 5


def perturbed(rng, rec):
    """a reference for the estimate `rec` (NOTE_RECORD array): dropped, moved, re-pitched and added notes, shuffled"""
    import numpy as np
    keep = rec[rng.random(rec.size) >= 0.1].copy()
    move = rng.random(keep.size) < 0.6
    keep["onset"] += np.where(move, rng.integers(-7, 8, keep.size), 0) / 100
    move = rng.random(keep.size) < 0.6
    keep["offset"] += np.where(move, rng.integers(-30, 31, keep.size), 0) / 100
    repitch = rng.random(keep.size) < 0.05
    keep["pitch"] = np.where(repitch, (keep["pitch"] + 1) % 128, keep["pitch"])
    extra = rec[rng.integers(0, rec.size, rec.size // 10)].copy()
    extra["onset"] += rng.integers(-20, 21, extra.size) / 100
    extra["offset"] += rng.integers(-20, 21, extra.size) / 100
    out = np.concatenate([keep, extra])
    return out[rng.permutation(out.size)]


def child(name):
    import numpy as np
    import torch
    import gpu_detok_bench as DB
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.metrics import note_metrics, to_records
    from yourmt3_amd.model import YourMT3
    from yourmt3_amd.task_manager import TaskManager
    w = DB.WORKLOADS[name]
    tm = TaskManager(w["task"])
    tokens_np, starts, end_sec, _ = DB.build_tokens(tm, w)
    est = to_records(tm.tokens_to_notes([tokens_np], starts, end_sec))
    ref = perturbed(np.random.default_rng(SEED), est)
    lo, hi = tm.codec.range_of("program")
    n_programs = hi - lo
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_enc_layers=1, n_dec_layers=1, n_channels=w["channels"])    # only the handle matters here
    m = YourMT3(cfg, max_batch=1)
    nm = m.compile_note_metrics(n_programs, ref.size, est.size)
    ref_bytes, est_bytes = (torch.from_numpy(r.view(np.uint8).reshape(-1).copy()) for r in (ref, est))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    times = {"host": [], "upload": [], "kernels": [], "kernels_by_events": [], "copy_back": []}
    reps = int(os.environ.get("REPS", REPS))
    want = got = None
    for rep in range(reps + 1):                                   # (the first pass warms up)
        th, want = wall(lambda: note_metrics(ref, est, n_programs))
        tu, (rd, ed) = wall(lambda: (ref_bytes.cuda(), est_bytes.cuda()))
        tk, counts = wall(lambda: nm.run(rd, ed))
        tc, got = wall(lambda: counts.cpu().numpy())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        nm.run(rd, ed)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            for k, v in (("host", th), ("upload", tu), ("kernels", tk), ("copy_back", tc), ("kernels_by_events", e0.elapsed_time(e1) / 1e3)):
                times[k].append(v)
    med = {k: float(np.median(v)) for k, v in times.items()}
    device = med["upload"] + med["kernels"] + med["copy_back"]
    res = {"workload": f"{w['n']} segments x {w['channels']} channels x {w['L']} columns ({w['task']}), detok seed {DB.SEED}, reference seed {SEED}, "
                       f"{reps} interleaved repetitions (medians)",
           "n_ref": int(ref.size), "n_est": int(est.size), "counts_equal_host": bool(np.array_equal(got, want.flat())),
           "onset_f": round(want.onset_f, 4), "offset_f": round(want.offset_f, 4), "drum_onset_f": round(want.drum_onset_f, 4),
           "host_s": round(med["host"], 5), "device_s": round(device, 6), "host_over_device": round(med["host"] / device, 1),
           "device_parts_s": {"upload": round(med["upload"], 6), "kernels": round(med["kernels"], 6), "copy_back": round(med["copy_back"], 6),
                              "stream_work_by_device_events": round(med["kernels_by_events"], 6)},
           "host_s_all": [round(x, 4) for x in times["host"]], "kernels_s_all": [round(x, 6) for x in times["kernels"]]}
    nm.close()
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if res["counts_equal_host"] else 3


def launcher():
    import gpu_detok_bench as DB
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "metrics_bench.json"))
    results = {}
    me = os.path.abspath(__file__)
    for name in DB.WORKLOADS:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, me, "--workload", name], capture_output=True, text=True, cwd=ROOT)
        line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(r.stdout[-4000:], r.stderr[-4000:], sep="\n")
            print(f"{name}: exit status {r.returncode}; nothing further is started")
            return r.returncode or 1
        results[name] = json.loads(line[len("RESULT "):])
        print(name, json.dumps(results[name]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(results, open(out_path, "w"), indent=1)
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    sys.exit(child(sys.argv[sys.argv.index("--workload") + 1]) if "--workload" in sys.argv else launcher())
