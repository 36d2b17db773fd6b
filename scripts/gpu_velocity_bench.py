"""Host note velocities (yourmt3_amd/velocity.py, the specification) against the device call (include/ymt3.h, note velocities) on the same
input.

One workload (seed 20261019): 10 minutes of synthetic audio at 16 kHz -- 20 000 decaying sinusoids at note pitches, amplitudes spread over
40 dB, plus 1 200 broadband bursts and -60 dB noise -- and one record per sinusoid and per burst, in random order; the default parameters
(a window of 1024 samples, 4 harmonics).
Timed in one process, audio and records already on the device, after a warm-up:
  device   NoteVelocity.run with and without the energies (the second is the same call; the C ABI's NULL energy buffer, which measures
           twice, is timed through ctypes): device events around each single call, the median of RUNS
  host     note_velocities(...) once: a host clock
The only comparison is host specification against device path: the parent commit has no such call.  No ratio is promised.

Run without arguments this file is the launcher: the workload is a fresh process under its own `timeout`.  `--child --profile` runs every
device call once after a warm-up and nothing else: the process to put under a kernel trace.
Output: profiles/velocity_bench.json (OUT=... for another path)."""
import ctypes, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261019
RUNS = 30
SR = 16000
SECONDS = 600
N_TONES, N_BURSTS = 20000, 1200


def workload():
    import numpy as np
    from yourmt3_amd.task_manager import NOTE_RECORD
    from yourmt3_amd.velocity import pitch_hz
    rng = np.random.default_rng(SEED)
    n = SECONDS * SR
    x = 1e-3 * rng.standard_normal(n)
    rec = np.zeros(N_TONES + N_BURSTS, NOTE_RECORD)
    span = int(0.25 * SR)                                                   # a tone is written over 250 ms (decay 40 ms)
    t = np.arange(span) / SR
    starts = rng.integers(0, n - span, N_TONES)
    pitches = rng.integers(28, 100, N_TONES)
    amps = 0.3 * 10.0 ** (-40.0 * rng.random(N_TONES) / 20.0)
    for i in range(N_TONES):
        x[starts[i]:starts[i] + span] += amps[i] * np.exp(-t / 0.04) * np.sin(2 * np.pi * pitch_hz(int(pitches[i])) * t + rng.uniform(0, 2 * np.pi))
    rec["onset"][:N_TONES], rec["pitch"][:N_TONES], rec["program"][:N_TONES] = starts / SR, pitches, rng.integers(0, 128, N_TONES)
    b_starts = rng.integers(0, n - 400, N_BURSTS)
    b_amps = 0.3 * 10.0 ** (-40.0 * rng.random(N_BURSTS) / 20.0)
    for i in range(N_BURSTS):
        x[b_starts[i]:b_starts[i] + 400] += b_amps[i] * rng.standard_normal(400) * np.exp(-np.arange(400) / 120.0)
    rec["onset"][N_TONES:], rec["pitch"][N_TONES:], rec["program"][N_TONES:], rec["is_drum"][N_TONES:] = b_starts / SR, rng.integers(35, 82, N_BURSTS), 128, 1
    rec["offset"] = rec["onset"] + 0.2
    rec["score"] = np.nan
    return x.astype(np.float32), rec[rng.permutation(rec.size)]


def child(profile):
    import numpy as np
    import torch
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.model import YourMT3
    from yourmt3_amd.velocity import note_energies, note_velocities
    audio, rec = workload()
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_enc_layers=1, n_dec_layers=1)    # only the handle matters here
    m = YourMT3(cfg, max_batch=1)
    nv = m.compile_note_velocity()
    ad, rd = torch.from_numpy(audio).cuda(), torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    n = int(rec.size)
    vel, peaks, counts = torch.empty(n, dtype=torch.uint8).cuda(), torch.empty(2).cuda(), torch.empty(2, dtype=torch.int32).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def twice():                                                            # energy_dev = NULL: the second kernel measures again
        rc = m._lib.ymt3_note_velocities(m._handle, nv.ptr, p(ad), ad.numel(), p(rd), n, None, p(vel), None, p(peaks), p(counts), m._stream())
        assert rc == 0, m._lib.ymt3_last_error()
        return vel
    calls = {"run": lambda: nv.run(ad, rd), "run_energies": lambda: nv.run(ad, rd, energies=True), "c_abi_null_energy": twice}
    for fn in calls.values():                                               # warm-up: code objects, the allocator's blocks
        fn()
    torch.cuda.synchronize()
    if profile:
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        nv.close()
        m.close()
        return 0
    runs = int(os.environ.get("RUNS", RUNS))
    times = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / 1e3)
            del out
    t0 = time.perf_counter()
    want_vel, want_e, want_peaks, want_counts = note_velocities(audio, SR, rec)
    host_s = time.perf_counter() - t0
    _, power, _ = note_energies(audio, SR, rec)
    got_vel, got_e, got_peaks, got_counts = (t.cpu().numpy() for t in nv.run(ad, rd, energies=True))
    measured = ~np.isnan(want_e)
    split = bool(np.array_equal(~np.isnan(got_e), measured))
    err = np.abs(got_e[measured].astype(np.float64) - want_e[measured]) / np.maximum(power[measured], 1e-12) if split else np.array([np.inf])
    differ = int((got_vel != want_vel).sum())
    ok = split and got_counts.tolist() == want_counts.tolist() and bool(np.array_equal(twice().cpu().numpy(), got_vel))
    med = lambda v: float(np.median(v))
    res = {"workload": f"{SECONDS} s of synthetic audio at {SR} Hz ({audio.size} samples), {N_TONES} decaying sinusoids over 40 dB + {N_BURSTS} bursts + -60 dB noise, "
                       f"{n} records in random order, seed {SEED}; window 1024, 4 harmonics; device: events around one call, medians of {runs}; host: one run",
           "n_notes": n, "n_audio": int(audio.size), "counts": got_counts.tolist(), "counts_equal_host": got_counts.tolist() == want_counts.tolist(),
           "split_equals_host": split, "null_energy_call_same_bytes": ok,
           "largest_energy_error_over_window_power": float(err.max()), "velocities_differing_from_host": differ,
           "velocities_min_max": [int(got_vel.min()), int(got_vel.max())], "distinct_velocities": int(np.unique(got_vel).size),
           "host_s": round(host_s, 3),
           "device_s": {k: round(med(v), 7) for k, v in times.items()},
           "device_s_min_max": {k: [round(min(v), 7), round(max(v), 7)] for k, v in times.items()}}
    nv.close()
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if ok else 3


def launcher():
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "velocity_bench.json"))
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, cwd=ROOT)
    line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        print(r.stdout[-4000:], r.stderr[-4000:], sep="\n")
        print(f"exit status {r.returncode}")
        return r.returncode or 1
    res = json.loads(line[len("RESULT "):])
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        sys.exit(child("--profile" in sys.argv))
    sys.exit(launcher())
