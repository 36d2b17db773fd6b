"""Case sets for the beat tracker (tests/test_beats_cpu.py, tests/test_beats.py): NOTE_RECORD arrays, frame counts and parameter sets, all
small.  A case: (name, records, n_frames, params, count) with `count` the device count to pass (None: all records)."""
import math

import numpy as np

from yourmt3_amd.task_manager import NOTE_RECORD

FPS = 100.0
LAG_MIN, LAG_MAX, G, HN, WN = 25, 150, 13, 100, 800        # at the defaults
SECOND = dict(frames_per_second=50.0, lag_step_max=1, window_frames=400, hop_frames=50)      # lags 13 .. 75, G = 7
LOOSE = dict(tightness=0.001)                             # every penalty rounds to 0: ties between predecessors everywhere


def records(onsets, pitch=60, length=0.1, program=0, drum=False):
    rec = np.zeros(len(onsets), NOTE_RECORD)
    rec["onset"] = onsets
    rec["offset"] = np.asarray(onsets, np.float64) + length
    rec["program"], rec["pitch"], rec["is_drum"], rec["score"] = program, pitch, drum, np.nan
    return rec


def clicks(period_sec, first=0.5, dur=12.5):
    return np.arange(first, dur - 1e-9, period_sec)


def metronome(bpm, first=0.5, dur=12.5):
    """-> (records, n_frames, the clicks' frames)"""
    t = clicks(60.0 / bpm, first, dur)
    return records(t), int(round(dur * FPS)), np.rint(t * FPS).astype(np.int64)


METRONOME_BPM = (60, 80, 100, 120, 150)                   # whole-frame periods: 100, 75, 60, 50, 40 frames


def tempo_step():
    """90 bpm for 15 s, then 132 bpm for 15 s -> (records, n_frames, beat times)"""
    a = np.arange(0.5, 15.0, 60.0 / 90)
    b = np.arange(a[-1] + 60.0 / 132, 30.0, 60.0 / 132)
    t = np.concatenate([a, b])
    return records(t), 3000, t


def accelerando():
    """80 -> 120 bpm, linear in time over 30 s -> (records, n_frames, beat times)"""
    t, out = 0.5, []
    while t < 30.0:
        out.append(t)
        t += 60.0 / (80.0 + 40.0 * t / 30.0)
    t = np.array(out)
    return records(t), 3000, t


def music_like():
    """100 bpm for 20 s: a chord on every beat, an off-beat eighth on most, a drum on every second beat, 10 ms jitter"""
    rng = np.random.default_rng(22)
    beats = np.arange(0.4, 20.0, 0.6)
    parts = []
    for k, b in enumerate(beats):
        for pitch in (48, 60, 64, 67):
            parts.append((b + rng.normal(0, 0.01), pitch, 0, False))
        if rng.random() < 0.7:
            parts.append((b + 0.3 + rng.normal(0, 0.01), 72, 0, False))
        if k % 2 == 0:
            parts.append((b + rng.normal(0, 0.01), 36, 128, True))
    rec = np.zeros(len(parts), NOTE_RECORD)
    for i, (t, pitch, prog, drum) in enumerate(parts):
        rec[i] = (t, t + 0.25, prog, pitch, drum, np.nan)
    return rec, 2000, beats


def _random(seed, max_notes=400, max_frames=3000):
    rng = np.random.default_rng(1000 + seed)
    n, frames = int(rng.integers(0, max_notes + 1)), int(rng.integers(1, max_frames + 1))
    period = rng.uniform(0.3, 1.2)
    on = np.where(rng.random(n) < 0.6, np.rint(rng.uniform(0, frames / FPS / period, n)) * period, rng.uniform(-0.5, frames / FPS + 0.5, n))
    on = on + rng.normal(0, 0.008, n)
    rec = records(on, pitch=rng.integers(-2, 130, n), length=rng.uniform(0.02, 1.0, n), program=rng.integers(-1, 132, n))
    rec["is_drum"] = rng.random(n) < 0.15
    return rec, frames


def edge_cases():
    out = []
    some = records([0.0, 0.05, 0.11, 0.5, 0.93, 1.5, 2.0, 2.49, 3.0, 3.99, 4.0, 7.99, 8.0])
    for n_frames in (1, LAG_MIN - 1, G - 1, G, G + 1, HN - 1, HN, HN + 1, WN // 2, WN + 1):
        out.append((f"frames{n_frames}", some, n_frames, {}, None))
    out.append(("no_notes", records([]), 500, {}, None))
    out.append(("one_note", records([1.234]), 500, {}, None))
    out.append(("cap_300_in_one_frame", np.concatenate([records([2.0] * 300, pitch=np.arange(300) % 128), records([1.0, 3.0, 4.0])]), 600, {}, None))
    out.append(("clicks_at_lag_min", records(clicks(LAG_MIN / FPS, 0.25, 8.0)), 800, {}, None))
    out.append(("clicks_at_lag_max", records(clicks(LAG_MAX / FPS, 0.5, 16.0)), 1600, {}, None))
    out.append(("equal_predecessors", _random(77)[0], 1500, LOOSE, None))
    out.append(("silence_10s", records(np.concatenate([clicks(0.5, 0.5, 6.0), clicks(0.4, 16.0, 22.0)])), 2200, {}, None))
    bad = records([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0])
    bad["onset"][1], bad["onset"][3], bad["onset"][5] = np.nan, np.inf, -np.inf
    bad["program"][6], bad["program"][7], bad["pitch"][8] = 130, -1, 128
    bad["offset"][9] = np.nan
    out.append(("nonfinite_and_out_of_range", bad, 600, {}, None))
    out.append(("count_below_n", records(clicks(0.5, 0.5, 10.0)), 1000, {}, 11))
    out.append(("count_zero", records(clicks(0.5, 0.5, 10.0)), 1000, {}, 0))
    out.append(("second_params", records(clicks(0.44, 0.3, 12.0)), 600, SECOND, None))
    out.append(("second_params_random", _random(5)[0], 433, SECOND, None))
    return out


def musical_cases():
    out = [(f"metronome{bpm}", metronome(bpm)[0], metronome(bpm)[1], {}, None) for bpm in METRONOME_BPM + (200,)]
    for name, make in (("tempo_step", tempo_step), ("accelerando", accelerando), ("music_like", music_like)):
        rec, n_frames, _ = make()
        out.append((name, rec, n_frames, {}, None))
    return out


def random_cases():
    return [(f"random{seed}", *_random(seed), {}, None) for seed in range(20)]


def all_cases():
    return musical_cases() + edge_cases() + random_cases()


def live(rec, count):
    """the records a case's count leaves"""
    return rec if count is None else rec[:max(0, min(len(rec), count))]


def beat_f_measure(est_sec, ref_sec, tol=0.07):
    """one-to-one within `tol`: both lists ascend, so the greedy sweep is a maximum matching"""
    est, ref = list(est_sec), list(ref_sec)
    i = j = hits = 0
    while i < len(est) and j < len(ref):
        if abs(est[i] - ref[j]) <= tol:
            hits, i, j = hits + 1, i + 1, j + 1
        elif est[i] < ref[j]:
            i += 1
        else:
            j += 1
    return 2.0 * hits / (len(est) + len(ref)) if est and ref else 0.0
