"""Shared, deterministic cases of the note velocities (yourmt3_amd/velocity.py; include/ymt3.h, note velocities) for
tests/test_velocity_cpu.py (the specification itself, and the conditions the cases must meet) and tests/test_velocity.py (the device
against the specification).  The reference of every comparison is the host specification, velocity.note_velocities / note_energies.

A case: {"id", "audio" f32 (n,), "rec" NOTE_RECORD array, "params" (velocity.DEFAULTS' keys), "count" (None, or the value of the device
count: min(n, max(count, 0)) records are live)}.  The sample rate is SR throughout.

The audio (4.5 s): chords of decaying sinusoids at note pitches, one chord every 100 ms over the first 3 s, the chords' amplitudes spread
over 40 dB, the notes of a chord alike (a note 40 dB under its neighbour in the same window has E << P, and its velocity then hangs on
the last bits of the sum: such notes are what the 5 % condition below keeps rare); one isolated note at 3.2 s; broadband bursts for
the drums from 3.5 s on, their amplitudes spread over 40 dB as well; -60 dB noise everywhere.

The tolerance.  F32_ERROR is the largest |E_f32 - E_f64| / max(P, 1e-12) over all measured records of all cases, E_f32 being the
specification restated in numpy f32 (energies_f32 below), as test_velocity_cpu.py measures it: 2.49e-7 when this was written (a drum of window_64),
recorded here rounded up to one digit.  TAU = 16 * F32_ERROR is the device's bound (it sums in another order and uses another sincos); test_velocity_cpu.py fails if
the restatement's error ever exceeds F32_ERROR."""
import functools
import math

import numpy as np

from yourmt3_amd import velocity as V
from yourmt3_amd.task_manager import NOTE_RECORD

SR = 16000
F32_ERROR = 3e-7
TAU = 16 * F32_ERROR
N_AUDIO = int(4.5 * SR)
ISOLATED_SEC = 3.2
CHORDS = 30


def rec(onset, pitch, program=0, is_drum=0, offset=None):
    return (onset, onset + 0.1 if offset is None else offset, program, pitch, is_drum, float("nan"))


def records(rows) -> np.ndarray:
    return np.array(list(rows), NOTE_RECORD)


@functools.lru_cache(maxsize=None)
def _base():
    """-> (audio, pitched records (257: the chords' notes in time order, the isolated one last), drum records (24))"""
    rng = np.random.default_rng(20240521)
    t = np.arange(N_AUDIO) / SR
    x = 1e-3 * rng.standard_normal(N_AUDIO)
    notes = []
    per_chord = [9] * 16 + [8] * 14                                       # 256 notes
    levels = rng.permutation(np.linspace(0.0, -40.0, CHORDS))
    for j in range(CHORDS):
        on = round((0.02 + 0.1 * j) * SR) / SR
        amp = 0.08 * 10.0 ** (levels[j] / 20.0)
        pitches = rng.choice(np.arange(36, 97), per_chord[j], replace=False)
        for p in sorted(pitches.tolist()):
            f = V.pitch_hz(p)
            a = amp * 10.0 ** (rng.uniform(-1.5, 1.5) / 20.0)
            x += np.where(t >= on, a * np.exp(-(t - on) / 0.012) * np.sin(2 * np.pi * f * (t - on) + rng.uniform(0, 2 * np.pi)), 0.0)
            notes.append(rec(on, p, program=int(rng.integers(0, 100))))
    x += np.where(t >= ISOLATED_SEC, 0.05 * np.exp(-(t - ISOLATED_SEC) / 0.05) * np.sin(2 * np.pi * V.pitch_hz(69) * (t - ISOLATED_SEC)), 0.0)
    notes.append(rec(ISOLATED_SEC, 69))
    drums = []
    for j in range(24):
        on = round((3.5 + 0.04 * j) * SR) / SR
        n0 = int(round(on * SR))
        amp = 0.3 * 10.0 ** (-40.0 * ((j * 7) % 24) / 23.0 / 20.0)
        burst = amp * rng.standard_normal(400) * np.exp(-np.arange(400) / 120.0)
        x[n0:n0 + 400] += burst
        drums.append(rec(on, 35 + j, program=128, is_drum=1))
    return x.astype(np.float32), records(notes), records(drums)


def edge_records(n_audio: int = N_AUDIO) -> np.ndarray:
    """every edge of the rules, on the base audio"""
    end = n_audio / SR
    return records([
        rec(-0.01, 60),                         # the window starts before sample 0
        rec(-1024 / SR, 60),                    # ... and ends exactly there: all zeros
        rec((n_audio - 300) / SR, 62),          # crosses n_audio
        rec(end, 62),                           # starts at the end
        rec(end + 5.0, 64),                     # wholly past the end
        rec(float("inf"), 60), rec(float("-inf"), 60), rec(float("nan"), 60), rec(1e300, 60), rec(-1e300, 60),
        rec(0.5 / SR, 60), rec(1.5 / SR, 60),   # half samples: 0.5 rounds to 0, 1.5 to 2
        rec(0.32, -1), rec(0.32, 128), rec(0.32, 0),
        rec(0.32, 108),                         # only the fundamental lies below Nyquist
        rec(0.32, 127),                         # 12.5 kHz: not measured at 16 kHz
        rec(0.32, 127, program=128, is_drum=1),  # ... but a drum is
        rec(0.32, 40, program=5, is_drum=1),    # is_drum with a foreign program
        rec(0.32, 40, program=128, is_drum=0),  # the drum program without is_drum
        rec(0.32, 128, program=128, is_drum=1), rec(float("nan"), 40, is_drum=1),
        rec(0.32, 60, offset=float("nan")),     # the offset is not read
        rec(0.32, 60, offset=0.0),
    ])


def cases():
    audio, pitched, drums = _base()
    mixed = np.concatenate([pitched[:200], drums, pitched[200:]])[np.random.default_rng(5).permutation(257 + 24)]
    out = []

    def add(id, rec, audio=audio, count=None, **params):
        out.append({"id": id, "audio": audio, "rec": rec, "params": params, "count": count})

    for n in (0, 1, 4, 5, 65, 257):             # a partial workgroup, more than one workgroup, many workgroups
        add(f"n_{n}", mixed[:n])
    for W in (64, 96, 1000, 4096):
        add(f"window_{W}", mixed[:65], window_samples=W)
    add("harmonics_1", mixed[:65], n_harmonics=1)
    add("harmonics_8", mixed[:65], n_harmonics=8)
    add("edges", np.concatenate([edge_records(), mixed[:20]]))
    add("edges_window_4096_harmonics_8", np.concatenate([mixed[:9], edge_records()]), window_samples=4096, n_harmonics=8)
    add("only_drums", drums)
    add("only_pitched", pitched[100:165])
    add("peak_db", mixed[:65], peak_db=-20.0)
    add("peak_db_loud", mixed[:65], peak_db=-60.0)                      # most notes above the reference: clamped at 127
    add("mapping", mixed[:65], velocity_per_db=1.5, peak_velocity=127, min_velocity=40, default_velocity=64)
    add("drum_program_5", np.concatenate([edge_records(), mixed[:12]]), drum_program=5)
    tail = np.concatenate([mixed[:30], pitched[-1:], mixed[30:40]])      # the isolated note among others
    for name, bad in (("nan_sample", np.nan), ("inf_sample", np.inf), ("minus_inf_sample", -np.inf)):
        spoiled = audio.copy()
        spoiled[int(ISOLATED_SEC * SR) + 500] = bad                         # under the isolated note's window and no other's
        add(name, tail, audio=spoiled)
    add("zero_audio", mixed[:33], audio=np.zeros(8000, np.float32))
    add("no_audio", mixed[:5], audio=np.zeros(0, np.float32))
    for count in (0, -3, 40, 65, 165):
        add(f"count_{count}", mixed[:65], count=count)
    return out


def live(case) -> int:
    n = case["rec"].size
    return n if case["count"] is None else min(n, max(case["count"], 0))


def compute(case):
    """the specification's answer for the case's live records: vel, E, peaks, counts, P, drum (read-only arrays)"""
    rec = case["rec"][:live(case)]
    vel, E, peaks, counts = V.note_velocities(case["audio"], SR, rec, **case["params"])
    _, P, drum = V.note_energies(case["audio"], SR, rec, **case["params"])
    for a in (vel, E, peaks, counts, P, drum):
        a.setflags(write=False)
    return {"vel": vel, "E": E, "peaks": peaks, "counts": counts, "P": P, "drum": drum}


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    return compute(next(c for c in cases() if c["id"] == case_id))


def reference(case):
    """compute(case), once per named case; a case made on the spot (its id is None) carries its own under the key ref"""
    if case["id"] is None:
        if "ref" not in case:
            case["ref"] = compute(case)
        return case["ref"]
    return _reference(case["id"])


def energies_f32(case) -> np.ndarray:
    """The specification's energies restated in numpy f32, every product, sum and angle: what an f32 implementation can be expected to
    give.  NaN where the specification has NaN."""
    p = V.check_params(SR, **case["params"])
    rec = case["rec"][:live(case)]
    x, W, H = case["audio"], int(p["window_samples"]), int(p["n_harmonics"])
    w, steps, sw, sw2 = V.velocity_tables(SR, W, H)
    ref = reference(case)
    k = np.arange(W, dtype=np.uint64)
    f32 = np.float32
    out = np.full(rec.size, np.nan, f32)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(~np.isnan(ref["E"])):
            lo = int(min(max(np.rint(rec["onset"][i] * float(SR)), -float(W)), float(x.size)))
            seg = np.zeros(W, f32)
            a0, a1 = max(lo, 0), min(lo + W, x.size)
            if a0 < a1:
                seg[a0 - lo:a1 - lo] = x[a0:a1]
            a = w * seg
            if ref["drum"][i]:
                out[i] = np.sum(a * a, dtype=f32) * f32(2.0 / sw2)
                continue
            e = f32(0)
            for h in range(H):
                step = int(steps[int(rec["pitch"][i]), h])
                if step == 0:
                    continue
                phi = ((np.uint64(step) * k) & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)
                theta = (phi.astype(f32) * f32(2.0 ** -31)) * f32(math.pi)
                re, im = np.sum(a * np.cos(theta), dtype=f32), np.sum(a * np.sin(theta), dtype=f32)
                e = e + re * re + im * im
            out[i] = e * f32(4.0 / (sw * sw))
    return out


def admissible(case, tau: float = TAU):
    """Per live record the (lo, hi) range of velocities an implementation may give whose energies and peaks lie within tau * max(P, 1e-12)
    of the specification's: the clamped roundings of u over that interval, widened by 1e-9 for the f64 log10.  Unmeasured records:
    (default_velocity, default_velocity)."""
    p = V.check_params(SR, **case["params"])
    ref = reference(case)
    E, P, drum, peaks = ref["E"], ref["P"], ref["drum"], ref["peaks"]
    measured = ~np.isnan(E)
    floor = V.ENERGY_FLOOR
    span = []
    for cls in (0, 1):
        if math.isfinite(p["peak_db"]):
            r = math.pow(10.0, p["peak_db"] / 10.0)
            span.append((r, r))
            continue
        idx = np.flatnonzero(measured & (drum == bool(cls)))
        slack = tau * max(float(P[idx[np.argmax(E[idx])]]), floor) if idx.size else 0.0
        span.append((max(float(peaks[cls]) - slack, 0.0), float(peaks[cls]) + slack))
    db = lambda v: 10.0 * math.log10(max(v, floor))
    pv, vpd, mn = int(p["peak_velocity"]), float(p["velocity_per_db"]), int(p["min_velocity"])
    clamp = lambda u: int(min(max(np.rint(u), float(mn)), 127.0))
    out = []
    for i in range(E.size):
        if not measured[i]:
            out.append((int(p["default_velocity"]),) * 2)
            continue
        slack = tau * max(float(P[i]), floor)
        r_lo, r_hi = span[int(drum[i])]
        u_lo = pv + vpd * (db(max(float(E[i]) - slack, 0.0)) - db(r_hi)) - 1e-9
        u_hi = pv + vpd * (db(float(E[i]) + slack) - db(r_lo)) + 1e-9
        out.append((clamp(u_lo), clamp(u_hi)))
    return out


def peak_slack(case, tau: float = TAU):
    """tau * max(P, 1e-12) of the record that holds each class's peak (0 for an empty class)"""
    ref = reference(case)
    measured = ~np.isnan(ref["E"])
    out = []
    for cls in (0, 1):
        idx = np.flatnonzero(measured & (ref["drum"] == bool(cls)))
        out.append(tau * max(float(ref["P"][idx[np.argmax(ref["E"][idx])]]), V.ENERGY_FLOOR) if idx.size else 0.0)
    return out
