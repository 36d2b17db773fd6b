"""Beat tracking over note records: a tempo per window, the beats' frames, every note's position in beats (include/ymt3.h, beat tracking;
DESIGN section 22).

The vocabulary carries no metre, so a transcription's MIDI file has had a fixed 120 bpm whatever the music does.  The notes carry it: their
onsets are an onset-strength signal.  The rules below are this repository's own, shaped after the well-known autocorrelation plus
dynamic-programming beat tracker, written from memory and UNVERIFIED against any package.  `track_beats` and `beat_positions` are their host
specification: numpy, integers throughout except the two tables (f64 libm calls, rounded to integers once) and the position expression (f64,
no contraction).  `BeatTracker` is the device object (YourMT3.compile_beat_tracker; yourmt3_amd/csrc/beats.hip), which equals them bit for
bit.  Bars, the time signature, downbeats and the key are found on top of these beats by yourmt3_amd/bars.py.

The rules.  fps = frames_per_second, Wn = window_frames, Hn = hop_frames, D = lag_step_max; all divisions of integers below are floor
divisions.

  lags      lag_min = ceil(60 fps / bpm_max), lag_max = floor(60 fps / bpm_min), 4 <= lag_min <= lag_max <= 512 <= Wn / 2 ... Wn <= 2048.
  tables    prior[L] = rint(65535 exp(-0.5 (log2(L / L0) / prior_octaves)^2)), L0 = 60 fps / bpm_prior, L in [lag_min, lag_max];
            pen[t][d] = rint(tightness 1024 ln(d / t)^2), t in [lag_min, lag_max], d in [ceil(t / 2), 2 t].
  envelope  the counted records are those of metrics.classify (csrc/note_rule.h); the others are `skipped`.  A counted record adds 1 to
            e[F], F = rint(onset fps) in f64, if 0 <= F < n_frames (drums and pitched notes alike; an onset outside the frames adds nothing).
            e[f] = min(e[f], onset_cap); s[f] = e[f-1] + 2 e[f] + e[f+1], zeros outside [0, n_frames).
  tempogram nW = max(1, ceil(n_frames / Hn)); window w has c = w Hn + Hn / 2 and covers f in [c - Wn / 2, c + Wn / 2) within [0, n_frames);
            A[w][L] = sum of s[f] s[f+L] over the window's f with f + L < n_frames; T[w][L] = A[w][L] prior[L].
  tempo     V[0] = T[0]; V[w][L] = T[w][L] + max of V[w-1][L'] over |L' - L| <= D, L' in the lag range; ties to the nearest L', then the
            smaller.  The end is the smallest L with V[nW-1][L] maximal; tempo[w] is the lag followed back from it.
  beats     t(f) = tempo[min(f / Hn, nW - 1)]; best(f) = max of C[p] - pen[t][f-p] over p in [max(0, f - 2 t), f - ceil(t / 2)]; with
            best > 0, back[f] is the LARGEST p attaining it, else best = 0 and back[f] = -1; C[f] = 1024 s[f] + best.  The last beat is the
            SMALLEST f with C[f] maximal, the beats the chain of back[] from it, ascending; with max C = 0 (no onset in the frames) none.
  positions with K >= 2 beats b: x = t fps, i the largest index with b[i] <= x clamped to [0, K-2], n0 = ceil(b[0] / (b[1] - b[0])),
            pos = (n0 + i) + (x - b[i]) / (b[i+1] - b[i]).  Q = divisions or 480 (divisions divides 480):
            tick = clamp(rint(pos Q), 0, 2^20) (480 / Q), rint half to even.  With K < 2: tick = clamp(rint(t 960), 0, 2^29), Q = 480.
            A counted pitched note's offset tick is at least its onset tick + 480 / Q.  A NaN time, an uncounted record: -1."""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .model import _Owned
from .task_manager import DRUM_PROGRAM, NOTE_RECORD, Note

TICKS_PER_BEAT = 480
DEFAULTS = dict(frames_per_second=100.0, bpm_min=40.0, bpm_max=240.0, bpm_prior=120.0, prior_octaves=1.0, tightness=100.0, window_frames=800,
                hop_frames=100, lag_step_max=4, onset_cap=15, n_programs=DRUM_PROGRAM + 2, drum_program=DRUM_PROGRAM)
MAX_FRAMES = 1 << 20
MAX_LAG, MAX_WINDOW, MAX_PROGRAMS = 512, 2048, 256
PRIOR_ONE = 65535
SUM_LIMIT = 1 << 62                       # what the tempo path's sums may reach
TICK_GRID_MAX, TICK_FLAT_MAX = 1 << 20, 1 << 29


def with_defaults(params: dict, defaults: dict, noun: str) -> dict:
    unknown = set(params) - set(defaults)
    if unknown:
        raise TypeError(f"unknown {noun} parameter(s): {sorted(unknown)}")
    return {**defaults, **params}


def check_params(**params) -> dict:
    """the parameters with their defaults and the two derived lags, refused (ValueError naming the parameter) outside what the C ABI accepts"""
    p = with_defaults(params, DEFAULTS, "beat")
    for k in ("frames_per_second", "bpm_min", "bpm_max", "bpm_prior", "prior_octaves", "tightness"):
        if not (math.isfinite(p[k]) and p[k] > 0):
            raise ValueError(f"{k}={p[k]} must be finite and > 0")
    if not p["bpm_min"] <= p["bpm_max"]:
        raise ValueError(f"bpm_min={p['bpm_min']} above bpm_max={p['bpm_max']}")
    if not p["tightness"] <= 10000:
        raise ValueError(f"tightness={p['tightness']} above 10000")
    fps = float(p["frames_per_second"])
    lo, hi = np.ceil(60.0 * fps / float(p["bpm_max"])), np.floor(60.0 * fps / float(p["bpm_min"]))
    if not 4 <= lo <= hi <= MAX_LAG:
        raise ValueError(f"lag_min={lo:g}, lag_max={hi:g} (60 frames_per_second / bpm_max, / bpm_min) must satisfy 4 <= lag_min <= lag_max <= {MAX_LAG}")
    p["lag_min"], p["lag_max"] = int(lo), int(hi)
    if not 2 * p["lag_max"] <= int(p["window_frames"]) <= MAX_WINDOW:
        raise ValueError(f"window_frames={p['window_frames']} outside [2 * lag_max={2 * p['lag_max']}, {MAX_WINDOW}]")
    if not 1 <= int(p["hop_frames"]) <= int(p["window_frames"]):
        raise ValueError(f"hop_frames={p['hop_frames']} outside [1, window_frames={p['window_frames']}]")
    if not 0 <= int(p["lag_step_max"]) <= MAX_LAG:
        raise ValueError(f"lag_step_max={p['lag_step_max']} outside [0, {MAX_LAG}]")
    if not 1 <= int(p["onset_cap"]) <= 255:
        raise ValueError(f"onset_cap={p['onset_cap']} outside [1, 255]")
    if not 1 <= int(p["n_programs"]) <= MAX_PROGRAMS:
        raise ValueError(f"n_programs={p['n_programs']} outside [1, {MAX_PROGRAMS}]")
    if not 0 <= int(p["drum_program"]) < int(p["n_programs"]):
        raise ValueError(f"drum_program={p['drum_program']} outside [0, n_programs={p['n_programs']})")
    return p


def n_windows(n_frames: int, hop_frames: int) -> int:
    return max(1, -(-int(n_frames) // int(hop_frames)))


def check_frames(p: dict, n_frames: int, name: str = "n_frames") -> None:
    """`n_frames` (a call's, or an object's max_frames) is in [1, 2^20] and keeps the tempo path's sums below 2^62"""
    if not 1 <= int(n_frames) <= MAX_FRAMES:
        raise ValueError(f"{name}={n_frames} outside [1, {MAX_FRAMES}]")
    s_max = 4 * int(p["onset_cap"])
    if n_windows(n_frames, p["hop_frames"]) * int(p["window_frames"]) * s_max * s_max * PRIOR_ONE > SUM_LIMIT:
        raise ValueError(f"{name}={n_frames} with hop_frames={p['hop_frames']}: the tempo path's sums could pass 2^62")


def max_beats(n_frames: int, lag_min: int) -> int:
    """the bound on the number of beats of `n_frames` frames: two beats are at least ceil(lag_min / 2) frames apart"""
    return int(n_frames) // ((int(lag_min) + 1) // 2) + 1


def beat_tables(p: dict) -> Tuple[np.ndarray, np.ndarray]:
    """-> (prior int32 (nL,), pen int32 (nL, 2 lag_max + 1), row t - lag_min, column d, 0 outside [ceil(t / 2), 2 t]): every value as
    ymt3_beats_create builds it (libm's log2, exp and log, element by element)"""
    lmin, lmax, fps = p["lag_min"], p["lag_max"], float(p["frames_per_second"])
    l0, octaves, tight = 60.0 * fps / float(p["bpm_prior"]), float(p["prior_octaves"]), float(p["tightness"])
    prior = np.zeros(lmax - lmin + 1, np.int32)
    pen = np.zeros((lmax - lmin + 1, 2 * lmax + 1), np.int32)
    for lag in range(lmin, lmax + 1):
        z = math.log2(lag / l0) / octaves
        prior[lag - lmin] = int(np.rint(65535.0 * math.exp(-0.5 * (z * z))))
        for d in range((lag + 1) // 2, 2 * lag + 1):
            g = math.log(d / lag)
            pen[lag - lmin, d] = int(np.rint(tight * 1024.0 * (g * g)))
    return prior, pen


def _records(notes) -> np.ndarray:
    from .metrics import to_records
    return to_records(notes)


def onset_envelope(notes, n_frames: int, p: dict) -> Tuple[np.ndarray, int]:
    """-> (s int64 (n_frames,), the number of skipped records)"""
    from .metrics import classify, frame_of
    rec = _records(notes)
    counted, _, _ = classify(rec, int(p["n_programs"]), int(p["drum_program"]))
    f = frame_of(rec["onset"][counted], float(p["frames_per_second"]))
    f = f[(f >= 0.0) & (f < np.float64(n_frames))].astype(np.int64)
    e = np.minimum(np.bincount(f, minlength=n_frames).astype(np.int64), int(p["onset_cap"]))
    s = 2 * e
    s[1:] += e[:-1]
    s[:-1] += e[1:]
    return s, int((~counted).sum())


def tempogram(s: np.ndarray, p: dict, prior: np.ndarray) -> np.ndarray:
    """-> T int64 (nW, nL)"""
    n, wn, hn, lmin, lmax = s.size, int(p["window_frames"]), int(p["hop_frames"]), p["lag_min"], p["lag_max"]
    nw = n_windows(n, hn)
    T = np.zeros((nw, lmax - lmin + 1), np.int64)
    for w in range(nw):
        c = w * hn + hn // 2
        lo, hi = max(0, c - wn // 2), min(n, c + wn // 2)
        for lag in range(lmin, lmax + 1):
            end = min(hi, n - lag)
            if end > lo:
                T[w, lag - lmin] = int(np.dot(s[lo:end], s[lo + lag:end + lag])) * int(prior[lag - lmin])
    return T


def tempo_path(T: np.ndarray, p: dict) -> Tuple[np.ndarray, int]:
    """-> (tempo int32 (nW,) lags, the maximum of V's last row)"""
    nw, nl = T.shape
    step, lmin = int(p["lag_step_max"]), p["lag_min"]
    V = T[0].copy()
    bp = np.zeros((nw, nl), np.int64)
    idx = np.arange(nl)
    for w in range(1, nw):
        best, arg = V.copy(), idx.copy()
        for k in range(1, step + 1):                      # the nearest first, the smaller before the larger: only a strictly larger value takes over
            for sgn in (-1, 1):
                j = idx + sgn * k
                ok = (j >= 0) & (j < nl)
                v = np.where(ok, V[np.clip(j, 0, nl - 1)], np.int64(-1))
                take = ok & (v > best)
                best, arg = np.where(take, v, best), np.where(take, j, arg)
        bp[w] = arg
        V = T[w] + best
    lag = int(np.argmax(V))                               # the first maximum: the smallest lag
    tempo = np.zeros(nw, np.int32)
    for w in range(nw - 1, -1, -1):
        tempo[w] = lag + lmin
        lag = int(bp[w, lag])
    return tempo, int(V.max())


def beat_chain(s: np.ndarray, tempo: np.ndarray, pen: np.ndarray, p: dict) -> Tuple[np.ndarray, int]:
    """-> (beats int32 ascending, max C)"""
    n, hn, lmin = s.size, int(p["hop_frames"]), p["lag_min"]
    C = np.zeros(n, np.int64)
    back = np.full(n, -1, np.int64)
    for f in range(n):
        t = int(tempo[min(f // hn, tempo.size - 1)])
        lo, hi = max(0, f - 2 * t), f - (t + 1) // 2
        best = 0
        if hi >= lo:
            cand = C[lo:hi + 1] - pen[t - lmin, f - hi:f - lo + 1][::-1]
            m = int(cand.max())
            if m > 0:
                best = m
                back[f] = lo + int(np.flatnonzero(cand == m)[-1])
        C[f] = 1024 * int(s[f]) + best
    top = int(C.max()) if n else 0
    if top == 0:
        return np.zeros(0, np.int32), 0
    f, chain = int(np.argmax(C)), []
    while f >= 0:
        chain.append(f)
        f = int(back[f])
    return np.array(chain[::-1], np.int32), top


def track_beats(notes, n_frames: int, **params) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The host specification -> (beats int32 (n_beats,) frames ascending, tempo int32 (nW,) lags in frames per beat, one per window,
    result int64 (4,): n_beats, max C, the maximum of V's last row, skipped records).  `notes`: a list of Note or a NOTE_RECORD array, in
    any order; `params`: DEFAULTS' keys."""
    p = check_params(**params)
    check_frames(p, n_frames)
    prior, pen = beat_tables(p)
    s, skipped = onset_envelope(notes, int(n_frames), p)
    tempo, v_max = tempo_path(tempogram(s, p, prior), p)
    beats, top = beat_chain(s, tempo, pen, p)
    return beats, tempo, np.array([beats.size, top, v_max, skipped], np.int64)


def lead_beats(beats) -> int:
    """n0: the whole beats before the first one, so that time 0 has a position >= 0"""
    b0, d = int(beats[0]), int(beats[1]) - int(beats[0])
    return -(-b0 // d)


def beat_positions(notes, beats, frames_per_second: float = 100.0, divisions: int = 0, n_programs: int = DEFAULTS["n_programs"],
                   drum_program: int = DRUM_PROGRAM) -> np.ndarray:
    """The host specification of the positions -> ticks int32 (n, 2): onset and offset tick of every record at TICKS_PER_BEAT per beat,
    snapped to `divisions` steps per beat if that is not 0; -1 for a NaN time or an uncounted record."""
    from .metrics import classify
    q = int(divisions)
    if q < 0 or (q and TICKS_PER_BEAT % q):
        raise ValueError(f"divisions={divisions} must be 0 or a divisor of {TICKS_PER_BEAT}")
    rec = _records(notes)
    b = np.asarray(beats, np.int64)
    counted, _, drum = classify(rec, int(n_programs), int(drum_program))
    fps = np.float64(frames_per_second)
    grid = q or TICKS_PER_BEAT
    step = TICKS_PER_BEAT // grid if b.size >= 2 else 1

    def ticks_of(t):
        t = np.asarray(t, np.float64)
        with np.errstate(all="ignore"):
            if b.size < 2:
                v = np.clip(np.rint(t * np.float64(2 * TICKS_PER_BEAT)), 0.0, float(TICK_FLAT_MAX))
            else:
                x = t * fps
                i = np.clip(np.searchsorted(b.astype(np.float64), x, side="right") - 1, 0, b.size - 2)
                pos = (lead_beats(b) + i).astype(np.float64) + (x - b[i].astype(np.float64)) / (b[i + 1] - b[i]).astype(np.float64)
                v = np.clip(np.rint(pos * np.float64(grid)), 0.0, float(TICK_GRID_MAX)) * np.float64(step)
        return np.where(np.isnan(t), -1, np.nan_to_num(v)).astype(np.int64)

    on, off = ticks_of(rec["onset"]), ticks_of(rec["offset"])
    off = np.where(counted & ~drum, np.maximum(off, on + step), off)
    out = np.stack([on, off], 1)
    out[~counted] = -1
    return out.astype(np.int32)


def tempo_map(beats, frames_per_second: float = 100.0) -> List[Tuple[int, int]]:
    """-> [(tick, microseconds per beat)] of the beats, equal consecutive tempos merged: the first interval's tempo from tick 0, interval
    i's (b[i+1] - b[i] frames) from tick (n0 + i) 480, the last one's to the end.  [] with fewer than two beats."""
    b = [int(v) for v in np.asarray(beats).tolist()]
    if len(b) < 2:
        return []
    n0, out = lead_beats(b), []
    for i in range(len(b) - 1):
        us = min(int(np.rint((b[i + 1] - b[i]) / float(frames_per_second) * 1e6)), 0xFFFFFF)
        if not out or out[-1][1] != us:
            out.append((0 if i == 0 else (n0 + i) * TICKS_PER_BEAT, us))
    return out


def lead_sec(beats, frames_per_second: float = 100.0) -> float:
    """where the audio's time 0 lies in a file written on the beats: less than one beat of lead-in (0 with fewer than two beats)"""
    if len(beats) < 2:
        return 0.0
    return (lead_beats(beats) * (int(beats[1]) - int(beats[0])) - int(beats[0])) / float(frames_per_second)


class BeatTracker(_Owned):
    """The device beat tracker of one model (YourMT3.compile_beat_tracker; include/ymt3.h, beat tracking): the parameters, the two tables
    and scratch for `max_frames` frames on the device.  `params`: DEFAULTS' keys, checked by the C ABI.  Freed by close(), by leaving a
    `with` block, or by the model's close()."""
    _destroy, _noun = "ymt3_beats_destroy", "beat tracker"

    def __init__(self, model, max_frames: int, **params):
        from . import _lib
        self.params = with_defaults(params, DEFAULTS, "beat")
        self.max_frames = int(max_frames)
        self._own(model)
        p = self.params
        c = _lib.BeatParams(*(float(p[k]) for k in ("frames_per_second", "bpm_min", "bpm_max", "bpm_prior", "prior_octaves", "tightness")),
                            *(int(p[k]) for k in ("window_frames", "hop_frames", "lag_step_max", "onset_cap", "n_programs", "drum_program")))
        _lib.check(self._lib.ymt3_beats_create(model._handle, ctypes.byref(c), self.max_frames, ctypes.byref(self._c)))
        fps = float(p["frames_per_second"])
        self.lag_min, self.lag_max = int(math.ceil(60.0 * fps / float(p["bpm_max"]))), int(math.floor(60.0 * fps / float(p["bpm_min"])))

    def track(self, records, n_frames: int, count=None, tempo: bool = True):
        """`records`: NOTE_RECORD bytes (uint8, a multiple of 32), uploaded if they are on the host; `count`: an int32 device tensor whose
        FIRST element is the number of records, read on the device (a Detokenizer.run_device counts tensor as it is).
        -> (beats int32 (max_beats(n_frames),), only the first n_beats written; tempo int32 (nW,) or None; result int64 (4,): n_beats,
        max C, max V, skipped): device tensors.  Asynchronous: nothing is copied back."""
        import torch
        from . import _lib
        from .model import _ptr, _records_side
        model = self._live_model()
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        n_frames = int(n_frames)
        cap = max_beats(max(n_frames, 0), self.lag_min)
        beats = torch.zeros(cap, device=model.device, dtype=torch.int32)
        lags = torch.zeros(n_windows(max(n_frames, 1), self.params["hop_frames"]), device=model.device, dtype=torch.int32) if tempo else None
        result = torch.zeros(4, device=model.device, dtype=torch.int64)
        _lib.check(self._lib.ymt3_track_beats(model._handle, self.ptr, _ptr(rec) if n else None, n, _ptr(cnt), n_frames, _ptr(beats), cap,
                                              _ptr(lags), _ptr(result), model._stream()))
        return beats, lags, result

    def positions(self, beats, result, records, count=None, divisions: int = 0):
        """`beats`, `result`: what track() returned (the number of beats is read from `result` on the device); `records`, `count` as
        track().  -> ticks int32 (n, 2) on the device, -1 at or beyond the count.  Asynchronous."""
        import torch
        from . import _lib
        from .model import _ptr, _records_side
        model = self._live_model()
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        ticks = torch.empty((n, 2), device=model.device, dtype=torch.int32)
        _lib.check(self._lib.ymt3_beat_positions(model._handle, self.ptr, _ptr(beats), _ptr(result), _ptr(rec) if n else None, n, _ptr(cnt),
                                                 int(divisions), _ptr(ticks) if n else None, model._stream()))
        return ticks

    def run(self, records, n_frames: int, count=None, divisions: int = 0):
        """track() and positions() on the same records, then ONE copy back -> (beats int32 (n_beats,), tempo int32 (nW,), result int64
        (4,), ticks int32 (n, 2)) as numpy arrays; without a count, n is the number of records given"""
        import torch
        beats, lags, result = self.track(records, n_frames, count)
        ticks = self.positions(beats, result, records, count, divisions)
        flat = torch.cat([result.view(torch.int32), lags, beats, ticks.view(-1)]).cpu().numpy()
        res = flat[:8].view(np.int64).copy()
        o = 8 + lags.numel()
        return flat[o:o + int(res[0])].copy(), flat[8:o].copy(), res, flat[o + beats.numel():].reshape(-1, 2).copy()


def n_frames_of(end_sec: float, frames_per_second: float) -> int:
    """the frames of `end_sec` seconds: every onset up to the end has one"""
    return max(1, int(math.ceil(float(end_sec) * float(frames_per_second))) + 1)


def beat_summary(beats, tempo, frames_per_second: float) -> dict:
    """what transcribe(beats=True) and estimate_beats add to a result: beats_sec, tempo_bpm (one per window) and lead_sec"""
    fps = float(frames_per_second)
    return {"beats_sec": [int(b) / fps for b in beats], "tempo_bpm": [60.0 * fps / int(t) for t in tempo], "lead_sec": lead_sec(beats, fps)}


def estimate_beats(model, notes_or_mid_path, end_sec: Optional[float] = None, divisions: int = 0, output_path: Optional[str] = None, **params) -> dict:
    """Find the beats of notes that have none: `notes_or_mid_path` (a list of Note, or the path of a flat .mid file) tracked on the device
    (BeatTracker; the rules: this module's docstring).  `end_sec`: the length of the music (None: the last note's end); `params`:
    DEFAULTS' keys.  -> {"beats_sec", "tempo_bpm", "lead_sec", "ticks" (int32 (n, 2), in the notes' order), "midi" (the bytes of the file
    on the beats)}; with `output_path` the bytes are written there too."""
    from .tracking import estimate
    return estimate(model, notes_or_mid_path, end_sec, divisions, output_path, params)[0]
