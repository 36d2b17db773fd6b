"""Bars and key over note records and tracked beats: every beat's metre and place in its bar, the downbeats, the time signatures, one key
per file (include/ymt3.h, bars and key).

The beat tracker (yourmt3_amd/beats.py) gives a tick a musical position; this module gives the file its bar lines and its key.  The
notes' accents, their durations and the change of harmony from beat to beat give the metre, their pitch classes the key.  The rules below
are this repository's own, written from memory and UNVERIFIED against any package.  `track_bars` is their host specification: numpy,
integers throughout.  `BarTracker` is the device object (YourMT3.compile_bar_tracker; yourmt3_amd/csrc/bars.hip), which equals it bit for
bit.  tests/bar_model.py states the same rules as plain loops.

The rules.  fps = frames_per_second, nd = near_div; every division of integers is a floor division.  Inputs: the records, the beats
b[0 .. K) in frames, ascending (beats.track_beats), and n_frames.

  slots     with K >= 2: D[i] = b[i+1] - b[i] for i < K-1, D[K-1] = D[K-2]; lo[0] = b[0] - D[0] / nd, lo[i] = b[i] - D[i-1] / nd for i >= 1
            (strictly ascending: nd >= 2 and two beats are at least a frame apart); hi[i] = lo[i+1], hi[K-1] = b[K-1] + D[K-1] - D[K-1] / nd.
            Slot i is [lo[i], hi[i]).
  accent    the counted records are those of metrics.classify (csrc/note_rule.h); the others are `skipped`.  F = rint(onset fps) in f64.
            A counted record with a finite F inside slot i and F <= b[i] + D[i] / nd adds to a[i]: 1, plus w_kick if it is a drum with
            kick_lo <= pitch <= kick_hi, plus w_long if it is pitched and F(offset) - F >= D[i] (in f64: an infinite offset is long).
            Then a[i] = min(a[i], accent_cap).
  chroma    a counted pitched record's span [F(on), max(F(off), F(on) + 1)), clipped to [0, n_frames) in f64 as metrics._cells clips it,
            adds the number of frames it shares with slot i to c[i][pitch mod 12], for every slot it overlaps, wherever its onset lies.
            sum[i] = the sum of c[i]; n[i][pc] = c[i][pc] 1024 / sum[i] (int64); h[0] = 0, h[i] = sum over pc of |n[i][pc] - n[i-1][pc]|
            if sum[i] and sum[i-1] are positive, else 0.
  salience  d[i] = w_accent a[i] + h[i] <= 1024 255 + 2048; mean_d = (sum of d) / K.
  bar path  states (m, k): m in `metres` in the given order, k = 0 .. m-1 the beat's place in its bar, k = 0 the downbeat.
            r(i, m, 0) = (60 / m) (m - 1) d[i], r(i, m, k > 0) = -(60 / m) d[i]: a whole bar earns 60 (its downbeat's d - the bar's mean d).
            V[0][(m, k)] = r(0, m, k) (k != 0: a pickup of m - k beats); V[i][(m, k > 0)] = V[i-1][(m, k-1)] + r;
            V[i][(m, 0)] = max(V[i-1][(m, m-1)], max over m' != m of V[i-1][(m', m'-1)] - P) + r, P = switch_cost 60 mean_d; ties to
            staying, then to the earliest m' in `metres`.  The end is the first state in state order (the order of `metres`, then k
            ascending) with V[K-1] maximal; the path is followed back from it.  |r| <= 50 263168, so |V| < 2^45 over 2^20 beats.
  key       tot[pc] = sum over i of c[i][pc] (int64); S[mode][t] = sum over pc of tot[pc] T_mode[(pc - t) mod 12] with KEY_MAJOR and
            KEY_MINOR below (the Krumhansl-Kessler profiles, written from memory and UNVERIFIED, centred and scaled to norm 1024: means
            and norms are equal across rotations, so the arg-max of the dot product is the arg-max of the correlation).  key = 12 mode + t
            of the maximum, major before minor, then the smaller t; -1 if the sum of tot is 0.  One key per file.
  outputs   metre[i] = 256 m + k for i < K.  result int64 (8,): n_downbeats, max V[K-1], mean_d, key, the best S, the second-best S (the
            largest among the other 23), skipped, 0.  With K < 2: no metre, no slots, key -1: result = (0, 0, 0, -1, 0, 0, skipped, 0).

Compound metres are tracked at the beat level, modulations not at all: the denominator of every time signature is 4."""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Tuple

import numpy as np

from .beats import TICKS_PER_BEAT, _records, lead_beats, with_defaults
from .model import _Owned
from .task_manager import DRUM_PROGRAM

DEFAULTS = dict(frames_per_second=100.0, metres=(4, 3, 2), near_div=4, accent_cap=15, w_long=1, w_kick=2, kick_lo=35, kick_hi=36, w_accent=64,
                switch_cost=4, n_programs=DRUM_PROGRAM + 2, drum_program=DRUM_PROGRAM)
MAX_FRAMES = 1 << 20
MAX_BEATS, MAX_NOTES = (1 << 20) + 1, 1 << 20
MAX_METRES, MAX_PROGRAMS = 5, 256
KEY_MAJOR = (671, -293, -1, -270, 210, 142, -225, 400, -256, 42, -279, -141)
KEY_MINOR = (671, -263, -48, 428, -284, -46, -299, 266, 69, -261, -94, -138)
_RANGES = (("near_div", 2, 64), ("accent_cap", 1, 255), ("w_long", 0, 15), ("w_kick", 0, 15), ("w_accent", 0, 1024), ("switch_cost", 0, 4096))
_MAJOR_NAMES = ("C", "Db", "D", "Eb", "E", "F", "F#", "G", "Ab", "A", "Bb", "B")
_MINOR_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "Bb", "B")


def check_shared(params: dict, defaults: dict, ranges, noun: str) -> dict:
    """what the bars' and the chords' check_params share -> the parameters with their defaults: the names known, frames_per_second
    finite and positive, every integer of `ranges` inside its range, the programs as the note rule needs them"""
    p = with_defaults(params, defaults, noun)
    if not (math.isfinite(p["frames_per_second"]) and p["frames_per_second"] > 0):
        raise ValueError(f"frames_per_second={p['frames_per_second']} must be finite and > 0")
    for k, lo, hi in ranges:
        if not lo <= int(p[k]) <= hi:
            raise ValueError(f"{k}={p[k]} outside [{lo}, {hi}]")
    if not 1 <= int(p["n_programs"]) <= MAX_PROGRAMS:
        raise ValueError(f"n_programs={p['n_programs']} outside [1, {MAX_PROGRAMS}]")
    if not 0 <= int(p["drum_program"]) < int(p["n_programs"]):
        raise ValueError(f"drum_program={p['drum_program']} outside [0, n_programs={p['n_programs']})")
    return p


def check_params(**params) -> dict:
    """the parameters with their defaults (`metres` as a tuple of ints), refused (ValueError naming the parameter) outside what the C ABI accepts"""
    p = check_shared(params, DEFAULTS, _RANGES, "bar")
    try:
        metres = tuple(int(m) for m in p["metres"])
    except TypeError:
        raise ValueError(f"metres={p['metres']!r} must be a tuple of integers") from None
    if not 1 <= len(metres) <= MAX_METRES:
        raise ValueError(f"metres={metres} must hold 1 to {MAX_METRES} metres")
    if any(not 2 <= m <= 6 for m in metres) or len(set(metres)) != len(metres):
        raise ValueError(f"metres={metres} must be distinct integers in [2, 6]")
    p["metres"] = metres
    if not 0 <= int(p["kick_lo"]) <= int(p["kick_hi"]) <= 127:
        raise ValueError(f"kick_lo={p['kick_lo']}, kick_hi={p['kick_hi']} must satisfy 0 <= kick_lo <= kick_hi <= 127")
    return p


def check_sizes(max_beats: int, max_notes: int) -> None:
    if not 1 <= int(max_beats) <= MAX_BEATS:
        raise ValueError(f"max_beats={max_beats} outside [1, {MAX_BEATS}]")
    if not 1 <= int(max_notes) <= MAX_NOTES:
        raise ValueError(f"max_notes={max_notes} outside [1, {MAX_NOTES}]")


def slot_edges(beats, near_div: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (D int64 (K,), the slots' edges int64 (K + 1,): lo[0 .. K) and hi[K-1]) of K >= 2 beats"""
    b = np.asarray(beats, np.int64)
    d = np.empty(b.size, np.int64)
    d[:-1] = np.diff(b)
    d[-1] = d[-2]
    e = np.empty(b.size + 1, np.int64)
    e[0] = b[0] - d[0] // near_div
    e[1:-1] = b[1:] - d[:-1] // near_div
    e[-1] = b[-1] + d[-1] - d[-1] // near_div
    return d, e


def pitched_spans(rec, drum, n_frames: int, fps: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """the counted records `rec` (`drum`: which of them are drums) -> (lo, hi, pitch) int64 of the pitched ones whose span
    [F(on), max(F(off), F(on) + 1)), clipped to [0, n_frames) in f64, is not empty"""
    from .metrics import frame_of
    rec = rec[~drum]
    f_on, f_off = frame_of(rec["onset"], fps), frame_of(rec["offset"], fps)
    lo, hi = np.maximum(f_on, 0.0), np.minimum(np.maximum(f_off, f_on + 1.0), np.float64(n_frames))
    some = lo < hi
    return lo[some].astype(np.int64), hi[some].astype(np.int64), rec["pitch"][some].astype(np.int64)


def share_spans(lo, hi, pitch, e, each=None) -> np.ndarray:
    """the spans [lo, hi) shared out among the slots of edges `e` -> c int64 (K, 12): the frames every span shares with slot s, added to
    c[s][pitch mod 12].  `each(s, ok, share)`: called per slot with the spans that overlap it and every span's share."""
    c = np.zeros((e.size - 1, 12), np.int64)
    for s in range(e.size - 1):
        share = np.minimum(hi, e[s + 1]) - np.maximum(lo, e[s])
        ok = share > 0
        c[s] += np.bincount(pitch[ok] % 12, weights=share[ok], minlength=12).astype(np.int64)
        if each is not None:
            each(s, ok, share)
    return c


def bar_features(notes, beats, n_frames: int, p: dict) -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (a int64 (K,) before the cap, c int64 (K, 12), the number of skipped records); K >= 2"""
    from .metrics import classify, frame_of
    rec = _records(notes)
    b = np.asarray(beats, np.int64)
    K, nd, fps = b.size, int(p["near_div"]), float(p["frames_per_second"])
    d, e = slot_edges(b, nd)
    counted, _, drum = classify(rec, int(p["n_programs"]), int(p["drum_program"]))
    rec, drum = rec[counted], drum[counted]
    f_on = frame_of(rec["onset"], fps)
    f_off = frame_of(np.where(drum, 0.0, rec["offset"]), fps)
    pitch = rec["pitch"].astype(np.int64)
    # accents: the onset's frame is finite and inside a slot, near its beat
    inside = np.isfinite(f_on) & (f_on >= np.float64(e[0])) & (f_on < np.float64(e[-1]))
    fi = f_on[inside].astype(np.int64)
    i = np.searchsorted(e, fi, side="right") - 1
    near = fi <= b[i] + d[i] // nd
    i, fi = i[near], fi[near]
    dr, pt = drum[inside][near], pitch[inside][near]
    with np.errstate(invalid="ignore"):
        long_ = ~dr & (f_off[inside][near] - fi.astype(np.float64) >= d[i].astype(np.float64))
    w = 1 + np.where(dr & (pt >= int(p["kick_lo"])) & (pt <= int(p["kick_hi"])), int(p["w_kick"]), 0) + np.where(long_, int(p["w_long"]), 0)
    a = np.bincount(i, weights=w, minlength=K).astype(np.int64)
    # chroma: the pitched records' spans, shared out among the slots
    return a, share_spans(*pitched_spans(rec, drum, n_frames, fps), e), int((~counted).sum())


def salience(a: np.ndarray, c: np.ndarray, p: dict) -> np.ndarray:
    """-> d int64 (K,)"""
    total = c.sum(1)
    n = c * 1024 // np.maximum(total, 1)[:, None]
    h = np.zeros(a.size, np.int64)
    h[1:] = np.where((total[1:] > 0) & (total[:-1] > 0), np.abs(n[1:] - n[:-1]).sum(1), 0)
    return int(p["w_accent"]) * np.minimum(a, int(p["accent_cap"])) + h


def bar_states(metres) -> List[Tuple[int, int]]:
    return [(m, k) for m in metres for k in range(m)]


def bar_path(d: np.ndarray, p: dict) -> Tuple[np.ndarray, int, int]:
    """-> (metre int32 (K,), max V[K-1], mean_d)"""
    metres = p["metres"]
    states = bar_states(metres)
    K, nS, nM = d.size, len(states), len(metres)
    mean_d = int(d.sum()) // K
    P = int(p["switch_cost"]) * 60 * mean_d
    gain = np.array([(60 // m) * (m - 1) if k == 0 else -(60 // m) for m, k in states], np.int64)
    first = np.array([states.index((m, 0)) for m in metres])
    last = first + np.array(metres) - 1
    inner = np.array([s for s, (m, k) in enumerate(states) if k > 0], np.int64)
    V = gain * int(d[0])
    choice = np.zeros((K, nM), np.int8)
    for i in range(1, K):
        ends = V[last]
        new = np.empty(nS, np.int64)
        new[inner] = V[inner - 1]
        for q in range(nM):
            best, arg = ends[q], q
            for q2 in range(nM):                                   # only a strictly larger value takes over: staying, then the earliest m'
                if q2 != q and ends[q2] - P > best:
                    best, arg = ends[q2] - P, q2
            new[first[q]], choice[i, q] = best, arg
        V = new + gain * int(d[i])
    s = int(np.argmax(V))                                          # the first maximum in state order
    top = int(V[s])
    metre = np.zeros(K, np.int32)
    for i in range(K - 1, -1, -1):
        m, k = states[s]
        metre[i] = 256 * m + k
        s = s - 1 if k else int(last[choice[i, metres.index(m)]])
    return metre, top, mean_d


def key_of(tot) -> Tuple[int, int, int]:
    """-> (key, the best S, the second-best S) of the twelve pitch-class totals"""
    tot = [int(v) for v in tot]
    if sum(tot) == 0:
        return -1, 0, 0
    S = [sum(tot[pc] * table[(pc - t) % 12] for pc in range(12)) for table in (KEY_MAJOR, KEY_MINOR) for t in range(12)]
    key = max(range(24), key=lambda j: (S[j], -j))
    return key, S[key], max(S[j] for j in range(24) if j != key)


def check_inputs(notes, beats, n_frames: int, p: dict, metre=None) -> Tuple[np.ndarray, np.ndarray, Optional[int]]:
    """what track_bars and track_chords ask of their inputs -> (the records, the beats int64, with fewer than two beats the number of
    skipped records: all that is left to report then)"""
    from .metrics import classify
    if not 1 <= int(n_frames) <= MAX_FRAMES:
        raise ValueError(f"n_frames={n_frames} outside [1, {MAX_FRAMES}]")
    rec = _records(notes)
    b = np.asarray(beats, np.int64)
    if rec.size > MAX_NOTES:
        raise ValueError(f"{rec.size} notes: at most {MAX_NOTES}")
    if b.size > MAX_BEATS:
        raise ValueError(f"{b.size} beats: at most {MAX_BEATS}")
    if metre is not None and len(metre) < b.size:
        raise ValueError(f"{len(metre)} metre entries for {b.size} beats")
    if b.size < 2:
        return rec, b, int((~classify(rec, int(p["n_programs"]), int(p["drum_program"]))[0]).sum())
    if not bool(np.all(np.diff(b) > 0)):
        raise ValueError("beats must ascend strictly")
    return rec, b, None


def track_bars(notes, beats, n_frames: int, **params) -> Tuple[np.ndarray, np.ndarray]:
    """The host specification -> (metre int32 (K,): 256 m + k of every beat, result int64 (8,): n_downbeats, max V[K-1], mean_d, key,
    the best S, the second-best S, skipped records, 0).  `notes`: a list of Note or a NOTE_RECORD array, in any order; `beats`: the
    beats' frames, ascending (beats.track_beats); `params`: DEFAULTS' keys."""
    p = check_params(**params)
    rec, b, skipped = check_inputs(notes, beats, n_frames, p)
    if b.size < 2:
        return np.zeros(0, np.int32), np.array([0, 0, 0, -1, 0, 0, skipped, 0], np.int64)
    a, c, skipped = bar_features(rec, b, int(n_frames), p)
    metre, top, mean_d = bar_path(salience(a, c, p), p)
    key, best, second = key_of(c.sum(0))
    return metre, np.array([int(((metre & 255) == 0).sum()), top, mean_d, key, best, second, skipped, 0], np.int64)


def bar_list(metre, beats=None) -> List[Tuple[int, int, int]]:
    """the bars of a tracked file -> [(first beat index, length in beats, m)]; the first and the last may be short"""
    mk = [int(v) for v in np.asarray(metre).tolist()]
    starts = [i for i, v in enumerate(mk) if i == 0 or v & 255 == 0]
    return [(s, (starts[j + 1] if j + 1 < len(starts) else len(mk)) - s, mk[s] >> 8) for j, s in enumerate(starts)]


def metre_runs(metre) -> List[Tuple[int, int]]:
    """-> [(m, the number of downbeats in a row under it)]"""
    out: List[List[int]] = []
    for v in np.asarray(metre).tolist():
        if v & 255 == 0:
            if out and out[-1][0] == v >> 8:
                out[-1][1] += 1
            else:
                out.append([v >> 8, 1])
    return [tuple(r) for r in out]


def time_signatures(metre, beats) -> List[Tuple[int, int]]:
    """-> [(tick, numerator)] over the denominator 4, in the layout of a file on the beats (beat i at tick (n0 + i) 480): with the first
    downbeat i0 under m0 and r = (n0 + i0) mod m0, a bar of r/4 at tick 0 and m0/4 at tick 480 r if r > 0, else m0/4 at tick 0; then one
    event at every downbeat whose m differs from the bar before.  [] without downbeats."""
    mk = [int(v) for v in np.asarray(metre).tolist()]
    downs = [i for i, v in enumerate(mk) if v & 255 == 0]
    if not downs or len(beats) < 2:
        return []
    n0, i0 = lead_beats(beats), downs[0]
    m = mk[i0] >> 8
    r = (n0 + i0) % m
    out = [(0, r), (r * TICKS_PER_BEAT, m)] if r else [(0, m)]
    for i in downs[1:]:
        if mk[i] >> 8 != m:
            m = mk[i] >> 8
            out.append(((n0 + i) * TICKS_PER_BEAT, m))
    return out


def key_name(key: int) -> str:
    """e.g. 21 -> "A minor"; -1 -> "none" """
    key = int(key)
    if key < 0:
        return "none"
    if key >= 24:
        raise ValueError(f"key={key} outside [-1, 24)")
    return f"{(_MINOR_NAMES if key >= 12 else _MAJOR_NAMES)[key % 12]} {'minor' if key >= 12 else 'major'}"


def key_signature(key: int) -> Tuple[int, int]:
    """-> (sf, mi) of MIDI's FF 59: sf sharps (negative: flats), mi 1 for minor.  A major tonic t has sf = 7 t mod 12, minus 12 above 6; a
    minor key takes its relative major's."""
    key = int(key)
    if not 0 <= key < 24:
        raise ValueError(f"key={key} outside [0, 24)")
    mi, t = divmod(key, 12)
    sf = 7 * ((t + 3) % 12 if mi else t) % 12
    return (sf - 12 if sf > 6 else sf), mi


class BarTracker(_Owned):
    """The device bar tracker of one model (YourMT3.compile_bar_tracker; include/ymt3.h, bars and key): the parameters and scratch for
    `max_beats` beats on the device; a call takes at most `max_notes` records.  `params`: DEFAULTS' keys, checked by the C ABI.  Freed by
    close(), by leaving a `with` block, or by the model's close()."""
    _destroy, _noun = "ymt3_bars_destroy", "bar tracker"

    def __init__(self, model, max_beats: int, max_notes: int, **params):
        from . import _lib
        self.params = p = with_defaults(params, DEFAULTS, "bar")
        metres = tuple(int(m) for m in p["metres"])
        if not 1 <= len(metres) <= MAX_METRES:
            raise ValueError(f"metres={metres} must hold 1 to {MAX_METRES} metres")
        self.max_beats, self.max_notes = int(max_beats), int(max_notes)
        self._own(model)
        c = _lib.BarParams(float(p["frames_per_second"]), len(metres), (ctypes.c_int32 * MAX_METRES)(*metres),
                           *(int(p[k]) for k in ("near_div", "accent_cap", "w_long", "w_kick", "kick_lo", "kick_hi", "w_accent", "switch_cost",
                                                 "n_programs", "drum_program")))
        _lib.check(self._lib.ymt3_bars_create(model._handle, ctypes.byref(c), self.max_beats, self.max_notes, ctypes.byref(self._c)))

    def track(self, beats, beat_result, records, n_frames: int, count=None):
        """`beats`, `beat_result`: what BeatTracker.track returned, device tensors (the number of beats is read from `beat_result` on the
        device); `records`, `count` as BeatTracker.track.  -> (metre int32 (max_beats,), only the first n_beats written; result int64
        (8,)): device tensors.  Asynchronous: nothing is copied back."""
        import torch
        from . import _lib
        from .model import _ptr, _records_side
        model = self._live_model()
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        metre = torch.zeros(self.max_beats, device=model.device, dtype=torch.int32)
        result = torch.zeros(8, device=model.device, dtype=torch.int64)
        _lib.check(self._lib.ymt3_track_bars(model._handle, self.ptr, _ptr(beats), _ptr(beat_result), _ptr(rec) if n else None, n, _ptr(cnt),
                                             int(n_frames), _ptr(metre), self.max_beats, _ptr(result), model._stream()))
        return metre, result

    def run(self, beats, records, n_frames: int, count=None):
        """`beats`: the beats' frames (a sequence or an int32 tensor, uploaded if on the host), all of them live.  track(), then ONE copy
        back -> (metre int32 (n_beats,), result int64 (8,)) as numpy arrays"""
        return run_on_beats(self, beats, lambda b, beat_result, k: self.track(b, beat_result, records, n_frames, count))


def _to_device(device, x):
    import torch
    return torch.as_tensor(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, np.int32)).to(device)


def run_on_beats(tracker, beats, track) -> Tuple[np.ndarray, np.ndarray]:
    """What BarTracker.run and ChordTracker.run share: `beats` go up (one zero where there are none: the kernels take no null) with a
    beat tracker's result that says their number k, `track(b, beat_result, k)` gives the per-beat output and the result on the device,
    then ONE copy back -> (the per-beat output int32 (k,), none with fewer than two beats; result int64 (8,))"""
    import torch
    device = tracker._live_model().device
    b = _to_device(device, beats)
    k = int(b.numel())
    if k > tracker.max_beats:
        raise ValueError(f"{k} beats: the {tracker._noun} was made for max_beats={tracker.max_beats}")
    per_beat, result = track(b if k else torch.zeros(1, dtype=torch.int32, device=device), torch.tensor([k, 0, 0, 0], dtype=torch.int64).to(device), k)
    flat = torch.cat([result.view(torch.int32), per_beat[:k]]).cpu().numpy()
    return flat[16:16 + (k if k >= 2 else 0)].copy(), flat[:16].view(np.int64).copy()


def bar_summary(metre, result, beats, frames_per_second: float) -> dict:
    """what transcribe(bars=True) and estimate_bars add to a result: downbeats_sec, time_signatures ([(tick, numerator)]), key (its name),
    key_margin (the best S minus the second-best)"""
    fps = float(frames_per_second)
    return {"downbeats_sec": [int(b) / fps for b, v in zip(beats, np.asarray(metre).tolist()) if v & 255 == 0],
            "time_signatures": time_signatures(metre, beats), "key": key_name(int(result[3])), "key_margin": int(result[4]) - int(result[5])}


def estimate_bars(model, notes_or_mid_path, end_sec: Optional[float] = None, divisions: int = 0, output_path: Optional[str] = None,
                  beat_params: Optional[dict] = None, **params) -> dict:
    """Find the beats, the bars and the key of notes that have none: `notes_or_mid_path` (a list of Note, or the path of a flat .mid file)
    tracked on the device (BeatTracker, then BarTracker; the rules: this module's docstring).  `end_sec`: the length of the music (None:
    the last note's end); `beat_params`: beats.DEFAULTS' keys; `params`: DEFAULTS' keys.  -> estimate_beats' dict plus {"downbeats_sec",
    "time_signatures", "key", "key_margin", "metre" (int32 (n_beats,))}, "midi" being the bytes of the file on the bars; with `output_path`
    the bytes are written there too."""
    from .tracking import estimate
    out, tracked = estimate(model, notes_or_mid_path, end_sec, divisions, output_path, beat_params, params)
    out["metre"] = tracked["metre"]
    return out
