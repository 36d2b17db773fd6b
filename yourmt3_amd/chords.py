"""Chords over note records and tracked beats: one chord per beat, the runs of equal chords, lead-sheet markers for the MIDI file
(include/ymt3.h, chords).

The bar tracker (yourmt3_amd/bars.py) gives the file its bar lines and one key; this module gives every beat a chord symbol.  A beat's
pitch-class content is matched against chord templates, its lowest long note says which root is in the bass, and a smoothing path keeps a
chord until the evidence against it pays for a change.  The rules below are this repository's own, written from memory and UNVERIFIED
against any package.  `track_chords` is their host specification: numpy, integers throughout.  `ChordTracker` is the device object
(YourMT3.compile_chord_tracker; yourmt3_amd/csrc/chords.hip), which equals it bit for bit.  tests/chord_model.py states the same rules as
plain loops.

The rules.  fps = frames_per_second, nd = near_div; every division of integers is a floor division.  Inputs: the records, the beats
b[0 .. K) in frames, ascending (beats.track_beats), optionally the bar tracker's metre (256 m + k per beat), and n_frames.

  table     quality q of QUALITIES has the intervals INTERVALS[q]: 0 maj {0,4,7}, 1 min {0,3,7}, 2 dim {0,3,6}, 3 aug {0,4,8}, 4 sus4 {0,5,7},
            5 "7" {0,4,7,10}, 6 maj7 {0,4,7,11}, 7 min7 {0,3,7,10}.  W_q = 591 for three tones, 512 for four: 1024 / sqrt(n), so a bare
            triad beats its seventh chords and a sounded seventh beats the triad.
  slots     bars.slot_edges, unchanged: K >= 2, slot i is [lo[i], hi[i]).
  chroma    c[i][pc] is the bar tracker's: a counted (metrics.classify) pitched record's span [F(on), max(F(off), F(on) + 1)), clipped to
            [0, n_frames) in f64, adds the frames it shares with slot i to c[i][pitch mod 12], for every slot it overlaps.
            n[i][pc] = c[i][pc] 1024 / max(sum of c[i], 1): the product needs 64 bits.
  bass      bass[i] = the smallest pitch among the counted pitched records whose share with slot i satisfies
            bass_div share >= hi[i] - lo[i]; 255 with none.  A passing low eighth does not take it.
  states    (q, r) for q in `qualities`' order and r = 0 .. 11, then N (no chord) last: S = 12 |qualities| + 1 <= 97.
  emission  e[i][(q, r)] = W_q (sum over s in INTERVALS[q] of n[i][(r + s) mod 12]) + (1024 w_bass if bass[i] < 128 and bass[i] mod 12 = r);
            e[i][N] = 1024 w_none.  The n of a beat sum to at most 1024: e <= 591 1024 + 1024 1024 < 2^21.
  path      V[0] = e[0].  For i >= 1: j* = the first state with V[i-1] maximal; P_i = 1024 change_cost_down if a metre is given and
            metre[i] & 255 = 0, else 1024 change_cost; jump = V[i-1][j*] - P_i; state s stays if V[i-1][s] >= jump, else it comes from j*;
            V[i][s] = max(V[i-1][s], jump) + e[i][s].  0 <= V < 2^41 + 2^21 over 2^20 + 1 beats.  The end is the first state with V[K-1]
            maximal; the path is followed back.  Every state's predecessor is itself or the one j*.
  outputs   chord[i] = 256 bass[i] + label for i < K; label = 12 q + r with q the index in QUALITIES (so codes do not depend on
            `qualities`), 255 for N.  result int64 (8,): the number of runs of equal label, max V[K-1], the number of N beats, skipped
            records, 0, 0, 0, 0.  With K < 2: no chord, result = (0, 0, 0, skipped, 0, 0, 0, 0).

One chord per beat at the finest: changes inside a beat, chords beyond the eight qualities and enharmonic spelling by key are out of scope."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .bars import (MAX_BEATS, MAX_FRAMES, MAX_NOTES, MAX_PROGRAMS, _MAJOR_NAMES, _records, _to_device, check_inputs, check_shared,  # noqa: F401
                   check_sizes, pitched_spans, run_on_beats, share_spans, slot_edges)  # (the sizes and the slot rule are the bars')
from .beats import TICKS_PER_BEAT, lead_beats, with_defaults
from .model import _Owned
from .task_manager import DRUM_PROGRAM

QUALITIES = ("maj", "min", "dim", "aug", "sus4", "7", "maj7", "min7")
INTERVALS = ((0, 4, 7), (0, 3, 7), (0, 3, 6), (0, 4, 8), (0, 5, 7), (0, 4, 7, 10), (0, 4, 7, 11), (0, 3, 7, 10))
WEIGHTS = tuple(591 if len(t) == 3 else 512 for t in INTERVALS)
_SUFFIX = ("", "m", "dim", "aug", "sus4", "7", "maj7", "m7")
NO_CHORD, NO_BASS = 255, 255
DEFAULTS = dict(frames_per_second=100.0, near_div=4, qualities=QUALITIES, bass_div=2, w_bass=64, w_none=300, change_cost=160, change_cost_down=48,
                n_programs=DRUM_PROGRAM + 2, drum_program=DRUM_PROGRAM)
_RANGES = (("near_div", 2, 64), ("bass_div", 1, 64), ("w_bass", 0, 1024), ("w_none", 0, 1024), ("change_cost", 0, 4096), ("change_cost_down", 0, 4096))


def check_params(**params) -> dict:
    """the parameters with their defaults (`qualities` as a tuple of names), refused (ValueError naming the parameter) outside what the C ABI accepts"""
    p = check_shared(params, DEFAULTS, _RANGES, "chord")
    q = p["qualities"]
    if isinstance(q, str) or not isinstance(q, (tuple, list)):
        raise ValueError(f"qualities={q!r} must be a tuple of names")
    q = tuple(q)
    if not 1 <= len(q) <= len(QUALITIES):
        raise ValueError(f"qualities={q} must hold 1 to {len(QUALITIES)} names")
    if any(name not in QUALITIES for name in q) or len(set(q)) != len(q):
        raise ValueError(f"qualities={q} must be distinct names of {QUALITIES}")
    p["qualities"] = q
    return p


def chord_features(notes, beats, n_frames: int, p: dict) -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (c int64 (K, 12), bass int64 (K,), the number of skipped records); K >= 2"""
    from .metrics import classify
    rec = _records(notes)
    b = np.asarray(beats, np.int64)
    _, e = slot_edges(b, int(p["near_div"]))
    counted, _, drum = classify(rec, int(p["n_programs"]), int(p["drum_program"]))
    lo, hi, pitch = pitched_spans(rec[counted], drum[counted], n_frames, float(p["frames_per_second"]))
    bass = np.full(b.size, NO_BASS, np.int64)

    def lowest_long(s, ok, share):
        long_ = ok & (int(p["bass_div"]) * share >= e[s + 1] - e[s])
        if long_.any():
            bass[s] = pitch[long_].min()

    return share_spans(lo, hi, pitch, e, lowest_long), bass, int((~counted).sum())


def chord_states(qualities) -> List[Tuple[int, int]]:
    """-> [(q the index in QUALITIES, r)] of every state but N, which is last"""
    return [(QUALITIES.index(name), r) for name in qualities for r in range(12)]


def emissions(c: np.ndarray, bass: np.ndarray, p: dict) -> np.ndarray:
    """-> e int64 (K, S)"""
    n = c * 1024 // np.maximum(c.sum(1), 1)[:, None]
    states = chord_states(p["qualities"])
    e = np.empty((c.shape[0], len(states) + 1), np.int64)
    for s, (q, r) in enumerate(states):
        e[:, s] = WEIGHTS[q] * sum(n[:, (r + t) % 12] for t in INTERVALS[q]) + np.where((bass < 128) & (bass % 12 == r), 1024 * int(p["w_bass"]), 0)
    e[:, -1] = 1024 * int(p["w_none"])
    return e


def chord_path(e: np.ndarray, metre, p: dict) -> Tuple[np.ndarray, int]:
    """-> (the state of every beat int64 (K,), max V[K-1])"""
    K, S = e.shape
    V = e[0].copy()
    stay, best = np.ones((K, S), bool), np.zeros(K, np.int64)
    for i in range(1, K):
        j = int(np.argmax(V))                                              # the first maximum
        down = metre is not None and int(metre[i]) & 255 == 0
        jump = int(V[j]) - 1024 * int(p["change_cost_down"] if down else p["change_cost"])
        stay[i], best[i] = V >= jump, j
        V = np.maximum(V, jump) + e[i]
    s = int(np.argmax(V))
    top, path = int(V[s]), np.empty(K, np.int64)
    for i in range(K - 1, -1, -1):
        path[i] = s
        if i and not stay[i, s]:
            s = int(best[i])
    return path, top


def track_chords(notes, beats, n_frames: int, metre=None, **params) -> Tuple[np.ndarray, np.ndarray]:
    """The host specification -> (chord int32 (K,): 256 bass + label of every beat, result int64 (8,): runs, max V[K-1], N beats, skipped
    records, 0, 0, 0, 0).  `notes`: a list of Note or a NOTE_RECORD array, in any order; `beats`: the beats' frames, ascending
    (beats.track_beats); `metre`: bars.track_bars' metre of the same beats, or None; `params`: DEFAULTS' keys."""
    p = check_params(**params)
    rec, b, skipped = check_inputs(notes, beats, n_frames, p, metre)
    if b.size < 2:
        return np.zeros(0, np.int32), np.array([0, 0, 0, skipped, 0, 0, 0, 0], np.int64)
    c, bass, skipped = chord_features(rec, b, int(n_frames), p)
    path, top = chord_path(emissions(c, bass, p), metre, p)
    states = chord_states(p["qualities"])
    label = np.array([12 * q + r for q, r in states] + [NO_CHORD], np.int64)[path]
    runs = 1 + int((label[1:] != label[:-1]).sum())
    return (256 * bass + label).astype(np.int32), np.array([runs, top, int((label == NO_CHORD).sum()), skipped, 0, 0, 0, 0], np.int64)


def chord_segments(chord, beats) -> List[Tuple[int, int, int, int]]:
    """the runs of equal label -> [(first beat, end beat (exclusive), label, the bass of the run's first beat)]"""
    v = [int(x) for x in np.asarray(chord).tolist()]
    if len(v) > len(beats):
        raise ValueError(f"{len(v)} chords for {len(beats)} beats")
    out: List[List[int]] = []
    for i, x in enumerate(v):
        if out and out[-1][2] == x & 255:
            out[-1][1] = i + 1
        else:
            out.append([i, i + 1, x & 255, x >> 8])
    return [tuple(r) for r in out]


def chord_name(label: int, bass: int = NO_BASS) -> str:
    """e.g. (0, 255) -> "C", (21, 255) -> "Am", (67, 255) -> "G7", (0, 52) -> "C/E"; 255 -> "N".  The bass is named when its pitch class
    differs from the root and is a chord tone; spelling as bars.key_name's major tonics."""
    label, bass = int(label), int(bass)
    if label == NO_CHORD:
        return "N"
    if not 0 <= label < 12 * len(QUALITIES):
        raise ValueError(f"label={label} outside [0, {12 * len(QUALITIES)}) and not {NO_CHORD}")
    q, r = divmod(label, 12)
    name = _MAJOR_NAMES[r] + _SUFFIX[q]
    if 0 <= bass < 128 and bass % 12 != r and (bass - r) % 12 in INTERVALS[q]:
        name += "/" + _MAJOR_NAMES[bass % 12]
    return name


def harte_label(label: int) -> str:
    """e.g. 0 -> "C:maj", 93 -> "A:min7", 255 -> "N" """
    label = int(label)
    if label == NO_CHORD:
        return "N"
    if not 0 <= label < 12 * len(QUALITIES):
        raise ValueError(f"label={label} outside [0, {12 * len(QUALITIES)}) and not {NO_CHORD}")
    return f"{_MAJOR_NAMES[label % 12]}:{QUALITIES[label // 12]}"


def _edge_sec(beats, i: int, fps: float) -> float:
    """the time of beat i; of one beat after the last for i = K"""
    b = [int(x) for x in beats]
    return (b[i] if i < len(b) else b[-1] + (b[-1] - b[-2] if len(b) > 1 else 0)) / fps


def chord_lab(segments, beats, fps: float = 100.0) -> str:
    """the text of a .lab file: one line `start_sec end_sec label` per run, labels as harte_label; a run ends where the next begins, the
    last one a beat after the last beat"""
    return "".join(f"{_edge_sec(beats, s, fps):.3f} {_edge_sec(beats, e, fps):.3f} {harte_label(label)}\n" for s, e, label, _ in segments)


def chord_markers(segments, beats) -> List[Tuple[int, str]]:
    """-> [(tick, name)] for midi's writers on the beats: every run's name at the tick of its first beat, (n0 + i) 480"""
    if len(beats) < 2:
        return []
    n0 = lead_beats(beats)
    return [((n0 + s) * TICKS_PER_BEAT, chord_name(label, bass)) for s, _, label, bass in segments]


def chord_summary(chord, result, beats, frames_per_second: float) -> dict:
    """what transcribe(chords=True) and estimate_chords add to a result: chords ([(start_sec, end_sec, name)], one per run) and chord_labels
    (every beat's label: 12 q + r, 255 for N)"""
    fps = float(frames_per_second)
    seg = chord_segments(chord, beats)
    return {"chords": [(_edge_sec(beats, s, fps), _edge_sec(beats, e, fps), chord_name(label, bass)) for s, e, label, bass in seg],
            "chord_labels": [int(x) & 255 for x in np.asarray(chord).tolist()]}


class ChordTracker(_Owned):
    """The device chord tracker of one model (YourMT3.compile_chord_tracker; include/ymt3.h, chords): the parameters and scratch for
    `max_beats` beats on the device; a call takes at most `max_notes` records.  `params`: DEFAULTS' keys, checked by the C ABI.  Freed by
    close(), by leaving a `with` block, or by the model's close()."""
    _destroy, _noun = "ymt3_chords_destroy", "chord tracker"

    def __init__(self, model, max_beats: int, max_notes: int, **params):
        from . import _lib
        self.params = p = with_defaults(params, DEFAULTS, "chord")
        names = tuple(p["qualities"])
        if isinstance(p["qualities"], str) or not 1 <= len(names) <= len(QUALITIES) or any(n not in QUALITIES for n in names):
            raise ValueError(f"qualities={p['qualities']!r} must hold 1 to {len(QUALITIES)} names of {QUALITIES}")
        self.max_beats, self.max_notes = int(max_beats), int(max_notes)
        self._own(model)
        c = _lib.ChordParams(float(p["frames_per_second"]), len(names), (ctypes.c_int32 * len(QUALITIES))(*(QUALITIES.index(n) for n in names)),
                             *(int(p[k]) for k in ("near_div", "bass_div", "w_bass", "w_none", "change_cost", "change_cost_down", "n_programs", "drum_program")))
        _lib.check(self._lib.ymt3_chords_create(model._handle, ctypes.byref(c), self.max_beats, self.max_notes, ctypes.byref(self._c)))

    def track(self, beats, beat_result, metre, records, n_frames: int, count=None):
        """`beats`, `beat_result`: what BeatTracker.track returned, device tensors (the number of beats is read from `beat_result` on the
        device); `metre`: what BarTracker.track returned, or None; `records`, `count` as BeatTracker.track.  -> (chord int32 (max_beats,),
        only the first n_beats written; result int64 (8,)): device tensors.  Asynchronous: nothing is copied back."""
        import torch
        from . import _lib
        from .model import _ptr, _records_side
        model = self._live_model()
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        chord = torch.zeros(self.max_beats, device=model.device, dtype=torch.int32)
        result = torch.zeros(8, device=model.device, dtype=torch.int64)
        _lib.check(self._lib.ymt3_track_chords(model._handle, self.ptr, _ptr(beats), _ptr(beat_result), _ptr(metre), _ptr(rec) if n else None, n,
                                               _ptr(cnt), int(n_frames), _ptr(chord), self.max_beats, _ptr(result), model._stream()))
        return chord, result

    def run(self, beats, records, n_frames: int, metre=None, count=None):
        """`beats`: the beats' frames, `metre`: their metre or None (sequences or int32 tensors, uploaded if on the host), all of them
        live.  track(), then ONE copy back -> (chord int32 (n_beats,), result int64 (8,)) as numpy arrays"""
        def track(b, beat_result, k):
            m = None
            if metre is not None and k >= 2:
                m = _to_device(b.device, metre)
                if int(m.numel()) < k:
                    raise ValueError(f"{int(m.numel())} metre entries for {k} beats")
            return self.track(b, beat_result, m, records, n_frames, count)

        return run_on_beats(self, beats, track)


def estimate_chords(model, notes_or_mid_path, end_sec: Optional[float] = None, divisions: int = 0, output_path: Optional[str] = None,
                    lab_path: Optional[str] = None, beat_params: Optional[dict] = None, bar_params: Optional[dict] = None, **params) -> dict:
    """Find the beats, the bars, the key and the chords of notes that have none: `notes_or_mid_path` (a list of Note, or the path of a flat
    .mid file) tracked on the device (BeatTracker, BarTracker, then ChordTracker with the bars' metre; the rules: this module's docstring).
    `end_sec`, `divisions`, `beat_params` as estimate_bars; `bar_params`: bars.DEFAULTS' keys; `params`: DEFAULTS' keys.  -> estimate_bars'
    dict plus {"chords", "chord_labels", "chord" (int32 (n_beats,)), "lab" (the text of a .lab file)}, "midi" being the bytes of the file
    on the bars with one marker per chord; with `output_path` / `lab_path` the bytes and the text are written there too."""
    from .tracking import beats_fps, estimate
    out, tracked = estimate(model, notes_or_mid_path, end_sec, divisions, output_path, beat_params, dict(bar_params or {}), params)
    out.update(metre=tracked["metre"], chord=tracked["chord"],
               lab=chord_lab(chord_segments(tracked["chord"], tracked["beats"]), tracked["beats"], beats_fps(beat_params)))
    if lab_path is not None:
        with open(lab_path, "w") as f:
            f.write(out["lab"])
    return out
